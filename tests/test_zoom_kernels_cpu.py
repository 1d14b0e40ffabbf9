"""Zoom kernels (arco_amd/csrc/zoom.hip, arco_amd/utils/zoom_gpu.py), the part that needs no GPU:
  reference     ref_zoom of tests/zoom_kernel_refs.py equals scipy.ndimage.zoom(order=0) on every case, both directions, float32 and int64
  cases         what each case is there for actually holds (the zeroed last rows / columns, the .5 ties)
  checkers      the canary check rejects a planted write on either side
  C ABI         the two entry points are exported; ARCO_ERR_ARG on the host for every rejection of include/arco_hip.h
  rejections    check_zoom, test_single_volume(zoom="gpu", surface="host"), an output axis of one point, a host or float64 tensor -
                all raised before any GPU call (there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

import zoom_kernel_refs as R


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
@pytest.mark.parametrize("direction", ["fwd", "back"])
def test_ref_zoom_is_scipy(case, direction):
    dst = R.target(case, direction)
    for a in (R.image(case, direction), R.labels(case, direction)):
        assert a.shape[0] == R.slices(case) and (a != 0).all()
        got = R.ref_zoom(a, dst)
        assert got.dtype == a.dtype and got.shape == (a.shape[0],) + tuple(dst)
        for s in range(a.shape[0]):
            exp = zoom(a[s], (dst[0] / a.shape[1], dst[1] / a.shape[2]), order=0)
            assert exp.shape == tuple(dst) and np.array_equal(got[s], exp), s


def _facts(case, direction):
    """per axis: (number of output indices that read nothing, whether the last one is among them, .5 ties)"""
    patch, xy = case
    src, dst = (xy, patch) if direction == "fwd" else (patch, xy)
    out = []
    for k in (0, 1):
        _, ok, ties = R.axis_map(src[k], dst[k])
        out.append((int((~ok).sum()), bool(not ok[-1]), ties))
    return out


def test_cases_are_what_they_are_for():
    c = R.CASES
    zeroed, kept = (1, True), (0, False)
    assert [f[:2] for f in _facts(c[0], "fwd")] == [zeroed, kept] and [f[:2] for f in _facts(c[0], "back")] == [kept, zeroed]
    assert c[1][1][0] > c[1][0][0] and c[1][1][1] > c[1][0][1]                                    # downsampling forward
    assert [f[:2] for f in _facts(c[1], "fwd")] == [zeroed, zeroed]
    assert _facts(c[2], "back") == [(0, False, 63), (1, True, 0)]
    (p0, p1), (x, y) = c[3]
    assert x < p0 and y > p1 and _facts(c[3], "back")[0][2] == 21
    assert [f[:2] for f in _facts(c[4], "back")] == [zeroed, zeroed]
    assert c[5][1] == (2, 3) and c[6][0] == c[6][1]
    for d in ("fwd", "back"):                                                                        # identity: the array itself
        assert np.array_equal(R.ref_zoom(R.image(c[6], d), R.target(c[6], d)), R.image(c[6], d))
    assert R.slices(R.RAGGED) == 3 and all(R.target(R.RAGGED, d)[1] % 4 for d in ("fwd", "back"))
    # a zeroed edge is visible in the float32 inputs (nowhere 0) and in the labels (1..3)
    z = R.ref_zoom(R.image(c[0], "fwd"), c[0][0])
    assert (z[:, -1, :] == 0).all() and (z[:, :-1, :] != 0).all()
    z = R.ref_zoom(R.labels(c[4], "back"), c[4][1])
    assert (z[:, -1, :] == 0).all() and (z[:, :, -1] == 0).all() and (z[:, :-1, :-1] > 0).all()


def test_canary_check_rejects_a_planted_write():
    for dtype in (torch.float32, torch.int64):
        buf, view = R.guarded(100, dtype, "cpu")
        assert view.numel() == 100 and view.data_ptr() == buf.data_ptr() + R.GUARD * buf.element_size()
        view.fill_(7)
        assert R.guards_intact(buf, 100)
        for pos in (R.GUARD - 1, R.GUARD + 100, 0, buf.numel() - 1):
            b2 = buf.clone()
            b2[pos] = 0
            assert not R.guards_intact(b2, 100), pos


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_exports():
    import arco_amd._lib as L
    lib = L.load()
    for name in ("arco_zoom_nearest2d", "arco_argmax_zoom_back2d"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced."""
    import arco_amd._lib as L
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    nan, inf = float("nan"), float("inf")
    # src, S, n0, n1, N0, N1, z0, z1, elem_bytes, out
    ok = [p, 2, 5, 6, 7, 8, 4 / 6, 5 / 7, 4, p]
    rejected = [(0, None), (9, None),                                                       # a null pointer
                (1, 0), (2, 0), (3, 0), (1, -1),                                            # a size < 1
                (4, 1), (5, 1), (4, 0), (5, -3),                                            # an output axis < 2
                (8, 0), (8, 2), (8, 16), (8, 3),                                            # an element size other than 4 or 8
                (6, nan), (7, nan), (6, inf), (7, -inf), (6, -0.5), (7, -1e-300)]           # a non-finite or negative z
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_zoom_nearest2d(*args, None) == -1, (pos, val)
    # X, ld, C, n, P0, P1, N0, N1, z0, z1, out
    ok = [p, 4, 4, 2, 5, 6, 7, 8, 4 / 6, 5 / 7, p]
    rejected = [(0, None), (10, None),                                                      # a null pointer
                (2, 0), (2, 33), (2, -1),                                                   # C < 1 or > 32
                (1, 3), (1, 0),                                                             # ld < C
                (3, 0), (4, 0), (5, 0), (3, -2),                                            # a size < 1
                (6, 1), (7, 1), (6, 0),                                                     # an output axis < 2
                (8, nan), (9, inf), (8, -0.5)]                                              # a non-finite or negative z
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_argmax_zoom_back2d(*args, None) == -1, (pos, val)
    assert (buf == 0).all()


# ---- Python level ------------------------------------------------------------------------------------------------------------------------
def test_zoom_gpu_refuses_before_any_gpu_call():
    from arco_amd.dataloaders import gpu_ingest
    from arco_amd.utils import zoom_gpu
    assert zoom_gpu.ROUTES == ("host", "gpu") and zoom_gpu.zoomed_size is gpu_ingest.zoomed_size
    assert zoom_gpu.zoomed_size(28, 48) == (48, 27 / 47)
    t = torch.ones((2, 5, 6), dtype=torch.float32)
    with pytest.raises(TypeError):
        zoom_gpu.zoom_nearest(t, (7, 8))                                                   # a host tensor
    with pytest.raises(TypeError):
        zoom_gpu.zoom_nearest(t.numpy(), (7, 8))
    with pytest.raises(TypeError):
        zoom_gpu.zoom_nearest(t.double(), (7, 8))                                          # float64 (refused as a host tensor here)
    with pytest.raises(TypeError):
        zoom_gpu.argmax_zoom_back(torch.ones((2, 4, 5, 6)), (7, 8))
    for size in ((1, 8), (7, 1), (0, 0)):                                                  # an output axis < 2
        with pytest.raises(ValueError, match="at least 2"):
            zoom_gpu.zoom_nearest(t, size)
        with pytest.raises(ValueError, match="at least 2"):
            zoom_gpu.argmax_zoom_back(torch.ones((2, 4, 5, 6)), size)


def test_float64_is_refused_by_dtype(monkeypatch):
    """The dtype check itself, with the device check out of the way: a float64 tensor is a TypeError whatever device it is on."""
    from arco_amd.utils import zoom_gpu

    class OnDevice(torch.Tensor):
        is_cuda = True
    for dtype in (torch.float64, torch.float16, torch.int32, torch.uint8, torch.bool):
        t = torch.ones((2, 5, 6), dtype=dtype).as_subclass(OnDevice)
        assert t.is_cuda
        with pytest.raises(TypeError, match="float32 or int64"):
            zoom_gpu.zoom_nearest(t, (7, 8))


def test_route_keywords():
    from arco_amd import eval_surface
    from arco_amd.utils import zoom_gpu
    assert zoom_gpu.check_zoom("host") == "host" and zoom_gpu.check_zoom("gpu") == "gpu"
    img, lab = np.ones((2, 8, 9), dtype=np.float32), np.ones((2, 8, 9), dtype=np.int64)
    for bad in ("x", "cuda", "GPU", None, 1):
        with pytest.raises(ValueError, match="zoom"):
            zoom_gpu.check_zoom(bad)
        with pytest.raises(ValueError, match="zoom"):
            eval_surface.predict_volume(img, None, (16, 16), zoom=bad)
        with pytest.raises(ValueError, match="zoom"):
            eval_surface.test_single_volume(img, lab, None, 4, (16, 16), surface="gpu", zoom=bad)
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_single_volume(img, lab, None, 4, (16, 16), zoom="gpu", surface="host")      # before the net is touched
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_single_volume(img, lab, None, 4, (16, 16), zoom="gpu")                      # the default surface is the host route
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_single_volume(img, lab, None, 4, (16, 16), zoom="gpu", surface="cuda")
    with pytest.raises(ValueError, match="one point"):                                                # a slice axis of 1: before any upload
        eval_surface.predict_volume(np.ones((2, 1, 9), dtype=np.float32), None, (16, 16), zoom="gpu")


def test_round_trip_size_always_comes_back():
    """predict_volume(zoom="gpu") raises when scipy's round trip would not come back to the slice's size; for the sizes in use it does."""
    from arco_amd.utils import zoom_gpu
    for patch in (224, 256):
        for x in range(2, 1025):
            Z = zoom_gpu.zoomed_size(x, patch)[0]
            assert Z == patch and int(round(Z * (x / patch))) == x, (x, patch)
