"""Cubic-spline zoom kernels (arco_amd/csrc/zoom.hip, arco_amd/utils/zoom_gpu.py), the part that needs no GPU:
  reference     ref_zoom_cubic of tests/zoom_cubic_kernel_refs.py against scipy.ndimage.zoom(order=3) on every case and variant: the
                float32 results equal, except that at most 1 output in 10 000 of a case may differ, and then by one float32 ulp (the two
                float64 paths agree to a few 1e-16 relative, so a float32 rounding boundary is crossed about once in 1e8 outputs);
                ref_prefilter against scipy.ndimage.spline_filter within COEF_BOUND of max|c|
  cases         what each case is there for actually holds
  host doubles  the pole, the gain and the powers of the pole that zoom_gpu hands to the kernels are the restatement's
  C ABI         the two entry points are exported; ARCO_ERR_ARG on the host for every rejection of include/arco_hip.h
  rejections    check_order, order=5 at every entry point, a float64 volume on the device route, bad dtypes / sizes of zoom_cubic and
                spline_prefilter - all raised before any GPU call (there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import spline_filter, zoom

import zoom_cubic_kernel_refs as C


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_restatement_is_scipy(case):
    (S, n0, n1), dst = case
    for variant in C.VARIANTS:
        a = C.image(case, variant)
        assert a.dtype == np.float32 and a.shape == (S, n0, n1) and (a != 0).all()
        coef = C.ref_prefilter(a)
        got = C.ref_interpolate(coef, dst)
        assert coef.dtype == np.float64 and got.dtype == np.float32 and got.shape == (S,) + dst
        exp = np.stack([zoom(a[s], (dst[0] / n0, dst[1] / n1), order=3) for s in range(S)])
        assert exp.shape == got.shape and exp.dtype == np.float32
        differ = got != exp
        n_diff, dev = int(differ.sum()), 0.0
        sc = np.stack([spline_filter(a[s], order=3, output=np.float64, mode='constant') for s in range(S)])
        dev = float(np.abs(sc - coef).max() / np.abs(coef).max())
        print("%s %s: %d of %d outputs differ, coefficients deviate by %.3g of max|c|" % (C.IDS[C.CASES.index(case)], variant, n_diff,
                                                                                        got.size, dev))
        assert n_diff * 10000 <= got.size, (variant, n_diff, got.size)
        assert n_diff == 0 or int(_ulps(got[differ], exp[differ]).max()) == 1
        assert dev <= C.COEF_BOUND, (variant, dev)


def test_cases_are_what_they_are_for():
    c = C.CASES
    shapes = [s for s, _ in c]
    assert any(s[1] == 2 and s[2] == 3 for s in shapes) and any(s[1] == 3 and s[2] == 2 for s in shapes)
    for case in c[:2]:                                                   # an axis of 2 and one of 3 points: every tap set holds a mirrored tap
        for n_in, n_out in zip(case[0][1:], case[1]):
            ok, idx, _ = C.axis_taps(n_in, n_out)
            fl = np.floor(np.arange(n_out) * ((n_in - 1) / (n_out - 1))).astype(np.int64)
            raw = fl[:, None] - 1 + np.arange(4)[None, :]
            assert ok.all() and ((raw < 0) | (raw > n_in - 1)).any(axis=1).all() and idx.min() >= 0 and idx.max() <= n_in - 1
    pairs = {(n_in, n_out): C.axis_taps(n_in, n_out)[0] for n_in, n_out in ((8, 26), (28, 14), (15, 51))}
    for ok in pairs.values():                                            # exactly the last index is outside
        assert ok[:-1].all() and not ok[-1]
    assert C.zeroed_edges(c[2]) == (True, True) and C.zeroed_edges(c[3]) == (True, True) and C.zeroed_edges(c[4]) == (True, True)
    assert c[3][0][1] > c[3][1][0] and c[2][0][1] < c[2][1][0]           # down and up
    z = C.ref_zoom_cubic(C.image(c[3], "unit"), c[3][1])
    assert (z[:, -1, :] == 0).all() and (z[:, :, -1] == 0).all() and (z[:, :-1, :-1] != 0).all()      # a zeroed edge is visible
    for case, ax in ((c[5], 0), (c[6], 1)):                              # one axis kept: its step is exactly 1
        assert case[0][1 + ax] == case[1][ax] and case[0][2 - ax] != case[1][1 - ax]
        ok, idx, w = C.axis_taps(case[0][1 + ax], case[1][ax])
        assert ok.all() and (idx[:, 1] == np.arange(case[1][ax])).all() and (w == w[0]).all() and w[0, 1] == 4.0 / 6.0
        assert 0 < w[0, 3] < 1e-16                                       # ... and still not the identity in bits: w3 is not 0
    for case in (c[7], c[8]):
        assert case[0][0] == 3 and case[0][2] % 4 and case[1][1] % 4 and {case[0][2], case[1][1]} == {37, 53}
    (S, n0, n1), _ = c[9]
    assert n1 % C.ROW_TILE and n1 > 2 * C.ROW_TILE and S * n0 > 128 and (S * n0) % 64          # three tiles; three waves, the last short
    assert c[10][0][2] == 520 and c[11][0][1] == 520 and 0 < abs(C.pole_power(520)) < 1e-290
    assert max(c[12][0][1:]) <= 12 and abs(C.pole_power(12)) > 1e-7
    assert c[13][0][2] == 600 and c[14][0][1] == 600 and C.pole_power(600) == 0.0
    zi, seen_denormal = C.Z, False
    for _ in range(598):
        zi *= C.Z
        seen_denormal |= 0 < abs(zi) < 2.3e-308
    assert seen_denormal and zi == 0.0
    for case in c:                                                       # a constant slice: the variant is one
        a = C.image(case, "const")
        assert (a == a[:, :1, :1]).all()
        a, k = C.image(case, "unit"), C.image(case, "kilo")
        assert (np.abs(a) >= 0.5).all() and (np.abs(a) <= 2).all() and (np.abs(k) >= 500).all()


def test_single_pass_restatements_compose():
    case = C.CASES[9]
    a = C.image(case, "unit")
    assert np.array_equal(C.ref_prefilter(C.ref_prefilter(a, axes=(0,)), axes=(1,)), C.ref_prefilter(a))


def test_host_doubles_are_the_restatements():
    from arco_amd.utils import zoom_gpu
    assert zoom_gpu.SPLINE_POLE == C.Z and zoom_gpu.SPLINE_GAIN == C.GAIN
    for n0, n1 in ((2, 3), (12, 9), (75, 70), (520, 6), (256, 216), (600, 3), (512, 512)):
        assert zoom_gpu.spline_constants(n0, n1) == (C.Z, C.GAIN, C.pole_power(n0), C.pole_power(n1))
    assert zoom_gpu._step(28, 14) == 27 / 13


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_exports():
    import arco_amd._lib as L
    lib = L.load()
    for name in ("arco_spline_prefilter2d", "arco_zoom_cubic2d"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced."""
    import arco_amd._lib as L
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    nan, inf = float("nan"), float("inf")
    # src, S, n0, n1, z, gain, zn0, zn1, axes, out
    ok = [p, 2, 5, 6, C.Z, C.GAIN, C.pole_power(5), C.pole_power(6), 3, p]
    rejected = [(0, None), (9, None),                                                       # a null pointer
                (1, 0), (1, -1),                                                            # S < 1
                (2, 1), (3, 1), (2, 0), (3, -4),                                            # an input axis < 2
                (4, nan), (5, inf), (6, nan), (7, -inf),                                    # a constant that is not finite
                (8, 0), (8, 4), (8, -1)]                                                    # axes outside 1..3
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_spline_prefilter2d(*args, None) == -1, (pos, val)
    # coef, S, n0, n1, N0, N1, z0, z1, out
    ok = [p, 2, 5, 6, 7, 8, 4 / 6, 5 / 7, p]
    rejected = [(0, None), (8, None),                                                       # a null pointer
                (1, 0), (1, -1),                                                            # S < 1
                (2, 1), (3, 1), (2, 0), (3, -4), (2, (1 << 30) + 1),                        # an input axis < 2 (or past the mirror period)
                (4, 1), (5, 1), (4, 0), (5, -3),                                            # an output axis < 2
                (6, nan), (7, nan), (6, inf), (7, -inf), (6, -0.5), (7, -1e-300)]           # a step that is negative or not finite
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_zoom_cubic2d(*args, None) == -1, (pos, val)
    assert (buf == 0).all()


# ---- Python level ------------------------------------------------------------------------------------------------------------------------
def test_order_keyword():
    from arco_amd import eval_surface
    from arco_amd.utils import zoom_gpu
    assert zoom_gpu.ORDERS == (0, 3) and zoom_gpu.check_order(0) == 0 and zoom_gpu.check_order(3) == 3
    img, lab = np.ones((2, 8, 9), dtype=np.float32), np.ones((2, 8, 9), dtype=np.int64)
    for bad in (5, 1, 2, -3, None, "3", True, 3.5):
        with pytest.raises(ValueError, match="order"):
            zoom_gpu.check_order(bad)
        for zm in ("host", "gpu"):
            with pytest.raises(ValueError, match="order"):                                  # before the net (None) is touched
                eval_surface.predict_volume(img, None, (16, 16), zoom=zm, order=bad)
            with pytest.raises(ValueError, match="order"):
                eval_surface.test_single_volume(img, lab, None, 4, (16, 16), surface="gpu", zoom=zm, order=bad)
    with pytest.raises(ValueError, match="order"):
        eval_surface.test_single_volume(img, lab, None, 4, (16, 16), order=5)
    # the device route takes a float32 volume only at order 3
    for dtype in (np.float64, np.int16):
        with pytest.raises(ValueError, match="float32"):
            eval_surface.predict_volume(img.astype(dtype), None, (16, 16), zoom="gpu", order=3)
        with pytest.raises(ValueError, match="float32"):
            eval_surface.test_single_volume(img.astype(dtype), lab, None, 4, (16, 16), surface="gpu", zoom="gpu", order=3)
    with pytest.raises(ValueError, match="surface"):                                        # zoom="gpu" still needs surface="gpu"
        eval_surface.test_single_volume(img, lab, None, 4, (16, 16), zoom="gpu", order=3)
    with pytest.raises(ValueError, match="one point"):
        eval_surface.predict_volume(np.ones((2, 1, 9), dtype=np.float32), None, (16, 16), zoom="gpu", order=3)


def test_cubic_wrappers_refuse_before_any_gpu_call():
    from arco_amd.utils import zoom_gpu

    class OnDevice(torch.Tensor):
        is_cuda = True
    t = torch.ones((2, 5, 6), dtype=torch.float32)
    for fn in (lambda x: zoom_gpu.zoom_cubic(x, (7, 8)), zoom_gpu.spline_prefilter):
        with pytest.raises(TypeError, match="on the GPU"):
            fn(t)                                                                           # a host tensor
        with pytest.raises(TypeError, match="on the GPU"):
            fn(t.numpy())
        for dtype in (torch.float64, torch.int64, torch.float16, torch.int32, torch.uint8):
            with pytest.raises(TypeError, match="takes float32"):
                fn(torch.ones((2, 5, 6), dtype=dtype).as_subclass(OnDevice))
        for shape in ((2, 1, 6), (2, 5, 1), (1, 1, 1)):                                     # an input axis of one point
            with pytest.raises(ValueError, match="at least 2"):
                fn(torch.ones(shape).as_subclass(OnDevice))
        with pytest.raises(ValueError, match="non-empty"):
            fn(torch.ones((5, 6)).as_subclass(OnDevice))
    for size in ((1, 8), (7, 1), (0, 0)):                                                   # an output axis of one point
        with pytest.raises(ValueError, match="at least 2"):
            zoom_gpu.zoom_cubic(t.as_subclass(OnDevice), size)
