"""Zoom kernels (arco_amd/csrc/zoom.hip) on the GPU, exact everywhere (array_equal):
  zoom_nearest       equals ref_zoom (tests/zoom_kernel_refs.py, held to scipy by tests/test_zoom_kernels_cpu.py) on every case in both
                     directions, float32 (nowhere 0, so a zeroed edge shows) and int64 labels in 1..3; the entry point itself writes
                     into a buffer with canary margins before and after, which stay untouched
  argmax_zoom_back   (a) equals zoom_nearest(glue.softmax_max(logits)[1], (x, y)) on every case with random logits - the existing
                     kernel is the yardstick -, the logits handed over as a contiguous NCHW tensor, channels-last, and as a channel
                     slice (ld > C);  (b) crafted integer-valued rows with a unique maximum in every class position, C = 1, 2, 4, 32,
                     against numpy;  (c) the tie rows: equal fp32 probabilities take the first class, where an arg-max of the logits
                     would take the other."""
import numpy as np
import pytest
import torch

import zoom_kernel_refs as R

pytestmark = pytest.mark.gpu

DIRECTIONS = ["fwd", "back"]


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_zoom_nearest_equals_reference(case, direction):
    import arco_amd._lib as L
    from arco_amd.utils import zoom_gpu
    dst = R.target(case, direction)
    for a in (R.image(case, direction), R.labels(case, direction)):
        exp = R.ref_zoom(a, dst)
        x = torch.from_numpy(a).cuda()
        got = zoom_gpu.zoom_nearest(x, dst)
        assert got.dtype == x.dtype and got.is_cuda and tuple(got.shape) == exp.shape
        assert np.array_equal(got.cpu().numpy(), exp)
        # the entry point on an exactly-sized output between two canary margins
        S, n0, n1 = a.shape
        buf, out = R.guarded(exp.size, x.dtype, "cuda")
        L.call("arco_zoom_nearest2d", L.ptr(x), S, n0, n1, dst[0], dst[1], (n0 - 1) / (dst[0] - 1), (n1 - 1) / (dst[1] - 1),
               x.element_size(), L.ptr(out))
        torch.cuda.synchronize()
        assert R.guards_intact(buf, exp.size)
        assert np.array_equal(out.cpu().numpy().reshape(exp.shape), exp)


def test_zoom_nearest_takes_a_strided_view_and_refuses_float64():
    from arco_amd.utils import zoom_gpu
    case = R.CASES[0]
    a = R.image(case, "fwd")
    wide = torch.from_numpy(np.concatenate([a, a], axis=2)).cuda()
    assert np.array_equal(zoom_gpu.zoom_nearest(wide[:, :, :a.shape[2]], case[0]).cpu().numpy(), R.ref_zoom(a, case[0]))
    with pytest.raises(TypeError, match="float32 or int64"):
        zoom_gpu.zoom_nearest(torch.from_numpy(a).cuda().double(), case[0])
    with pytest.raises(ValueError, match="at least 2"):
        zoom_gpu.zoom_nearest(torch.from_numpy(a).cuda(), (1, 9))


def _forms(logits):
    """the same [n, C, P0, P1] logits as a contiguous NCHW tensor, channels-last, and a channel slice of a wider channels-last tensor"""
    n, C, P0, P1 = logits.shape
    nchw = logits.contiguous()
    cl = logits.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wide = torch.full((n, P0, P1, C + 4), 99.0, dtype=logits.dtype, device=logits.device)       # the extra channels would win
    wide[..., :C] = logits.permute(0, 2, 3, 1)
    sl = wide.permute(0, 3, 1, 2)[:, :C]
    assert nchw.is_contiguous() and sl.stride(3) == C + 4 and not sl.is_contiguous()
    assert C == 1 or (not cl.is_contiguous() and cl.stride(1) == 1 and sl.stride(1) == 1)      # (a one-channel axis has no stride to speak of)
    return {"nchw": nchw, "channels_last": cl, "ld>C": sl}


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_argmax_zoom_back_equals_softmax_max_then_zoom(case):
    import arco_amd._lib as L
    from arco_amd import glue
    from arco_amd._contrast import rows_view
    from arco_amd.utils import zoom_gpu
    patch, xy = case
    n, C = R.slices(case), 4
    rng = np.random.default_rng(sum(patch) + sum(xy))
    logits = torch.from_numpy(rng.standard_normal((n, C) + patch).astype(np.float32)).cuda()
    amax = glue.softmax_max(logits)[1]
    exp = zoom_gpu.zoom_nearest(amax, xy)
    assert np.array_equal(exp.cpu().numpy(), R.ref_zoom(amax.cpu().numpy(), xy))
    for name, form in _forms(logits).items():
        got = zoom_gpu.argmax_zoom_back(form, xy)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (n,) + xy, name
        assert torch.equal(got, exp), name
    # the entry point on an exactly-sized output between two canary margins
    r, ld = rows_view(logits)
    buf, out = R.guarded(exp.numel(), torch.int64, "cuda")
    L.call("arco_argmax_zoom_back2d", L.ptr(r), ld, C, n, patch[0], patch[1], xy[0], xy[1], (patch[0] - 1) / (xy[0] - 1),
           (patch[1] - 1) / (xy[1] - 1), L.ptr(out))
    torch.cuda.synchronize()
    assert R.guards_intact(buf, exp.numel()) and torch.equal(out.view(exp.shape), exp)


@pytest.mark.parametrize("C", [1, 2, 4, 32])
def test_argmax_zoom_back_crafted_rows(C):
    """Integer-valued logits, the maximum (5, the rest in -3..3) unique and in class position (s + 7 i + j) % C: every class position
    wins somewhere, the probabilities are far apart, and numpy's argmax of the logits is the expected class."""
    from arco_amd.utils import zoom_gpu
    patch, xy = R.CASES[0]
    n = 2
    rng = np.random.default_rng(C)
    logits = rng.integers(-3, 4, size=(n, C) + patch).astype(np.float32)
    s, i, j = np.indices((n,) + patch)
    win = (s + 7 * i + j) % C
    np.put_along_axis(logits, win[:, None], 5.0, axis=1)
    assert np.array_equal(logits.argmax(axis=1), win) and set(np.unique(win)) == set(range(C))
    exp = R.ref_zoom(win.astype(np.int64), xy)
    assert set(np.unique(exp)) == set(range(C)) and (exp[:, :, -1] == 0).all()              # this case zeroes the last label column
    for name, form in _forms(torch.from_numpy(logits).cuda()).items():
        assert np.array_equal(zoom_gpu.argmax_zoom_back(form, xy).cpu().numpy(), exp), name


def test_argmax_zoom_back_tie_rows():
    """argmax(softmax(.)) takes the FIRST class when the fp32 probabilities tie: [0, 0], and [-1e-9, 0], whose exp(-1e-9) is 1.0f.  The
    arg-max of the logits takes class 1 in the second row."""
    from arco_amd import glue
    from arco_amd.utils import zoom_gpu
    P = (8, 8)
    rows = {(0.0, 0.0): 0, (-1e-9, 0.0): 0, (0.0, -1e-9): 0, (0.0, 1.0): 1, (1.0, 0.0): 0}
    for (a, b), cls in rows.items():
        logits = torch.empty((1, 2) + P, dtype=torch.float32)
        logits[:, 0], logits[:, 1] = a, b
        if (a, b) == (-1e-9, 0.0):
            assert float(logits[0, 0, 0, 0]) < 0 and int(logits.argmax(dim=1)[0, 0, 0]) == 1      # the logits' own arg-max differs
        d = logits.cuda()
        assert (glue.softmax_max(d)[1] == cls).all(), (a, b)
        for size in (P, (5, 11)):
            assert all(R.axis_map(8, m)[1].all() for m in size)                                 # no zeroed edge at these sizes
            got = zoom_gpu.argmax_zoom_back(d, size)
            assert tuple(got.shape) == (1,) + size and (got == cls).all(), (a, b, size)
