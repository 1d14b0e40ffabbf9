"""Cubic-spline zoom kernels (arco_amd/csrc/zoom.hip) on the GPU, exact everywhere (array_equal) against the float64 restatement of
tests/zoom_cubic_kernel_refs.py (held to scipy by tests/test_zoom_cubic_kernels_cpu.py), on every case and every variant of its data:
  spline_prefilter   the float64 coefficients, and each of the two passes alone through the entry point (axis 0: src -> out; axis 1:
                     in place), on exactly-sized outputs between canary margins, which stay untouched
  zoom_cubic         the float32 result; the interpolation entry point alone on the restatement's coefficients, between canary margins
  wrappers           a strided view is accepted; float64 and int64 inputs, a one-point axis and a one-point target are refused."""
import numpy as np
import pytest
import torch

import zoom_cubic_kernel_refs as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    """(coefficients after axis 0, coefficients, float32 zoom) of the restatement per (case, variant), computed once."""
    out = {}
    for case in C.CASES:
        for variant in C.VARIANTS:
            a = C.image(case, variant)
            c0 = C.ref_prefilter(a, axes=(0,))
            coef = C.ref_prefilter(c0, axes=(1,))
            out[case, variant] = (c0, coef, C.ref_interpolate(coef, case[1]))
    return out


def _guarded64(n):
    """C.guarded for float64, which zoom_kernel_refs has no sentinel for: (buffer, view, intact())."""
    sent = -12345.5
    buf = torch.full((n + 2 * 64,), sent, dtype=torch.float64, device="cuda")
    return buf, buf[64:64 + n], lambda: bool((buf[:64] == sent).all().item()) and bool((buf[64 + n:] == sent).all().item())


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_spline_prefilter_equals_restatement(case, expected):
    import arco_amd._lib as L
    from arco_amd.utils import zoom_gpu
    S, n0, n1 = case[0]
    for variant in C.VARIANTS:
        c0, coef, _ = expected[case, variant]
        x = torch.from_numpy(C.image(case, variant)).cuda()
        got = zoom_gpu.spline_prefilter(x)
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == coef.shape
        assert np.array_equal(got.cpu().numpy(), coef), variant
        # the entry point, one pass at a time, on an exactly-sized output between two canary margins
        buf, out, intact = _guarded64(coef.size)
        consts = zoom_gpu.spline_constants(n0, n1)
        L.call("arco_spline_prefilter2d", L.ptr(x), S, n0, n1, *consts, 1, L.ptr(out))
        torch.cuda.synchronize()
        assert intact() and np.array_equal(out.cpu().numpy().reshape(c0.shape), c0), variant
        L.call("arco_spline_prefilter2d", L.ptr(x), S, n0, n1, *consts, 2, L.ptr(out))
        torch.cuda.synchronize()
        assert intact() and np.array_equal(out.cpu().numpy().reshape(coef.shape), coef), variant


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_zoom_cubic_equals_restatement(case, expected):
    import arco_amd._lib as L
    from arco_amd.utils import zoom_gpu
    (S, n0, n1), dst = case
    for variant in C.VARIANTS:
        _, coef, exp = expected[case, variant]
        x = torch.from_numpy(C.image(case, variant)).cuda()
        got = zoom_gpu.zoom_cubic(x, dst)
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == exp.shape
        assert np.array_equal(got.cpu().numpy(), exp), variant
        # the interpolation entry point on the restatement's coefficients, output between two canary margins
        buf, out = C.guarded(exp.size, torch.float32, "cuda")
        L.call("arco_zoom_cubic2d", L.ptr(torch.from_numpy(coef).cuda()), S, n0, n1, dst[0], dst[1], (n0 - 1) / (dst[0] - 1),
               (n1 - 1) / (dst[1] - 1), L.ptr(out))
        torch.cuda.synchronize()
        assert C.guards_intact(buf, exp.size)
        assert np.array_equal(out.cpu().numpy().reshape(exp.shape), exp), variant
    rows, cols = C.zeroed_edges(case)
    if rows:
        assert (exp[:, -1, :] == 0).all() and (exp[:, :-1, :-1] != 0).all()
    if cols:
        assert (exp[:, :, -1] == 0).all()


def test_cubic_wrappers_take_a_strided_view_and_refuse_other_inputs(expected):
    from arco_amd.utils import zoom_gpu
    case = C.CASES[7]
    a = C.image(case, "unit")
    _, coef, exp = expected[case, "unit"]
    wide = torch.from_numpy(np.concatenate([a, a], axis=2)).cuda()
    view = wide[:, :, :a.shape[2]]
    assert not view.is_contiguous()
    assert np.array_equal(zoom_gpu.zoom_cubic(view, case[1]).cpu().numpy(), exp)
    assert np.array_equal(zoom_gpu.spline_prefilter(view).cpu().numpy(), coef)
    x = torch.from_numpy(a).cuda()
    for bad in (x.double(), x.long()):
        with pytest.raises(TypeError, match="takes float32"):
            zoom_gpu.zoom_cubic(bad, case[1])
        with pytest.raises(TypeError, match="takes float32"):
            zoom_gpu.spline_prefilter(bad)
    for one in (x[:, :1, :], x[:, :, :1]):                                   # an input axis of one point
        with pytest.raises(ValueError, match="at least 2"):
            zoom_gpu.zoom_cubic(one, case[1])
        with pytest.raises(ValueError, match="at least 2"):
            zoom_gpu.spline_prefilter(one)
    for size in ((1, 9), (9, 1)):                                            # a target axis of one point
        with pytest.raises(ValueError, match="at least 2"):
            zoom_gpu.zoom_cubic(x, size)
