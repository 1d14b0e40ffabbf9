"""The two kernels of the f16 inference route on the GPU, bit for bit:

  arco_bn_act_pool_fwd_h     both outputs torch.equal to arco_bn_act_fwd_h followed by arco_maxpool2_fwd_h on the same input, the
                             full-resolution one also bit for bit tests/eval_half_kernel_refs.ref_bn_act_pool (operation for operation,
                             held to exact rational arithmetic by tests/test_eval_half_kernels_cpu.py); a wider output buffer (the
                             decoder's concat room) keeps its other channels
  arco_argmax_zoom_back2d_h  torch.equal to arco_argmax_zoom_back2d on the fp32 cast of the same f16 rows and to
                             ref_argmax_zoom_back: dense rows, wide rows that allow 8-byte loads and wide rows that do not, exact ties,
                             +0.0 against -0.0; 33 classes are an error return"""
import numpy as np
import pytest
import torch

import eval_half_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -777.0          # what the concat room holds before the launch


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("room", R.CAT_ROOMS, ids=["dense", "cat_room16"])
@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=R.POOL_IDS)
def test_bn_act_pool_fwd_h_equals_apply_then_pool_and_the_reference(shape, slope, room):
    from arco_amd import _lib as L
    c, H, W = shape
    z_np, mean, istd, gamma, beta = R.pool_case(c, H, W)
    z = _dev(z_np)                                                   # [NB, H, W, c] rows
    par = [_dev(v) for v in (mean, istd, gamma, beta)]
    ld = c + room
    m = R.NB * H * W
    fused = torch.full((R.NB, H, W, ld), SENT, dtype=torch.float16, device=DEV)
    pooled = torch.full((R.NB, H // 2, W // 2, c), SENT, dtype=torch.float16, device=DEV)
    L.call("arco_bn_act_pool_fwd_h", L.ptr(z), c, R.NB, H, W, c, *(L.ptr(p) for p in par), float(slope), L.ptr(fused), ld,
           L.ptr(pooled), c, 1)
    two = torch.full((R.NB, H, W, ld), SENT, dtype=torch.float16, device=DEV)
    two_pooled = torch.full((R.NB, H // 2, W // 2, c), SENT, dtype=torch.float16, device=DEV)
    L.call("arco_bn_act_fwd_h", L.ptr(z), c, m, c, *(L.ptr(p) for p in par), float(slope), 0, 0.0, 0, H * W, L.ptr(two), ld, None, 1)
    L.call("arco_maxpool2_fwd_h", L.ptr(two), ld, R.NB, H, W, c, L.ptr(two_pooled), c)
    torch.cuda.synchronize()
    assert torch.equal(fused[..., :c], two[..., :c])
    assert torch.equal(pooled, two_pooled)
    assert torch.equal(fused.view(torch.int16), two.view(torch.int16))              # the bits, signed zeros included
    if room:
        assert bool((fused[..., c:] == SENT).all())                                 # the concat room is untouched
    a_ref, p_ref = R.ref_bn_act_pool(z_np, mean, istd, gamma, beta, slope)
    got = fused[..., :c].contiguous().cpu().numpy()
    assert np.array_equal(got.view(np.uint16), a_ref.view(np.uint16))
    assert np.array_equal(pooled.cpu().numpy(), p_ref)


def test_bn_act_pool_fwd_h_refuses_what_it_cannot_run():
    from arco_amd import _lib as L
    z = torch.zeros((2, 4, 4, 16), dtype=torch.float16, device=DEV)
    a, p = torch.zeros_like(z), torch.zeros((2, 2, 2, 16), dtype=torch.float16, device=DEV)
    par = [torch.ones(16, device=DEV) for _ in range(4)]
    lib = L.load()

    def rc(H, W, C, lda):
        return lib.arco_bn_act_pool_fwd_h(L.ptr(z), 16, 2, H, W, C, *(L.ptr(q) for q in par), 0.01, L.ptr(a), lda, L.ptr(p), 16, 1, L.stream())
    assert rc(4, 4, 16, 16) == 0
    assert rc(3, 4, 16, 16) == -1 and rc(4, 3, 16, 16) == -1            # odd sides
    assert rc(4, 4, 6, 16) == -1 and rc(4, 4, 16, 12) == -1             # C not a multiple of 4; a row shorter than C
    torch.cuda.synchronize()


def _lds(C):
    """dense; wide and odd (no 8-byte loads); wide with rows of whole 8-byte pieces."""
    return [C, C + 5, (C + 3) // 4 * 4 + 8]


@pytest.mark.parametrize("sizes", R.ARGMAX_SIZES, ids=R.ARGMAX_IDS)
@pytest.mark.parametrize("C", R.ARGMAX_CLASSES)
def test_argmax_zoom_back2d_h_equals_the_fp32_kernel_and_the_reference(C, sizes):
    from arco_amd import _lib as L
    patch, out_size = sizes
    (P0, P1), (N0, N1) = patch, out_size
    z0, z1 = (P0 - 1) / (N0 - 1), (P1 - 1) / (N1 - 1)
    for ld in _lds(C):
        rows_np = R.argmax_case(C, patch, ld=ld)
        rows = _dev(rows_np)
        rows32 = rows.float()
        got = torch.full((R.ARGMAX_N, N0, N1), -1, dtype=torch.int64, device=DEV)
        want = torch.full_like(got, -2)
        L.call("arco_argmax_zoom_back2d_h", L.ptr(rows), ld, C, R.ARGMAX_N, P0, P1, N0, N1, z0, z1, L.ptr(got))
        L.call("arco_argmax_zoom_back2d", L.ptr(rows32), ld, C, R.ARGMAX_N, P0, P1, N0, N1, z0, z1, L.ptr(want))
        torch.cuda.synchronize()
        assert torch.equal(got, want), ld
        assert np.array_equal(got.cpu().numpy(), R.ref_argmax_zoom_back(rows_np[..., :C], out_size)), ld


def test_argmax_zoom_back_dispatches_on_the_dtype_of_the_logits():
    """zoom_gpu.argmax_zoom_back on f16 channels-last logits (what `ops.eval_half(logits="stored")` hands out) and on their fp32 cast."""
    from arco_amd.utils import zoom_gpu
    rows_np = R.argmax_case(4, (8, 8))
    logits16 = _dev(rows_np).permute(0, 3, 1, 2)                     # [n, C, P0, P1] over channels-last memory
    a = zoom_gpu.argmax_zoom_back(logits16, (5, 7))
    b = zoom_gpu.argmax_zoom_back(logits16.float(), (5, 7))
    assert a.dtype == torch.int64 and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), R.ref_argmax_zoom_back(rows_np, (5, 7)))


def test_argmax_zoom_back2d_h_33_classes_is_an_error_return():
    from arco_amd import _lib as L
    rows = torch.zeros((2, 8, 8, 36), dtype=torch.float16, device=DEV)
    out = torch.full((2, 8, 8), -1, dtype=torch.int64, device=DEV)
    rc = L.load().arco_argmax_zoom_back2d_h(L.ptr(rows), 36, 33, 2, 8, 8, 8, 8, 1.0, 1.0, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == -1).all())                      # ARCO_ERR_ARG, nothing launched
    with pytest.raises(RuntimeError, match="arco_argmax_zoom_back2d_h failed"):
        L.call("arco_argmax_zoom_back2d_h", L.ptr(rows), 36, 33, 2, 8, 8, 8, 8, 1.0, 1.0, L.ptr(out))
