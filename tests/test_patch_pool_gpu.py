"""arco_patch_pool_fwd / arco_patch_pool_bwd (csrc/patch_pool.hip) against their fp32 statements of tests/patch_pool_refs.py, bit for
bit, on the case table shared with tests/test_patch_pool_cpu.py; run-to-run identity; every element of gx written; stage1.PatchPoolFn;
the refusals (-m gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import patch_pool_refs as R        # noqa: E402

pytestmark = pytest.mark.gpu


def _geom(n, patch, pool, B, C):
    return (len(n), B, C) + tuple(n) + (1,) * (3 - len(n)) + (patch, pool)


def _fwd(x, n, patch, pool, y):
    from arco_amd import _lib as L
    L.call("arco_patch_pool_fwd", L.ptr(x), *_geom(n, patch, pool, x.shape[0], x.shape[1]), L.ptr(y))
    return y


def _bwd(gy, n, patch, pool, gx):
    from arco_amd import _lib as L
    L.call("arco_patch_pool_bwd", L.ptr(gy), *_geom(n, patch, pool, gy.shape[1], gy.shape[2]), L.ptr(gx))
    return gx


def _same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32))


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_forward_bit_for_bit(case):
    n, patch, pool, B, C = case
    x, gy = R.case_input(case)
    want = R.patch_pool_fwd_f32(x, patch, pool)
    xd = torch.from_numpy(x).cuda()
    y1 = _fwd(xd, n, patch, pool, torch.full(want.shape, float("nan"), device="cuda"))
    y2 = _fwd(xd, n, patch, pool, torch.full(want.shape, float("nan"), device="cuda"))
    assert not torch.isnan(y1).any()
    assert _same_bits(y1, want)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_backward_bit_for_bit_and_writes_every_element(case):
    n, patch, pool, B, C = case
    x, gy = R.case_input(case)
    want, _, terms = R.patch_pool_bwd_f32(gy, n, patch, pool)
    gyd = torch.from_numpy(gy).cuda()
    g1 = _bwd(gyd, n, patch, pool, torch.full(x.shape, float("nan"), device="cuda"))
    g2 = _bwd(gyd, n, patch, pool, torch.full(x.shape, float("nan"), device="cuda"))
    assert not torch.isnan(g1).any()                      # the output was NaN before the launch: every element is written
    assert _same_bits(g1, want)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert (g1.cpu().numpy()[:, :, terms == 0] == 0).all()


def test_patch_pool_fn():
    from arco_amd.stage1 import PatchPoolFn
    n, patch, pool, B, C = R.CASES[0]
    x, gy = R.case_input(R.CASES[0])
    xd, gyd = torch.from_numpy(x).cuda(), torch.from_numpy(gy).cuda()
    want = _fwd(xd, n, patch, pool, torch.empty(gy.shape, device="cuda"))
    # a permuted view of the same values
    view = xd.permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2)
    assert not view.is_contiguous()
    assert torch.equal(PatchPoolFn.apply(view, patch, pool), want)
    with torch.no_grad():
        y = PatchPoolFn.apply(xd.clone().requires_grad_(True), patch, pool)
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, want)
    leaf = view.detach().requires_grad_(True)
    y = PatchPoolFn.apply(leaf, patch, pool)
    assert y.grad_fn is not None and tuple(y.grad_fn.saved_tensors) == ()       # the geometry alone
    y.backward(gyd)
    assert torch.equal(leaf.grad, _bwd(gyd, n, patch, pool, torch.empty(x.shape, device="cuda")))
    # 2-D, through a non-contiguous incoming gradient
    n, patch, pool, B, C = R.CASES[-1]
    x, gy = R.case_input(R.CASES[-1])
    xd, gyd = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(gy).cuda()
    y = PatchPoolFn.apply(xd, patch, pool)
    assert y.shape == gy.shape
    (y.transpose(-1, -2) * gyd.transpose(-1, -2)).sum().backward()
    assert torch.equal(xd.grad, _bwd(gyd, n, patch, pool, torch.empty(x.shape, device="cuda")))
    with pytest.raises(ValueError):
        PatchPoolFn.apply(xd.detach().double(), patch, pool)


@pytest.mark.parametrize("entry", ["arco_patch_pool_fwd", "arco_patch_pool_bwd"])
def test_refusals(entry):
    """nd outside {2, 3}, patch < 2, pool < 1, an axis shorter than the patch, null pointers: an error that names the entry point, before
    any launch - the output keeps its fill."""
    from arco_amd import _lib as L
    B, C, n, patch, pool = 1, 2, (8, 8, 8), 4, 2
    big = torch.full((27 * B * C * 8 + B * C * 512,), 7.0, device="cuda")      # room for either tensor of the good call
    src, dst = torch.arange(big.numel(), dtype=torch.float32, device="cuda"), big.clone()
    good = dict(nd=3, B=B, C=C, n0=8, n1=8, n2=8, patch=patch, pool=pool)
    bad = [dict(nd=1), dict(nd=4), dict(patch=1), dict(patch=0), dict(pool=0), dict(pool=-1), dict(n0=3), dict(n1=3), dict(n2=3), dict(B=0), dict(C=0),
           dict(nd=2, n1=3)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match=entry):
            L.call(entry, L.ptr(src), a["nd"], a["B"], a["C"], a["n0"], a["n1"], a["n2"], a["patch"], a["pool"], L.ptr(dst))
    for s, d in ((None, L.ptr(dst)), (L.ptr(src), None)):
        with pytest.raises(RuntimeError, match=entry):
            L.call(entry, s, *good.values(), d)
    torch.cuda.synchronize()
    assert torch.equal(dst, big)
    L.call(entry, L.ptr(src), *good.values(), L.ptr(dst))                      # the good call goes through and writes
    torch.cuda.synchronize()
    assert not torch.equal(dst, big)
