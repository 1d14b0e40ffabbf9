"""The numpy restatement of the fused patch-head kernels (tests/patch_head_refs.py) against float64 torch autograd of
stage1.patch_heads(route="torch") on CPU modules: output, input gradient and every parameter gradient; the --patch_heads flag, the
ISD / ISD_3d constructor keyword and the fused route's refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import patch_head_refs as R        # noqa: E402
import patch_pool_refs as PR       # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32


def _modules(nd, widths, layers):
    """A head (pooling + the first two layers) and a predictor (the rest) in float64 that hold the case's weights: the shape
    stage1.patch_heads takes.  A chain of one layer has a one-layer head and no predictor."""
    conv = torch.nn.Conv2d if nd == 2 else torch.nn.Conv3d
    mods = []
    for k, (W, b) in enumerate(layers):
        m = conv(widths[k], widths[k + 1], kernel_size=1, bias=b is not None).double()
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(W.astype(np.float64)).reshape(m.weight.shape))
            if b is not None:
                m.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        mods.append(m)
    return mods


class _Head(torch.nn.Module):
    def __init__(self, nd, pool, mods):
        super().__init__()
        self.proj = torch.nn.Sequential((torch.nn.AdaptiveAvgPool2d if nd == 2 else torch.nn.AdaptiveAvgPool3d)(pool), *mods)


def _torch64(x, gy, patch, pool, mods, absolute=False):
    """(output stacked, x gradient, [(weight gradient, bias gradient or None)]) of sum(gy * patch_heads(route="torch")) in float64;
    absolute: with |x|, |gy|, |weights| and |biases| - every sum then is the sum of its terms' magnitudes."""
    from arco_amd.stage1 import patch_heads
    nd = x.ndim - 2
    if absolute:
        import copy
        mods = copy.deepcopy(mods)
        with torch.no_grad():
            for m in mods:
                for p in m.parameters():
                    p.abs_()
        x, gy = np.abs(x), np.abs(gy)
    for m in mods:
        m.zero_grad(set_to_none=True)
    head = _Head(nd, pool, mods[:2])
    predictor = torch.nn.Sequential(*mods[2:]) if len(mods) > 2 else None
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    out = torch.cat(patch_heads(xt, patch, head, predictor, "torch"))
    (out * torch.from_numpy(gy.astype(np.float64))).sum().backward()
    grads = [(m.weight.grad.numpy().reshape(m.weight.shape[:2]), None if m.bias is None else m.bias.grad.numpy()) for m in mods]
    return out.detach().numpy(), xt.grad.numpy(), grads


@pytest.mark.parametrize("case", R.CASES[:-1], ids=R.CASE_IDS[:-1])
def test_restatement_against_float64_autograd(case):
    """Every fp32 result e of the restatement against its float64 value: |error| <= gamma_R * MAG, gamma_R = R u / (1 - R u), u = 2^-24,
    where MAG is the same sum with every term replaced by its magnitude (the float64 route on |x|, |gy|, |W|, |b|) and R counts the
    roundings a term can meet on its way:
      m + 1                    the pooling: a window of m elements summed from 0.f and one division
      sum of (c_{k-1} + 1)     the forward chain: per layer one product and at most c_{k-1} additions (the bias start included)
      sum of c_k               the backward chain: per layer one product and c_k - 1 additions (the first one, to 0.f, is exact)
      t + 1                    the pooling's adjoint: t (patch, cell) tuples cover a voxel - t divisions and t - 1 additions, and one more
      1                        a parameter gradient's single rounding of its float64 sum to fp32 (the float64 sum's own error is 2^-29 u)
    No tensor meets all of them, so one R for all is a bound for each."""
    n, patch, pool, B, widths, nobias = case
    nd = len(n)
    x, layers, gy = R.case_input(case)
    mods = _modules(nd, widths, layers)
    out64, gx64, grads64 = _torch64(x, gy, patch, pool, mods)
    mag_out, mag_gx, mag_grads = _torch64(x, gy, patch, pool, mods, absolute=True)

    pooled, y = R.head_fwd_f32(x, patch, pool, layers)
    d0, grads = R.head_bwd(pooled, gy, layers)
    gx, _, terms = PR.patch_pool_bwd_f32(d0, n, patch, pool)
    assert y.dtype == d0.dtype == gx.dtype == np.float32 and y.shape == out64.shape and gx.shape == gx64.shape

    m = max(hi - lo for lo, hi in PR.windows(patch, pool)) ** nd
    rounds = (m + 1) + sum(c + 1 for c in widths[:-1]) + sum(widths[1:]) + (int(terms.max()) + 1) + 1
    gamma = rounds * U / (1 - rounds * U)
    print(f"{rounds} roundings, rtol {gamma:.2e}")

    def check(name, got, ref, mag):
        err = np.abs(np.asarray(got, np.float64) - ref)
        print(f"{name}: largest error / bound {float((err / np.maximum(gamma * mag, 1e-300)).max()):.3f}")
        assert (err <= gamma * mag).all(), name

    check("output", y, out64, mag_out)
    check("input gradient", gx, gx64, mag_gx)
    for k, ((gw64, gb64), (mw, mb)) in enumerate(zip(grads64, mag_grads)):
        check(f"layer {k} weight gradient", grads[k]["w"].astype(np.float32), gw64, mw)
        if gb64 is not None:
            check(f"layer {k} bias gradient", grads[k]["b"].astype(np.float32), gb64, mb)


def test_patch_heads_flag_fused():
    from arco_amd import pretrain_2D as P2, pretrain_3D as P3
    for mod in (P2, P3):
        assert mod.build_parser().parse_args([]).patch_heads == "torch"
        assert mod.build_parser().parse_args(["--patch_heads", "fused"]).patch_heads == "fused"


def test_patch_heads_constructor_keyword_fused():
    from arco_amd.model_2D import ISD
    from arco_amd.model_3D import ISD_3d
    for cls in (ISD, ISD_3d):
        assert cls(K=4, num_classes=2, patch_heads="fused").patch_heads == "fused"


def test_fused_route_refusals():
    """A head the fused kernels do not take is a ValueError that names the limit, before anything touches a device."""
    from arco_amd.stage1 import patch_heads
    x = torch.zeros(1, 4, 16, 16)
    pool = torch.nn.AdaptiveAvgPool2d(2)

    def head(*mods):
        h = torch.nn.Module()
        h.proj = torch.nn.Sequential(pool, *mods)
        return h
    c = torch.nn.Conv2d
    with pytest.raises(ValueError, match="kernel-1"):
        patch_heads(x, 8, head(c(4, 8, 3, padding=1), c(8, 4, 1)), None, "fused")
    with pytest.raises(ValueError, match="kernel-1"):
        patch_heads(x, 8, head(c(4, 8, 1, stride=2), c(8, 4, 1)), None, "fused")
    with pytest.raises(ValueError, match="kernel-1"):
        patch_heads(x, 8, head(c(4, 8, 1, groups=2), c(8, 4, 1)), None, "fused")
    with pytest.raises(ValueError, match="kernel-1"):
        patch_heads(x, 8, head(c(4, 8, 1), torch.nn.ReLU(), c(8, 4, 1)), None, "fused")
    with pytest.raises(ValueError, match="kernel-1"):
        patch_heads(x, 8, head(torch.nn.Conv3d(4, 8, 1), c(8, 4, 1)), None, "fused")
    with pytest.raises(ValueError, match="1 to 4"):
        patch_heads(x, 8, head(c(4, 8, 1), c(8, 4, 1)), torch.nn.Sequential(c(4, 4, 1), c(4, 4, 1), c(4, 4, 1)), "fused")
    with pytest.raises(ValueError, match="up to 32"):
        patch_heads(x, 8, head(c(4, 33, 1), c(33, 4, 1)), None, "fused")
    with pytest.raises(ValueError, match="fp32"):
        patch_heads(x.double(), 8, head(c(4, 8, 1), c(8, 4, 1)).double(), None, "fused")
    with pytest.raises(ValueError, match="fp32"):
        patch_heads(x.half(), 8, head(c(4, 8, 1), c(8, 4, 1)).half(), None, "fused")
    with pytest.raises(ValueError, match="route"):
        patch_heads(x, 8, head(c(4, 8, 1), c(8, 4, 1)), None, "hip")
