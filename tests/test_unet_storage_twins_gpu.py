"""Storage invariance of the U-Net pooling, resize and first-layer kernels, bit for bit.  Each of these operators is ONE kernel
template over the storage type (csrc/elementwise.hip: maxpool2_fwd / maxpool2_bwd / bn_act_pool_fwd / bilinear_fwd / bilinear_bwd
_kernel<T, V>; csrc/igemm.hip: conv3x3_image_kernel<TOut>): fp32 arithmetic on the loaded values, one rounding per stored value.  So
for f16-representable inputs the `_h` entry on the f16 tensor must equal the plain entry on x.float(), rounded once to f16 - compared
here as int16 views, no tolerance.  (The float64 bounds of these kernels: tests/test_unet_ops_edges_gpu.py.)"""
import pytest
import torch

import test_unet_ops_edges_gpu as E

pytestmark = pytest.mark.gpu

DEV = E.DEV


def both(t):
    """The same f16-representable values as (fp32, f16) channels-last device tensors."""
    assert torch.equal(t.half().float(), t)
    return E.dev(t, "f"), E.dev(t, "h")


def assert_once_rounded(got_h, got_f, tag):
    """The f16 result equals the fp32 result rounded once to f16, as bits."""
    assert got_h.dtype == torch.float16 and got_f.dtype == torch.float32, tag
    want = got_f.half()
    diff = int((E.bits(got_h) != E.bits(want)).sum())
    print(f"{tag}: {diff} of {want.numel()} stored values differ")
    assert diff == 0, (tag, diff)


# ---- max-pool -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 4, 6), (1, 24, 2, 2)])
def test_maxpool_forward_and_backward(shape):
    """Inputs with ties (tie_input); gradients and skip gradients are integers / 8 in [-8, 8]: the fp32 sum is exact and rounds once."""
    from arco_amd import ops
    nb, c, h, w = shape
    g = torch.Generator().manual_seed(100 * c + h)
    x = E.tie_input(3 * c + w, nb, c, h, w)
    assert E.tie_share(x) > 0.2
    dy = torch.randint(-64, 65, (nb, c, h // 2, w // 2), generator=g).float() / 8
    dskip = torch.randint(-64, 65, (nb, c, h, w), generator=g).float() / 8
    out = []
    for xs, dys, dss in zip(both(x), both(dy), both(dskip)):
        x1 = xs.detach().requires_grad_(True)
        y1 = ops.maxpool2(x1)
        y1.backward(dys)
        x2 = xs.detach().requires_grad_(True)
        y2, skip = ops.maxpool2_skip(x2)
        torch.autograd.backward([y2, skip], [dys, dss])
        out.append((y1.detach(), x1.grad, x2.grad))
    for name, f, hh in zip(("forward", "backward", "backward + skip gradient"), *out):
        assert_once_rounded(hh, f, f"maxpool {shape} {name}")


# ---- bn_act_pool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.01, 0.0])
@pytest.mark.parametrize("nb,c,h,w,groups,wide", [(2, 8, 4, 6, 1, False),      # 16-byte lanes
                                                  (2, 8, 4, 6, 2, False),      # per-group statistics
                                                  (2, 12, 4, 6, 1, False),     # 8-byte lanes (f16 rows of 24 bytes)
                                                  (2, 8, 4, 6, 1, True)])      # the output inside a buffer with lda = 2 C
def test_bn_act_pool(nb, c, h, w, groups, wide, slope):
    """Full-resolution and pooled output (rounding is monotone: the maximum of the rounded values is the rounded maximum).  Slope 0
    stores zeros whose sign depends on the storage (a negative value that rounds to zero), so there the VALUES are compared, and the
    bits only where the value is not zero."""
    from arco_amd import _lib as L
    g = torch.Generator().manual_seed(1000 * c + 10 * groups + wide)
    z = torch.randn((nb, c, h, w), generator=g).half().float()
    mean = torch.randn((groups, c), generator=g).mul(0.3).to(DEV)
    istd = torch.rand((groups, c), generator=g).add(0.5).to(DEV)
    gamma = torch.rand((c,), generator=g).add(0.5).to(DEV)
    beta = torch.randn((c,), generator=g).mul(0.2).to(DEV)
    res = []
    for zs in both(z):
        zr = zs.permute(0, 2, 3, 1)                                           # [nb, h, w, c] rows, contiguous
        assert zr.is_contiguous()
        lda = 2 * c if wide else c
        abuf = torch.full((nb, h, w, lda), 99.0, dtype=zs.dtype, device=DEV)
        p = torch.empty((nb, h // 2, w // 2, c), dtype=zs.dtype, device=DEV)
        L.call(L.h("arco_bn_act_pool_fwd", zr), L.ptr(zr), c, nb, h, w, c, L.ptr(mean), L.ptr(istd), L.ptr(gamma), L.ptr(beta),
               float(slope), L.ptr(abuf), lda, L.ptr(p), c, groups)
        assert bool((abuf[..., c:] == 99.0).all())                            # the trailing channels of the buffer are untouched
        res.append((abuf[..., :c].contiguous(), p))
    for name, f, hh in zip(("activation", "pooled"), *res):
        tag = f"bn_act_pool {(nb, c, h, w, groups)} lda={'2C' if wide else 'C'} slope={slope} {name}"
        if slope != 0.0:
            assert_once_rounded(hh, f, tag)
            continue
        want = f.half()
        assert torch.equal(hh.float(), want.float()), tag                     # values (-0.0 == +0.0)
        nz = want != 0
        assert torch.equal(E.bits(hh)[nz], E.bits(want)[nz]), tag
        print(f"{tag}: values equal; {int((~nz).sum())} zeros of {want.numel()}")


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [8, 24])
@pytest.mark.parametrize("shape", [(3, 5, 6, 10), (4, 4, 7, 5), (1, 3, 4, 3), (6, 6, 3, 4)])      # (hi, wi, ho, wo): x2, odd, a side of 1, down
def test_resize_forward_and_adjoint(shape, c):
    """Both storage types evaluate ac_src and bl_blend1 (csrc/interp.h) on the same fp32 values; the adjoint adds w * g in one order."""
    from arco_amd import ops
    hi, wi, ho, wo = shape
    g = torch.Generator().manual_seed(hi * 1000 + wi * 100 + ho * 10 + wo + c)
    x = torch.randn((2, c, hi, wi), generator=g).half().float()
    dy = torch.randn((2, c, ho, wo), generator=g).half().float()
    out = []
    for xs, dys in zip(both(x), both(dy)):
        x1 = xs.detach().requires_grad_(True)
        y = ops.bilinear(x1, (ho, wo))
        y.backward(dys)
        out.append((y.detach(), x1.grad))
    for name, f, hh in zip(("forward", "adjoint"), *out):
        assert_once_rounded(hh, f, f"resize {hi}x{wi} -> {ho}x{wo} c={c} {name}")


# ---- first layer ----------------------------------------------------------------------------------------------------------------------
def test_first_layer_forward():
    """fp32 image of K channels -> 16 channels, 17 x 19 (ragged 16 x 16 tiles), for every K whose fp32 launch takes the streaming
    kernel conv3x3_image_kernel (route id 9.8e6 + 1000 K + 16; K = 1 may take the matrix-core image kernel: not a twin).  Outputs
    only: the BatchNorm statistics of the two modes are sums over different values."""
    from arco_amd import _lib as L
    from arco_amd import ops
    covered = []
    for k in (1, 2, 3, 4):
        g = torch.Generator().manual_seed(40 + k)
        x = E.nhwc(torch.rand((2, k, 17, 19), generator=g).to(DEV))
        wt = (torch.randn((16, k, 3, 3), generator=g) / 3).to(DEV)
        b = torch.randn((16,), generator=g).to(DEV)
        with torch.no_grad():
            with ops.open_half(False):
                yf = ops.conv(x, wt, b)
            route = L.query("arco_conv_last_route")
            if route != 9800000 + 1000 * k + 16:
                print(f"first layer K={k}: fp32 route {route} is not the streaming kernel")
                continue
            with ops.open_half(True):
                yh = ops.conv(x, wt, b)
        assert_once_rounded(yh, yf, f"first layer K={k}")
        covered.append(k)
    assert 3 in covered, covered
