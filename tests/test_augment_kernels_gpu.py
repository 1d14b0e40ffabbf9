"""arco_jitter_blur and arco_quantize8 of csrc/augment.hip called DIRECTLY (arco_amd._lib), one call of the case table per test, against
the integer restatement of Pillow's 8-bit arithmetic (oracle/arco_oracle.py q8 / color_jitter_u8 / gaussian_blur_u8, through
tests/augment_kernel_refs.py) computed on the CPU from the same float inputs - not through a golden file: tests/test_augment_kernels_cpu.py
holds that restatement to Pillow itself (recordings g12 / g20, and live Pillow on every image of this file's case table).  The output
buffer and the workspace (2 B + B C H W floats) are prefilled with a sentinel and carry GUARD sentinel elements behind them, which
must survive.

Every comparison is exact: torch.equal on round(out * 255) against the uint8 reference and on out * 255 == round(out * 255)
(every output is k / 255); arco_quantize8 bit for bit against floor-truncation in fp32 arithmetic.  No toleranced test, hence no
worst err / bound table: on an MI355X every case of this file passed, and the kernels and the restatement disagreed nowhere.

What the cases reach that the Pillow recordings of g12 do not: blur_to_tensor_kernel<2> (box radius 2 ... 3), planes smaller than the
kernel's halo (1 x 1 ... 3 x 3) and of more than one tile, batches that mix the three box-radius classes (the blur = -1 masking of
the one-launch-per-class loop), the full 32-image descriptor table, the second trip of both grid-stride loops (192 x 192), all 24
op orders, factors 0 / 1 / 2 and the ends of the hue range, two-way ties of the HSV maximum, the + 0.5 truncation of the contrast mean,
and inputs on both sides of every k / 255 threshold, negative, above 1 and -0.0."""
import pytest
import torch

import augment_kernel_refs as A
from augment_kernel_refs import GUARD, SENTINEL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def run(L, c):
    """one arco_jitter_blur call -> out [B, C, H, W] on the CPU; the guards behind out and behind the workspace hold"""
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    n = B * C * H * W
    x = c["x"].contiguous().to(DEV)
    out, ws = A.sentinel_buffer(n, DEV), A.sentinel_buffer(2 * B + n, DEV)
    L.call("arco_jitter_blur", L.ptr(x), B, C, H, W, c["desc"], L.ptr(ws), L.ptr(out))
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()) and out.numel() == n + GUARD, c["name"] + ": the guard behind out was written"
    assert bool((ws[2 * B + n:] == SENTINEL).all()), c["name"] + ": the guard behind the workspace was written"
    assert torch.equal(x.cpu(), c["x"])                                                   # the input is read only
    return out[:n].cpu().view(B, C, H, W)


@pytest.mark.parametrize("name", A.CALLS)
def test_jitter_blur(L, name):
    c = A.call_case(name)
    A.check_images(name, run(L, c), c["ref"])


@pytest.mark.parametrize("name", [n for n in A.CALLS if n.startswith("mixed")])
def test_jitter_blur_mixed_batch_equals_single_image_calls(L, name):
    """untouched, jitter only, blur r = 0 / 1 / 2 and jitter + blur images in one call: each image equals its own B = 1 call bit for bit"""
    c = A.call_case(name)
    got = run(L, c)
    for i in range(c["B"]):
        s = A.single(c, i)
        one = run(L, s)
        A.check_images(s["name"], one, s["ref"])
        assert torch.equal(got[i:i + 1].view(torch.int32), one.view(torch.int32)), (name, i)


def test_jitter_blur_33_images_through_the_package():
    """B = 33 = two chunks of the 32-image table, through arco_amd.augment.jitter_blur (its own descriptor packing and box radius)"""
    from arco_amd import augment
    c = A.call_case(A.PACKAGE_CALL)
    params = [dict(order=None if p["order"] is None else list(p["order"]), factors=p["factors"], sigma=p["sigma"]) for p in c["params"]]
    out = augment.jitter_blur(c["x"].to(DEV), params)
    assert out.shape == c["x"].shape and out.dtype == torch.float32
    A.check_images(A.PACKAGE_CALL, out, c["ref"])


@pytest.mark.parametrize("n", A.QUANT_N)
def test_quantize8(L, n):
    c = A.quant_case(n)
    x = c["x"].to(DEV) if n else torch.zeros(1, device=DEV)
    out = A.sentinel_buffer(n, DEV)
    L.call("arco_quantize8", L.ptr(x), n, L.ptr(out))
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()) and out.numel() == n + GUARD
    got = out[:n].cpu()
    assert torch.equal(got.view(torch.int32), c["ref"].view(torch.int32))                 # bit for bit (no -0.0, no NaN)
    assert torch.equal(got * 255, torch.round(got * 255))                                 # every output is k / 255
