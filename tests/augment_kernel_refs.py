"""Case tables, inputs and exact references shared by tests/test_augment_kernels_gpu.py (arco_jitter_blur and arco_quantize8 of
csrc/augment.hip called directly, one launch sequence per case) and tests/test_augment_kernels_cpu.py (the reference held to Pillow:
the recordings g12 / g20 always, live Pillow where it is installed; the host-side rejections).  Plain CPU numpy / torch only.

The reference is the integer restatement of oracle/arco_oracle.py (q8, color_jitter_u8, gaussian_blur_u8): every case is a CALL of
arco_jitter_blur - a batch of images [B, C, H, W] with one parameter record each - and its reference is computed per image, once
(functools.lru_cache), and never modified.  Every comparison of the GPU file is exact: no tolerance appears in this module.

A parameter record is dict(order, factors, sigma): order = the permutation of ColorJitter.get_params or None (no jitter), factors =
(brightness, contrast, saturation, hue), sigma = the GaussianBlur radius or None.  The descriptor the kernel takes carries the box
radius, not sigma: desc() packs arco_oracle.gaussian_blur_radius(sigma) (held bit-equal to the package's own restatement in the CPU
file)."""
import functools
import itertools
import struct

import numpy as np
import torch

import arco_oracle as orc
from loss_kernel_refs import SENTINEL, gen

F32 = np.float32
GUARD = 8                                              # sentinel elements kept behind every output buffer and the workspace
MAX_IMG = 32                                           # ARCO_MAX_IMG: images per call
DESC_BYTES = 44

# one sigma per integer box-radius class (fixture_inputs.BLUR_SIGMAS holds the same three): int(radius) = 0, 1, 2
CLASS_SIGMA = (0.5, 2.0, 3.0)
NONE = dict(order=None, factors=None, sigma=None)
JIT = dict(order=(2, 0, 3, 1), factors=(1.2, 0.8, 1.1, 0.1), sigma=None)


def P(order=None, factors=None, sigma=None):
    return dict(order=None if order is None else tuple(order), factors=None if factors is None else tuple(factors), sigma=sigma)


def with_sigma(p, sigma):
    return dict(p, sigma=sigma)


def desc(params):
    """the host descriptor table of arco_jitter_blur: {int order[4]; float f[4]; int jitter, blur; float blur_r;} per image"""
    raw = b""
    for p in params:
        order = p["order"] if p["order"] is not None else (0, 1, 2, 3)
        f = p["factors"] if p["factors"] is not None else (1.0, 1.0, 1.0, 0.0)
        fr = orc.gaussian_blur_radius(p["sigma"]) if p["sigma"] is not None else 0.0
        raw += struct.pack("<4i4fiif", *order, *f, int(p["order"] is not None), int(p["sigma"] is not None), fr)
    assert len(raw) == DESC_BYTES * len(params)
    return raw


def ref_image(x, p):
    """uint8 [C, H, W]: to_pil_image -> ColorJitter -> GaussianBlur of one float image, by the integer restatement"""
    a = orc.q8(x)
    if p["order"] is not None:
        a = orc.color_jitter_u8(a, list(p["order"]), p["factors"])
    if p["sigma"] is not None:
        a = orc.gaussian_blur_u8(a, p["sigma"])
    return a


# ======================================================================================================================================
# images
# ======================================================================================================================================
def rand_image(C, H, W, *seed):
    """uniform [0, 1) with an exact 0 and an exact 1 in the first and last pixel"""
    x = torch.rand((C, H, W), generator=gen(20, C, H, W, *seed)).numpy().astype(F32)
    x.reshape(C, -1)[:, 0] = 0.0
    x.reshape(C, -1)[:, -1] = 1.0
    return x


def levels(a):
    """uint8 levels -> the float32 image (k + 0.5) / 255: q8 gives back k whatever the rounding of the division and the product"""
    return ((np.asarray(a, dtype=F32) + F32(0.5)) / F32(255.0)).astype(F32)


# greys; the three primaries; two-way ties of the maximum r = g > b, g = b > r, r = b > g (twice each); 0 and 255; near-greys; one-level steps
PALETTE = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (1, 1, 1), (254, 254, 254), (77, 77, 77),
           (255, 0, 0), (0, 255, 0), (0, 0, 255),
           (200, 200, 10), (90, 90, 89), (10, 200, 200), (89, 90, 90), (200, 10, 200), (90, 89, 90),
           (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 128, 0), (0, 128, 255), (128, 0, 255),
           (1, 0, 0), (0, 1, 0), (0, 0, 1), (254, 255, 255), (255, 254, 255), (255, 255, 254),
           (12, 34, 56), (56, 34, 12), (34, 56, 12), (250, 5, 127), (127, 250, 5), (5, 127, 250), (100, 150, 200), (200, 150, 100)]


def palette_image(C):
    """5 x 7: the palette above (C = 1: its first channel)"""
    a = np.array(PALETTE, dtype=np.uint8).T.reshape(3, 5, 7)
    return levels(a[:C])


def input_values():
    """exactly k / 255 (fp32 division) and one ulp below, for every k; negative values, values above 1, -0.0, the smallest normal and a
    denormal, 1 and its neighbours.  520 values = a 20 x 26 plane.  No NaN."""
    k = (np.arange(256, dtype=F32) / F32(255.0)).astype(F32)
    below = np.nextafter(k, F32(-1.0)).astype(F32)
    extra = np.array([-0.5, -0.0, 1.5, 1.0, np.nextafter(F32(1), F32(2)), 1e-40, 2.0 ** -126, -1e-40], dtype=F32)
    v = np.concatenate([k, below, extra]).astype(F32)
    assert v.size == 520 and not np.isnan(v).any()
    return v


def half_mean_image(C, k):
    """two pixels k and k + 1 (C = 3: greys, whose luminance is the level itself): the mean luminance is exactly k + 0.5"""
    return levels(np.array([k, k + 1], dtype=np.uint8).reshape(1, 1, 2).repeat(C, 0))


# ======================================================================================================================================
# calls
# ======================================================================================================================================
PLANES = [(1, 1), (1, 2), (2, 1), (1, 7), (3, 3), (5, 2), (7, 9), (31, 33), (32, 32), (33, 65), (64, 1), (1, 64)]
ORDERS24 = list(itertools.permutations(range(4)))
ORDERS_C1 = [(1, 0, 2, 3), (0, 2, 3, 1), (0, 1, 2, 3)]          # contrast first, last, after brightness
FACTORS = (0.0, 1.0, 0.75, 1.25, 2.0)
HUES = (-0.5, -1.0 / 255.0, 0.0, 0.25, 0.5)
KINDS = [NONE, JIT, with_sigma(NONE, CLASS_SIGMA[0]), with_sigma(NONE, CLASS_SIGMA[1]), with_sigma(NONE, CLASS_SIGMA[2]),
         with_sigma(JIT, 0.9)]                        # untouched, jitter only, blur r = 0, 1, 2, jitter + blur
MIXED_ORDERS = [(0, 1, 2, 3, 4, 5), (4, 5, 1, 3, 0, 2)]


def _neutral(op, f, rot):
    """one op at factor f, the other three neutral (1, 1, 1, hue 0), the order rotated by rot"""
    fac = [1.0, 1.0, 1.0, 0.0]
    fac[op] = f
    order = [(op + rot + i) % 4 for i in range(4)]
    return P(order, fac)


def _images(name):
    """[(x [C, H, W] float32, record)] of a call"""
    kind, *a = name.split(":")
    if kind == "plane":                                # every plane in every radius class and unblurred, without and with jitter
        H, W, C = (int(v) for v in a)
        cls = [None, *CLASS_SIGMA]
        return [(rand_image(C, H, W, 8 * j + i), with_sigma(base, s)) for j, base in enumerate((NONE, JIT)) for i, s in enumerate(cls)]
    if kind == "stride":                               # 192 x 192 = 36 864 pixels: second trips of both jitter kernels, 36 blur tiles
        C = int(a[0])
        return [(rand_image(C, 192, 192, 1), P((0, 1, 2, 3), (1.1, 0.8, 1.2, -0.1), 0.9))]
    if kind == "mixed":                                # the six kinds in one call, in one of two orders
        C, o = int(a[0]), int(a[1])
        return [(rand_image(C, 31, 33, 100 + k), KINDS[k]) for k in MIXED_ORDERS[o]]
    if kind == "full":                                 # B = 32 (a full table), or 33 through the package (two chunks)
        C, B = int(a[0]), int(a[1])
        return [(rand_image(C, 7, 9, 200 + i), KINDS[i % 6] if i % 7 else with_sigma(JIT, CLASS_SIGMA[1 + i % 2])) for i in range(B)]
    if kind == "orders":
        C = int(a[0])
        fac = (1.25, 0.75, 1.25, 0.25)
        return [(palette_image(C), P(o, fac)) for o in (ORDERS24 if C == 3 else ORDERS_C1)]
    if kind == "factors":
        C = int(a[0])
        ops = ((0, FACTORS), (1, FACTORS), (2, FACTORS), (3, HUES)) if C == 3 else ((0, FACTORS), (1, FACTORS))
        out = []
        for op, fs in ops:
            for i, f in enumerate(fs):
                out.append((palette_image(C) if i % 2 else rand_image(C, 5, 7, 300 + 10 * op + i), _neutral(op, f, i)))
        return out
    if kind == "pixels":                               # a constant image, mean luminance exactly k + 0.5, extremes
        C = int(a[0])
        const = levels(np.full((C, 1, 2), 93, dtype=np.uint8))
        black, white = levels(np.zeros((C, 1, 2), dtype=np.uint8)), levels(np.full((C, 1, 2), 255, dtype=np.uint8))
        out = []
        for x in (const, black, white, half_mean_image(C, 0), half_mean_image(C, 100), half_mean_image(C, 254)):
            out += [(x, P((1, 0, 2, 3), (1.0, 0.0, 1.0, 0.0))),            # contrast 0: every pixel becomes the truncated mean + 0.5
                    (x, P((0, 2, 3, 1), (1.25, 0.75, 0.75, 0.25))),
                    (x, P((3, 1, 0, 2), (0.75, 1.25, 2.0, -0.5), CLASS_SIGMA[0]))]
        return out
    if kind == "inputs":                               # special float inputs, unjittered / jittered / blurred
        C = int(a[0])
        v = input_values()
        x = np.stack([np.roll(v, 7 * c) for c in range(C)]).reshape(C, 20, 26)
        return [(x, NONE), (x, JIT), (x, with_sigma(JIT, 0.3))]
    raise KeyError(name)


CALLS = ([f"plane:{H}:{W}:{C}" for (H, W) in PLANES for C in (1, 3)] + ["stride:1", "stride:3"] +
         [f"mixed:{C}:{o}" for C in (1, 3) for o in (0, 1)] + ["full:1:32", "full:3:32"] + ["orders:3", "orders:1"] +
         ["factors:3", "factors:1"] + ["pixels:1", "pixels:3"] + ["inputs:1", "inputs:3"])
PACKAGE_CALL = "full:3:33"                             # through arco_amd.augment.jitter_blur only (two chunks of the 32-image table)


@functools.lru_cache(maxsize=None)
def call_case(name):
    imgs = _images(name)
    x = np.stack([im for im, _ in imgs]).astype(F32)
    params = [p for _, p in imgs]
    ref = np.stack([ref_image(im, p) for im, p in imgs])
    B, C, H, W = x.shape
    return dict(name=name, B=B, C=C, H=H, W=W, x=torch.from_numpy(x), params=params, ref=torch.from_numpy(ref.astype(np.int32)),
                desc=desc(params) if B <= MAX_IMG else None)


def single(c, i):
    """image i of a call as a call of its own"""
    return dict(name=f"{c['name']}[{i}]", B=1, C=c["C"], H=c["H"], W=c["W"], x=c["x"][i:i + 1].contiguous(), params=[c["params"][i]],
                ref=c["ref"][i:i + 1], desc=desc([c["params"][i]]))


def check_images(name, out, ref):
    """out [B, C, H, W] fp32 (CPU) against the uint8 reference: round(out * 255) equal, and out * 255 an exact integer (k / 255 values)"""
    out = out.detach().cpu()
    lv = torch.round(out * 255)
    assert torch.equal(out * 255, lv), name + ": an output is not k / 255"
    if not torch.equal(lv.to(torch.int32), ref):
        bad = (lv.to(torch.int32) != ref)
        b = int(bad.flatten(1).any(1).nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} pixels differ from the restatement, first in image {b}: "
                             f"got {lv[b][bad[b]][:4].tolist()} want {ref[b][bad[b]][:4].tolist()}")


# ======================================================================================================================================
# arco_quantize8
# ======================================================================================================================================
QUANT_N = (0, 1, 255, 256, 257, 2048 * 256 + 1)       # ..., one element past the grid cap of 2048 blocks x 256 threads


@functools.lru_cache(maxsize=None)
def quant_case(n):
    """the special inputs (with two more denormals) in front, cycled through a random buffer; the reference: floor-truncation in fp32
    arithmetic, (x * 255f -> int, clipped to 0 .. 255) / 255f"""
    v = input_values()                                                         # (the out-of-range values and the denormals first)
    spec = np.concatenate([v[512:], np.array([1e-45, -1e-45, 1.1754942e-38], dtype=F32), v[:512]])
    x = (torch.rand((n,), generator=gen(21, n)).numpy().astype(F32) * F32(1.5) - F32(0.25)).astype(F32)
    k = np.arange(n)
    x = np.where(k % 3 == 0, spec[(k // 3) % spec.size], x).astype(F32) if n else x
    t = (x * F32(255.0)).astype(F32)
    lv = np.trunc(np.clip(t, F32(0), F32(255))).astype(F32)
    ref = (lv / F32(255.0)).astype(F32) + F32(0.0)                             # (+ 0: the clip of -0.0 is +0 in the kernel)
    return dict(n=n, x=torch.from_numpy(x), ref=torch.from_numpy(ref))


def sentinel_buffer(n, device="cpu"):
    return torch.full((int(n) + GUARD,), SENTINEL, dtype=torch.float32, device=device)
