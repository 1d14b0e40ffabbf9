"""References and cases for the two kernels of the f16 inference route (`ops.eval_half`):

  arco_bn_act_pool_fwd_h (csrc/elementwise.hip) ref_bn_act_pool: the pooled BatchNorm apply pass on f16 storage
  arco_argmax_zoom_back2d_h (csrc/zoom.hip)     ref_argmax_zoom_back: the arg-max of f16 logit rows, zoomed back by order 0

ref_bn_act_pool restates bn_act_fwd_kernel<_Float16>'s arithmetic operation for operation: in fp32 t = z - mean, u = t * istd,
y = fma(u, gamma, beta) (the compiler contracts the last product and the sum: ONE rounding; `fma32` below gives that rounding exactly,
from the exact float64 product and an error-free sum), a = y >= 0 ? y : y * slope, then one rounding to f16 (nearest even), then the
maximum of the 2 x 2 block of the ROUNDED values.  Results in the normal float32 range (the cases below stay in it).

ref_argmax_zoom_back: the first maximum of every row in class order, -0.0 == +0.0 (numpy's argmax in float64), sampled by scipy's
order-0 coordinate rule as tests/zoom_kernel_refs.py states it (0 where the rule reads outside the map).  The kernel takes the first
strict maximum of the row's fp32 softmax probabilities (glue.hip's softmax_rows, include/arco_hip.h): the same class whenever distinct
logits of a row give distinct fp32 probabilities - the cases below hold multiples of 1/8 in [-4, 4], whose probabilities differ by
a factor of exp(1/8) at least - and equal logits give equal probabilities, so ties fall the same way.

tests/test_eval_half_kernels_cpu.py holds both to independent second restatements (exact rational arithmetic with an explicit
rounding; plain Python loops) on the cases below."""
import numpy as np

import zoom_kernel_refs as zr

# ---- pooled apply ---------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(16, 64, 48), (32, 32, 32), (256, 4, 6), (16, 2, 2)]       # (c, H, W); two images each
POOL_IDS = ["c%d_%dx%d" % s for s in POOL_SHAPES]
SLOPES = [0.0, 0.01]
CAT_ROOMS = [0, 16]
NB = 2


def fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays with a single rounding.  The product of two float32 is exact in float64; s = p + c is
    rounded to float64 with the residual known exactly (TwoSum), so the one case where rounding s again to float32 differs from rounding
    the exact sum - s exactly midway between two float32 with a non-zero residual - is decided by the residual's sign."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    lo = np.where(r64 <= s, r, np.nextafter(r, np.float32(-np.inf)))
    hi = np.where(r64 >= s, r, np.nextafter(r, np.float32(np.inf)))
    tie = (lo != hi) & ((s - lo.astype(np.float64)) == (hi.astype(np.float64) - s)) & (err != 0)
    return np.where(tie, np.where(err > 0, hi, lo), r).astype(np.float32)


def ref_bn_act_pool(z, mean, istd, gamma, beta, slope):
    """z float16 [N, H, W, C] (channels-last rows), the four parameters float32 [C], slope a Python float ->
    (a float16 [N, H, W, C], pooled float16 [N, H / 2, W / 2, C])."""
    z = np.asarray(z)
    assert z.dtype == np.float16
    mean, istd, gamma, beta = (np.asarray(v, dtype=np.float32) for v in (mean, istd, gamma, beta))
    t = z.astype(np.float32) - mean
    u = t * istd
    y = fma32(u, gamma, beta)
    y = np.where(y >= 0, y, y * np.float32(slope)).astype(np.float32)
    a = y.astype(np.float16)
    n, h, w, c = a.shape
    blk = a.reshape(n, h // 2, 2, w // 2, 2, c)
    pooled = np.maximum(np.maximum(blk[:, :, 0, :, 0], blk[:, :, 0, :, 1]), np.maximum(blk[:, :, 1, :, 0], blk[:, :, 1, :, 1]))
    return a, pooled


def pool_case(c, H, W, seed=0):
    """(z float16 [NB, H, W, c], mean, istd, gamma, beta float32 [c]).  Channels 4 .. c-1: statistics of a trained layer (mean and
    beta of either sign, istd = rsqrt(var + eps), gamma in 0.5 .. 1.5) on z ~ N(0, 2): activations on both sides of zero.
    Channels 0 .. 3 sit on f16 rounding boundaries: z = +-(1 + k / 1024), mean 0, istd 1, gamma 1 and beta = 2^-11 (channel 0: y is
    EXACTLY midway between two f16 - ties to even), 2^-11 +- 2^-20 (channels 1, 2: just above / below the midpoint) and -2^-11
    (channel 3); the negative ones go through the slope first."""
    rs = np.random.RandomState(1000 * c + 10 * H + W + seed)
    z = (rs.standard_normal((NB, H, W, c)) * 2.0).astype(np.float16)
    mean = rs.standard_normal(c).astype(np.float32)
    var = rs.uniform(0.25, 4.0, c).astype(np.float32)
    istd = (1.0 / np.sqrt(var.astype(np.float64) + 1e-5)).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, c).astype(np.float32)
    beta = (rs.standard_normal(c) * 0.5).astype(np.float32)
    k = rs.randint(0, 1024, size=(NB, H, W, 4))
    sign = rs.choice([-1.0, 1.0], size=(NB, H, W, 4))
    z[..., :4] = (sign * (1.0 + k / 1024.0)).astype(np.float16)
    mean[:4], istd[:4], gamma[:4] = 0.0, 1.0, 1.0
    beta[:4] = np.array([2.0 ** -11, 2.0 ** -11 + 2.0 ** -20, 2.0 ** -11 - 2.0 ** -20, -2.0 ** -11], dtype=np.float32)
    return z, mean, istd, gamma, beta


# ---- arg-max zoom back ----------------------------------------------------------------------------------------------------------------
ARGMAX_CLASSES = [1, 2, 4, 32]
ARGMAX_SIZES = [((8, 8), (8, 8)), ((8, 8), (5, 7)), ((4, 6), (9, 5))]      # (P0, P1) -> (N0, N1)
ARGMAX_IDS = ["%dx%d_to_%dx%d" % (p + s) for p, s in ARGMAX_SIZES]
ARGMAX_N = 2
PAD = 100.0               # what the columns behind the classes of a wide row hold: larger than any logit, never to be read


def ref_argmax_zoom_back(logits, out_size):
    """logits [n, P0, P1, C] (any float dtype) -> int64 [n, N0, N1]."""
    amax = np.argmax(np.asarray(logits).astype(np.float64), axis=-1).astype(np.int64)
    return zr.ref_zoom(amax, out_size)


def argmax_case(C, patch, ld=None, seed=0):
    """float16 rows [ARGMAX_N, P0, P1, ld] (ld = C: dense; ld > C: the columns behind the classes hold PAD): multiples of 1/8 in
    [-4, 4]; every third pixel has its maximum copied to another class (an exact tie, before or behind the first maximum); every
    fifth pixel (C >= 2) is <= 0 everywhere with one +0.0 and one -0.0 in either order (equal: the first of the two wins)."""
    P0, P1 = patch
    ld = C if ld is None else ld
    rs = np.random.RandomState(100 * C + 10 * P0 + P1 + seed)
    x = (rs.randint(-32, 33, size=(ARGMAX_N, P0, P1, C)) / 8.0).astype(np.float16)
    flat = x.reshape(-1, C)
    for r in range(flat.shape[0]):
        if C >= 2 and r % 3 == 0:
            flat[r, rs.randint(C)] = flat[r].max()
        if C >= 2 and r % 5 == 0:
            flat[r] = -np.abs(flat[r]) - np.float16(0.125)
            i, j = rs.choice(C, 2, replace=False)
            flat[r, i], flat[r, j] = np.float16(0.0), np.float16(-0.0)
    rows = np.full((ARGMAX_N, P0, P1, ld), PAD, dtype=np.float16)
    rows[..., :C] = flat.reshape(ARGMAX_N, P0, P1, C)
    return rows
