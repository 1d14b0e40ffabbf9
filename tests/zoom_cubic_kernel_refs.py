"""References and cases for the cubic-spline zoom kernels (arco_amd/csrc/zoom.hip: arco_spline_prefilter2d, arco_zoom_cubic2d;
arco_amd/utils/zoom_gpu.py: spline_prefilter, zoom_cubic).

The restatement is scipy.ndimage.zoom(a, f, order=3) with scipy's defaults (mode='constant', cval=0, prefilter=True, grid_mode=False)
on one float32 [n0, n1] slice, in numpy float64, every operation rounded once (numpy does not fuse a product into a sum) and in the
order written here; the kernels make the same operations in the same order, so they are held to it bit for bit.

ref_prefilter: axis 0, then axis 1; along every line c[0..n-1] of n >= 2 points, with the pole z = sqrt(3) - 2:
    c[i]    = c[i] * gain                     gain = (1 - z) * (1 - 1 / z)
    zn      = z ** (n - 1)                    Python float64 `**`, on the host for the kernels too
    acc     = c[0] + zn * c[n - 1]
    acc    += zi * (c[i] + zn * c[n - 1 - i]);  zi *= z        i = 1 .. n - 2, zi = z at i = 1
    c[0]    = acc / (1 - zn * zn)
    c[i]    = c[i] + z * c[i - 1]             i = 1 .. n - 1
    c[n-1]  = ((z * c[n - 2] + c[n - 1]) * z) / (z * z - 1)
    c[i]    = z * (c[i + 1] - c[i])           i = n - 2 .. 0
  The initial sum is NOT shortened: it runs over the whole line, whatever its length.  (On a line of 520 points zn = z ** 519 is
  about 1e-297: a normal double, but c[i] + zn * c[n - 1 - i] is c[i] itself for every data of these tests, which is what "the far end
  no longer matters" means there.  From 568 points on zn is 0, and from i = 565 on zi is a denormal and then 0: the 600-point case.)
ref_interpolate: output index o of an axis samples cc = o * step, step = (n_in - 1) / (n_out - 1); the output is 0 where
  !(0 <= cc <= n_in - 1); taps floor(cc) - 1 .. + 2 mirrored into [0, n_in - 1] with period 2 (n_in - 1); with x = cc - floor(cc),
  t = 1 - x:  w1 = (x * x * (x - 2) * 3 + 4) / 6,  w2 = (t * t * (t - 2) * 3 + 4) / 6,  w0 = t * t * t / 6,  w3 = 1 - w0 - w1 - w2
  (every product and sum from left to right);  sum = 0; sum += (c * w_axis0) * w_axis1 over the 16 taps, axis 0 outer; float32(sum).

Against scipy 1.15.3 (tests/test_zoom_cubic_kernels_cpu.py, on every case and variant below): the float32 zoom was identical on every
output; the float64 coefficients deviated from scipy.ndimage.spline_filter by at most MEASURED_COEF_DEV of max|c| (the two do not
round in the same order), and COEF_BOUND = 8 * MEASURED_COEF_DEV is what that test holds them to.

A case is ((S, n0, n1), (N0, N1)); every case has three variants of data: "unit" (values in +-[0.5, 2], nowhere 0), "kilo" (the same
times 1e3) and "const" (every slice one constant)."""
import math

import numpy as np

from zoom_kernel_refs import guarded, guards_intact  # noqa: F401  (the canary margins are shared with the order-0 tests)

Z = math.sqrt(3.0) - 2.0
GAIN = (1.0 - Z) * (1.0 - 1.0 / Z)
ROW_TILE = 32                          # csrc/zoom.hip SPL_TC: columns of a row-pass tile

MEASURED_COEF_DEV = 1.2e-15            # largest |restatement - scipy.ndimage.spline_filter| / max|c| over all cases and variants
COEF_BOUND = 8 * MEASURED_COEF_DEV

CASES = [
    ((2, 2, 3), (10, 8)),              # an axis of 2 points and one of 3: every tap is mirrored.  (No output of the 2-point axis sits on
    ((2, 3, 2), (4, 6)),               # cc = 0.5, where the exact result is a float32 rounding tie for half of all data.)
    ((2, 8, 15), (26, 51)),            # 8 -> 26 and 15 -> 51: zeroed last row and column, upsampling
    ((2, 28, 15), (14, 51)),           # 28 -> 14: zeroed last row, downsampling
    ((2, 15, 28), (51, 14)),           # the same pairs on the other axes: zeroed last column, downsampling
    ((2, 20, 17), (20, 40)),           # axis 0 kept (step exactly 1), axis 1 resampled
    ((2, 13, 24), (30, 24)),           # axis 1 kept
    ((3, 19, 53), (24, 37)),           # three slices, fastest axes 53 and 37: the tail of the 16-byte stores and the slice stride
    ((3, 24, 37), (19, 53)),
    ((2, 70, 75), (33, 40)),           # rows of 75 = 32 + 32 + 11: three row-pass tiles, the last one short; 140 rows = 2 waves + 12 rows
    ((2, 6, 520), (9, 300)),           # a row of 520 points: z ** 519 ~ 1e-297
    ((2, 520, 5), (40, 9)),            # a column of 520 points
    ((2, 12, 9), (20, 21)),            # lines of 12 and 9 points: z ** (n - 1) decides low bits
    ((1, 3, 600), (5, 64)),            # a row of 600 points: z ** 599 is 0 and zi runs through the denormals to 0
    ((1, 600, 3), (64, 5)),            # a column of 600 points
]
IDS = ["%dx%dx%d_%dx%d" % (s + d) for s, d in CASES]
VARIANTS = ("unit", "kilo", "const")


def pole_power(n):
    return Z ** (n - 1)


def image(case, variant):
    """float32 [S, n0, n1]."""
    shape = case[0]
    if variant == "const":
        return np.broadcast_to(np.array([1.5, -0.75, 300.0][:shape[0]], dtype=np.float32)[:, None, None], shape).copy()
    rng = np.random.default_rng(17 * shape[1] + shape[2])
    a = rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return (a * (1e3 if variant == "kilo" else 1.0)).astype(np.float32)


def _filter_lines(c):
    """The prefilter along the LAST axis of the float64 array c [..., n], in place; vectorised over the lines."""
    n = c.shape[-1]
    assert n >= 2
    z, zn = Z, pole_power(n)
    c *= GAIN
    acc = c[..., 0] + zn * c[..., n - 1]
    zi = z
    for i in range(1, n - 1):
        acc += zi * (c[..., i] + zn * c[..., n - 1 - i])
        zi *= z
    c[..., 0] = acc / (1.0 - zn * zn)
    for i in range(1, n):
        c[..., i] = c[..., i] + z * c[..., i - 1]
    c[..., n - 1] = ((z * c[..., n - 2] + c[..., n - 1]) * z) / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[..., i] = z * (c[..., i + 1] - c[..., i])


def ref_prefilter(a, axes=(0, 1)):
    """float64 coefficients [S, n0, n1] of float32 (or, for one pass alone, float64) slices: axis 0 of a slice, then axis 1."""
    c = np.array(a, dtype=np.float64)
    for ax in axes:
        v = np.ascontiguousarray(np.moveaxis(c, 1 + ax, -1))
        _filter_lines(v)
        c = np.ascontiguousarray(np.moveaxis(v, -1, 1 + ax))
    return c


def axis_taps(n_in, n_out):
    """(ok bool [n_out], idx int64 [n_out, 4], w float64 [n_out, 4]) of one axis."""
    step = (n_in - 1) / (n_out - 1)
    cc = np.arange(n_out, dtype=np.float64) * step
    ok = (cc >= 0) & (cc <= n_in - 1)
    cc = np.where(ok, cc, 0.0)
    fl = np.floor(cc)
    x = cc - fl
    t = 1.0 - x
    w = np.empty((n_out, 4), dtype=np.float64)
    w[:, 1] = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 2] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 0] = t * t * t / 6.0
    w[:, 3] = 1.0 - w[:, 0] - w[:, 1] - w[:, 2]
    period = 2 * (n_in - 1)
    idx = (fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :]) % period
    idx = np.where(idx > n_in - 1, period - idx, idx)
    return ok, idx, w


def ref_interpolate(coef, out_size):
    """float32 [S, N0, N1] from float64 coefficients [S, n0, n1]."""
    coef = np.asarray(coef, dtype=np.float64)
    ok0, i0, w0 = axis_taps(coef.shape[1], out_size[0])
    ok1, i1, w1 = axis_taps(coef.shape[2], out_size[1])
    t = np.zeros((coef.shape[0],) + tuple(out_size), dtype=np.float64)
    for a in range(4):
        for b in range(4):
            t += (coef[:, i0[:, a][:, None], i1[:, b][None, :]] * w0[:, a][None, :, None]) * w1[:, b][None, None, :]
    return np.where(ok0[None, :, None] & ok1[None, None, :], t, 0.0).astype(np.float32)


def ref_zoom_cubic(a, out_size):
    return ref_interpolate(ref_prefilter(a), out_size)


def zeroed_edges(case):
    """(last row zeroed, last column zeroed) of the case's output."""
    (_, n0, n1), (N0, N1) = case
    return bool(not axis_taps(n0, N0)[0][-1]), bool(not axis_taps(n1, N1)[0][-1])
