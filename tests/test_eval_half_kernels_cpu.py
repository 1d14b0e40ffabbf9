"""tests/eval_half_kernel_refs.py held to independent second restatements on the CPU (no library, no GPU).

Pooled apply: every operation in exact rational arithmetic (fractions.Fraction) with an explicit round-to-nearest-even to the binary
format - fp32 after the subtraction, after the product with istd, ONCE after gamma * u + beta (the fused multiply-add), after the
slope; then f16 - on a sample of the elements of every case, the crafted rounding-boundary channels among them.
Arg-max zoom back: plain Python loops over the output pixels (the coordinate in Python floats, a scan with a strict `>`), and
scipy.ndimage.zoom(order=0) of numpy's arg-max map."""
import math
from fractions import Fraction

import numpy as np
import pytest

import eval_half_kernel_refs as R


def _round_binary(q, p, emin):
    """Fraction q -> the nearest value (ties to even) of the binary format with p significand bits and least normal exponent emin
    (fp32: 24, -126; f16: 11, -14), as a Fraction.  Overflow does not occur in these tests."""
    if q == 0:
        return Fraction(0)
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()          # 2^(e-1) <= a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                         # now 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, emin) - (p - 1))
    n = a / quantum
    f = n.numerator // n.denominator
    rem = n - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return s * f * quantum


def _f32(q):
    return _round_binary(q, 24, -126)


def _f16(q):
    return _round_binary(q, 11, -14)


def _element(z, mean, istd, gamma, beta, slope):
    t = _f32(Fraction(float(z)) - Fraction(float(mean)))
    u = _f32(t * Fraction(float(istd)))
    y = _f32(u * Fraction(float(gamma)) + Fraction(float(beta)))
    if y < 0:
        y = _f32(y * Fraction(float(np.float32(slope))))
    return float(_f16(y))


def test_round_binary_on_known_values():
    assert _f16(Fraction(1) + Fraction(1, 2048)) == 1                                  # a tie goes to the even neighbour
    assert _f16(Fraction(1) + Fraction(3, 2048)) == Fraction(1) + Fraction(2, 1024)
    assert _f32(Fraction(1, 3)) == Fraction(float(np.float32(1.0 / 3.0)))
    assert _f16(Fraction(1, 3)) == Fraction(float(np.float16(1.0 / 3.0)))
    assert _f16(Fraction(3, 2 ** 25)) == Fraction(float(np.float16(3.0 / 2 ** 25)))    # subnormal
    assert _f32(-Fraction(16777217)) == -16777216


def test_fma32_rounds_once():
    rs = np.random.RandomState(0)
    a = rs.standard_normal(4000).astype(np.float32)
    b = rs.standard_normal(4000).astype(np.float32)
    c = rs.standard_normal(4000).astype(np.float32)
    # a case where rounding the float64 sum again would go wrong: the product sits a hair above a float32 midpoint
    a[0], b[0], c[0] = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 + 2.0 ** -23), np.float32(2.0 ** -24 - 2.0 ** -45)
    got = R.fma32(a, b, c)
    for i in range(0, 4000, 7):
        want = float(_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))))
        assert float(got[i]) == want, i
    assert float(got[0]) == float(_f32(Fraction(float(a[0])) * Fraction(float(b[0])) + Fraction(float(c[0]))))


@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=R.POOL_IDS)
def test_pooled_apply_reference_equals_exact_rational_restatement(shape, slope):
    c, H, W = shape
    z, mean, istd, gamma, beta = R.pool_case(c, H, W)
    a, pooled = R.ref_bn_act_pool(z, mean, istd, gamma, beta, slope)
    assert a.dtype == np.float16 and a.shape == z.shape and pooled.shape == (R.NB, H // 2, W // 2, c)
    rs = np.random.RandomState(c + H)
    n_el = z.size
    idx = np.unique(np.concatenate([rs.randint(0, n_el, 600), np.arange(0, min(n_el, 64))]))      # (the first channels are the crafted ones)
    zf, af = z.reshape(-1), a.reshape(-1)
    for i in idx:
        ch = int(i % c)
        want = _element(zf[i], mean[ch], istd[ch], gamma[ch], beta[ch], slope)
        assert float(af[i]) == want, (i, ch, float(af[i]), want)
    # the pooled output: the maximum of the four rounded values, window by window
    for n in range(R.NB):
        for yo in range(H // 2):
            for xo in range(0, W // 2, max(1, W // 8)):
                blk = a[n, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2].astype(np.float64).reshape(4, c)
                assert np.array_equal(pooled[n, yo, xo].astype(np.float64), blk.max(axis=0))
    # the crafted channels reach what they were made for: channel 0 is exactly midway, so every result has an even last bit
    pos = z[..., 0] > 0
    assert np.all((a[..., 0][pos].view(np.uint16) & 1) == 0) and pos.any() and (~pos).any()
    assert np.any(a[..., 1][pos] != a[..., 2][pos])              # just above / just below the midpoint round apart
    assert (a[..., 4:] > 0).any() and (a[..., 4:] <= 0).any()


def _argmax_zoom_back_loops(rows, C, out_size):
    n, P0, P1, _ = rows.shape
    N0, N1 = out_size
    z0, z1 = (P0 - 1) / (N0 - 1), (P1 - 1) / (N1 - 1)
    out = np.zeros((n, N0, N1), dtype=np.int64)
    for s in range(n):
        for i in range(N0):
            c0 = i * z0
            if not 0.0 <= c0 <= P0 - 1:
                continue
            for j in range(N1):
                c1 = j * z1
                if not 0.0 <= c1 <= P1 - 1:
                    continue
                row = rows[s, int(math.floor(c0 + 0.5)), int(math.floor(c1 + 0.5))]
                best, bi = float(row[0]), 0
                for k in range(1, C):
                    if float(row[k]) > best:
                        best, bi = float(row[k]), k
                out[s, i, j] = bi
    return out


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "wide"])
@pytest.mark.parametrize("sizes", R.ARGMAX_SIZES, ids=R.ARGMAX_IDS)
@pytest.mark.parametrize("C", R.ARGMAX_CLASSES)
def test_argmax_zoom_back_reference_equals_loops_and_scipy(C, sizes, wide):
    from scipy.ndimage import zoom
    patch, out_size = sizes
    rows = R.argmax_case(C, patch, ld=C + 5 if wide else None)
    logits = rows[..., :C]
    got = R.ref_argmax_zoom_back(logits, out_size)
    assert got.dtype == np.int64 and got.shape == (R.ARGMAX_N,) + out_size
    assert np.array_equal(got, _argmax_zoom_back_loops(rows, C, out_size))
    amax = np.argmax(logits.astype(np.float32), axis=-1)
    sci = np.stack([zoom(amax[s], (out_size[0] / patch[0], out_size[1] / patch[1]), order=0) for s in range(R.ARGMAX_N)])
    assert np.array_equal(got, sci)
    if C >= 2:
        # the cases hold what they promise: exact ties at the maximum, and +0.0 against -0.0
        flat = logits.reshape(-1, C).astype(np.float64)
        assert np.any(np.sum(flat == flat.max(axis=1, keepdims=True), axis=1) >= 2)
        zero_rows = flat.max(axis=1) == 0.0
        assert zero_rows.any() and np.any(np.signbit(logits.reshape(-1, C)[zero_rows]) & (flat[zero_rows] == 0.0))
