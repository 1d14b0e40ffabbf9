"""Cases, inputs, float64 references, per-element bounds and planted errors shared by tests/test_mma12_kernels_gpu.py (the two
reduced-operand modes of arco_conv3d_fwd on fp32 tensors, mma 1 = f16 and mma 2 = bf16 operands: the MMA == 1 / MMA == 2 branches of
igemm_kernel in csrc/igemm.hip, to_f16x4 / to_bf16x4 of csrc/split_bf16.h, one route per test, called directly) and
tests/test_mma12_kernels_cpu.py (the routes through the host queries, the input conditions, an fp32 emulation of the bounded kind, the
planted errors, the rejections).  Plain CPU torch / numpy only; nothing here touches a GPU.  Built on tests/conv_kernel_refs.py, whose
helpers are imported, not copied.

The contract of the modes.  Both operands are rounded to f16 (mma 1) or bf16 (mma 2), to nearest even - f16 with gradual underflow and
overflow to +-inf, as torch's .half(); the products of two 11-bit or two 8-bit significands are exact in fp32; the accumulation is fp32;
bias and residual are added in fp32 in the epilogue and are not rounded.  So the reference is
    ref = conv64(rne(x), rne(w)) + bias + res          in float64
- the convolution of the ROUNDED operands, not a tolerance around the unrounded one.  The modes exist on the vector-load igemm_kernel
tiles of taps 1 and of taps 27 (DEPTH 3); every other shape runs the fp32 arithmetic of mma 0 whatever the mode (FALLBACK below), and
since the route id does not encode the mode, the data decide which arithmetic ran.

Kinds of input:
  fixed     integers times a power of two (x in 2^-3, w in 2^-5), (sum |x||w| + |b| + |r|) / quantum < 2^24 per output AFTER rounding (and
            before it): any fp32 order is exact, the kernel must equal the float64 reference bit for bit.  TIE channels hold values on
            rounding ties of the mode under test - odd 12-bit integers for f16 (2049 -> 2048, 2051 -> 2052), odd 9-bit integers for bf16
            (257 -> 256, 259 -> 260) - alternately on x (against small integers of w) and on w (against small integers of x), as many
            as the 2^24 budget allows; the other channels hold small integers.  Round-to-nearest-even, truncation and
            round-half-away-from-zero give three different references (asserted).
  impulse   unit impulses, three apart in every axis the kernel spans so that every output is ONE product, against 24-bit weights over
            the whole range of the mode (f16: 2^-26 .. 65520, the subnormal range 2^-24 .. 2^-14 and values within one ulp of 65504
            planted; bf16: 2^-60 .. 2^60): every output is rne(w) or zero, bit for bit.
  select    one +-2^e weight per output channel, every tap used (several passes where N < taps), against 24-bit activations of the same
            range, 20 % zeros: the output is the scaled, shifted rne(x), bit for bit.
  wide      six decades, 20 % zeros, |x| <= 65504 for f16: per ELEMENT |err| <= tol = gamma(taps K + 2) S_r + u |ref|,
            S_r = conv(|rne x|, |rne w|) + |bias| + |res|: one rounding per accumulated exact product plus the two of the epilogue (as
            hconv_kernel_refs takes t32 for the f16 MFMA).  The ratio to MEASURED = 3e-6 S_r is printed, not asserted.
  stats     the shrunk integer data of the fp32 file ({-1, 0, 1} times a power of two: representable in both formats, so this kind
            checks the slabs, not the rounding): the float64 host sum of each group's slab range equals that group's sum y and sum y^2.
  overflow  (mma 1, one small 1x1 case) single-product outputs of the select form with activations 65520 and 1e6, which become +inf:
            the output is what IEEE arithmetic on the rounded operands gives (+-inf where the weight is not zero, NaN = inf * 0 in
            the other channels of that row), compared with equal_nan.  Round-to-nearest with overflow to infinity, not saturation.

Preconditions of the exact kinds (fixed, impulse, select), asserted on the CPU: the rounded reference is representable in fp32, and it
differs from the unrounded reference on at least a quarter of the outputs of every case - a kernel that fell back to fp32 cannot pass."""
import functools
import math

import numpy as np
import torch

import conv_kernel_refs as R
from conv_kernel_refs import C, QUANT, QW, QX, _ints, _wide_values, bf16_rne, bf16_trunc, conv64, im2col
from conv_kernel_refs import equal_bits, representable      # noqa: F401  (used through this module by both test files)
from loss_kernel_refs import U, gamma, gen, worst

MEASURED = R.MEASURED
EXACT = ("fixed", "impulse", "select")
ALL = EXACT + ("wide",)
TWO = ("fixed", "wide")                              # the data-gradient cases, as in the fp32 file
MAXH = 65504.0


# ======================================================================================================================================
# the rounding rules: fp32 tensor -> fp32 tensor holding values of the format
# ======================================================================================================================================
def _np(t):
    return np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)


def rne_f16(x):
    """x.half(): to nearest even, gradual underflow kept, overflow to +-inf"""
    return x.half().float()


def rne_bf16(x):
    return torch.from_numpy(bf16_rne(_np(x))).view(x.shape)


def trunc_f16(x):
    """towards zero onto the f16 grid (subnormals kept)"""
    v = _np(x)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))
    h[over] = np.nextafter(h[over], np.float16(0))
    return torch.from_numpy(h.astype(np.float32)).view(x.shape)


def away_f16(x):
    """to nearest, ties away from zero"""
    v = _np(x).astype(np.float64)
    lo = trunc_f16(x).numpy().astype(np.float64)
    with np.errstate(over="ignore"):
        hi = np.nextafter(lo.astype(np.float16), np.where(v < 0, -np.inf, np.inf).astype(np.float16)).astype(np.float64)
    tie = (lo != v) & (np.abs(v - lo) == np.abs(hi - v))
    out = rne_f16(x).numpy().astype(np.float64)
    out[tie] = hi[tie]
    return torch.from_numpy(out.astype(np.float32)).view(x.shape)


def trunc_bf16(x):
    return torch.from_numpy(bf16_trunc(_np(x))).view(x.shape)


def away_bf16(x):
    b = _np(x).view(np.uint32).astype(np.uint64)
    return torch.from_numpy(((b + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32)).view(x.shape)


def ident(x):
    return x


RNE = {1: rne_f16, 2: rne_bf16}
TRUNC = {1: trunc_f16, 2: trunc_bf16}
AWAY = {1: away_f16, 2: away_bf16}
TIE_BITS = {1: 12, 2: 9}                             # odd integers of this many bits lie on a tie of the mode


def planted(mma):
    """the operand treatments that a wrong kernel could apply, (name, rule for x, rule for w): each must fail the exact kinds"""
    r, other = RNE[mma], RNE[3 - mma]
    return [("operands truncated", TRUNC[mma], TRUNC[mma]), ("only A rounded", r, ident), ("only B rounded", ident, r),
            ("the other format", other, other), ("no rounding", ident, ident), ("ties away from zero", AWAY[mma], AWAY[mma])]


# ======================================================================================================================================
# cases
# ======================================================================================================================================
def _both(name, taps, nv, d3, h, w, k, n, route, **opt):
    return [C(f"{name}-m{m}", taps, m, nv, d3, h, w, k, n, route, "mfma12", **opt) for m in (1, 2)]


# ---- taps 1: the six igemm_kernel<1,..> tiles of the non-split branch (the shapes of the fp32 file's -m0 cases; 64x224 at N = 448 with
# M Npad = 9400 * 448 just over 4096 * 1024), the narrow-shape miss (conv1x1_stream_dispatch refuses mma 1 / 2: M = 257 * 257, K = 16, N = 3
# is conv1x1_narrow_out_kernel<4> in mma 0 and igemm_kernel<1,256,16> here), bias + residual + a column offset, ld_out > N, two stat groups
CASES_1X1 = (
    _both("g256x16", 1, 1, 1, 3, 101, 20, 4, 1256016, bias=True, out_pad=4)
    + _both("g128x32", 1, 2, 1, 9, 17, 48, 19, 1128032, bias=True, res=True, res_pad=5, in_pad=4, in_off=4, stats=2)
    + _both("g32x64", 1, 1, 1, 5, 41, 48, 80, 1032064, bias=True, res=True)
    + _both("g64x64", 1, 1, 1, 61, 100, 48, 100, 1064064, bias=True)
    + _both("g64x224", 1, 1, 1, 94, 100, 32, 448, 1064224, res=True)
    + _both("g128x128", 1, 1, 1, 200, 164, 20, 128, 1128128, bias=True)
    + _both("narrow-miss", 1, 1, 1, 257, 257, 16, 3, 1256016, bias=True, out_pad=1))
# ---- taps 27, rectangular: dispatch_spatial<3> (W a multiple of 16), the smallest shapes of the fp32 file's CASES_3D per tile; one
# single-plane volume; bias + residual + a column offset and two stat groups on v32x32, ld_out > N on v128x16
CASES_RECT = (
    _both("v128x16", 27, 1, 3, 20, 16, 16, 4, 9128016, bias=True, out_pad=4, stats=1)
    + _both("v128x32", 27, 1, 8, 64, 128, 16, 20, 9128032)
    + _both("v64x32", 27, 1, 3, 6, 16, 20, 19, 9064032, bias=True, res=True, out_pad=1)
    + _both("v128x64", 27, 1, 8, 64, 128, 16, 64, 9128064)
    + _both("v64x64", 27, 1, 4, 64, 128, 16, 64, 9064064, bias=True)
    + _both("v64x32w", 27, 1, 2, 64, 128, 16, 64, 9064032, res=True)
    + _both("v32x32", 27, 2, 2, 5, 16, 20, 48, 9032032, bias=True, res=True, res_pad=4, in_pad=4, in_off=4, stats=2)
    + _both("v64x32-plane", 27, 1, 1, 6, 16, 20, 19, 9064032, bias=True))
# ---- taps 27, flat: dispatch_flat3 (ids + 5e5) at the plane widths 7 / 14 / 28 (W + 2 <= IGEMM_FLAT_WPMAX = 64, no multiple of 16).  The
# thresholds are 512 workgroups of flat_blocks = planes * ceil(H (W + 2) / BM) * ceil(Npad / BN): small planes, many of them
CASES_FLAT = (
    _both("f128x16", 27, 1, 3, 9, 14, 16, 12, 9628016, bias=True, res=True, res_pad=4)
    + _both("f128x32", 27, 2, 256, 7, 7, 16, 32, 9628032)                    # 512 planes of 63 positions: 512 tiles
    + _both("f64x32", 27, 1, 3, 7, 7, 32, 19, 9564032, bias=True, out_pad=5)
    + _both("f128x64", 27, 2, 256, 7, 14, 16, 64, 9628064)                   # 512 planes of 112 positions
    + _both("f64x64", 27, 1, 256, 4, 28, 16, 64, 9564064, bias=True)         # 256 planes of 120 positions: 256 | 512 tiles
    + _both("f64x32w", 27, 1, 128, 4, 28, 16, 64, 9564032, res=True)         # 128 | 256 | 512 tiles of 128x64 | 64x64 | 64x32
    + _both("f32x32", 27, 1, 2, 5, 7, 20, 48, 9532032, res=True)
    + _both("f64x32-plane", 27, 1, 1, 7, 7, 32, 19, 9564032, res=True))

CASES = CASES_1X1 + CASES_RECT + CASES_FLAT
FAMILY = {}
for _c in CASES_1X1:
    FAMILY[_c["name"]] = "1x1"
for _c in CASES_RECT:
    FAMILY[_c["name"]] = "3x3x3 rectangular"
for _c in CASES_FLAT:
    FAMILY[_c["name"]] = "3x3x3 flat"
# the data gradient: the same kernels on a mode-1 pack, mma 2 (what ops.py passes for every gradient); dY has N channels, dX K
DGRAD = [C("dgrad-1x1-m2", 1, 2, 1, 1, 5, 41, 80, 48, 1032064, "mfma12", kinds=TWO),
         C("dgrad-3x3x3-m2", 27, 2, 1, 4, 14, 14, 64, 32, 9564032, "mfma12", kinds=TWO)]
# the shapes that run the fp32 arithmetic whatever the mode: 3x3 per plane (igemm_kernel DEPTH 1 and the halo kernel), the scalar-load
# form (K % 4 != 0 or ld_in % 4 != 0: launch_igemm hands the modes to the vector-load instantiations only), the one-channel volume
FALLBACK = (
    _both("fb-3x3-s32x32", 9, 1, 1, 7, 5, 20, 48, 9032032, bias=True, res=True, kinds=("fixed",))
    + _both("fb-3x3-halo", 9, 1, 1, 5, 7, 32, 12, 9932016, kinds=("fixed",))
    + _both("fb-1x1-k19", 1, 2, 1, 7, 23, 19, 2, 1256016, res=True, kinds=("fixed",))
    + _both("fb-1x1-ld21", 1, 2, 1, 7, 23, 20, 2, 1256016, in_pad=1, kinds=("fixed",))
    + _both("fb-3x3x3-k19", 27, 1, 3, 6, 16, 19, 19, 9064032, bias=True, kinds=("fixed",))
    + _both("fb-3x3x3-ld21", 27, 1, 3, 6, 16, 20, 19, 9064032, in_pad=1, kinds=("fixed",))
    + _both("fb-image3", 27, 1, 2, 3, 5, 1, 8, 27701016, bias=True, kinds=("fixed",)))
OVERFLOW = C("overflow-m1", 1, 1, 1, 1, 3, 21, 20, 8, 1256016, "mfma12", kinds=("overflow",))

EVERY = CASES + DGRAD + FALLBACK + [OVERFLOW]
NAMES = [c["name"] for c in EVERY]
assert len(set(NAMES)) == len(NAMES)


def by_name(name):
    return EVERY[NAMES.index(name)]


def names(cases):
    return [c["name"] for c in cases]


def having(kind, cases=None):
    return [c for c in (CASES if cases is None else cases) if kind in c["kinds"]]


# ======================================================================================================================================
# inputs
# ======================================================================================================================================
def tie_channels(c):
    """the channels that hold tie values in the fixed kind, alternately on x and on w: as many as the 2^24 budget allows (a tie value
    below 2^bits against a small integer of at most 3), spread over K as conv_kernel_refs.wide_channels spreads its own"""
    top = 3 * 2 ** TIE_BITS[c["mma"]]
    nt = max(2, min(c["k"], 2 ** 23 // (c["taps"] * top)))
    nt = min(nt, c["k"])
    ch = sorted(set(int(v) for v in (np.arange(nt) * c["k"]) // nt + (c["k"] // nt) // 2))
    return ch[0::2], ch[1::2]                         # (ties on x, ties on w)


def _tie_ints(shape, g, bits):
    """odd integers of `bits` bits, both residues mod 4 and both signs: every one a rounding tie whose three rules disagree pairwise"""
    v = 2 ** (bits - 1) + 1 + 2 * _ints(shape, g, 0, 2 ** (bits - 2) - 1)
    return v * (2 * _ints(shape, g, 0, 1) - 1)


def _range_values(shape, g, mma, zeros):
    """24-bit values over the whole range of the mode: +-m 2^e, m a random 24-bit significand, e uniform"""
    lo, hi = (-26, 15) if mma == 1 else (-60, 60)
    m = 1.0 + torch.randint(0, 2 ** 23, shape, generator=g, dtype=torch.int64).double() / 2 ** 23
    e = torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).double()
    v = m * 2.0 ** e * (2 * torch.randint(0, 2, shape, generator=g, dtype=torch.int64).double() - 1)
    if mma == 1:
        v = v.clamp(-65519.0, 65519.0)                # (65520 is the tie that rounds to infinity: the overflow kind's subject)
    v[torch.rand(shape, generator=g) < zeros] = 0.0
    v = v.float()
    if mma == 1:                                      # planted: within one ulp (32) of 65504, and the subnormal range 2^-24 .. 2^-14
        flat = v.view(-1)
        plant = [65504.0 + 15.75, -(65504.0 - 15.75), 65504.0 - 31.5, 65519.0, 2.0 ** -24 * 1.75, -(2.0 ** -24) * 2.5, 2.0 ** -25 * 1.0001,
                 2.0 ** -25, 2.0 ** -15 * 1.0000001, 2.0 ** -14 * (1 - 2.0 ** -12)]
        for i, p in enumerate(plant[:flat.numel()]):
            flat[(i * 7919) % flat.numel()] = p
    return v


def impulse_rows(c):
    """rows of the unit impulses: every third position of every axis the kernel spans (taps 1: every row), so that every output is at
    most one product and almost every output is one"""
    if c["taps"] == 1:
        return list(range(c["M"]))
    zs = range(0, c["d3"], 3) if c["taps"] == 27 else range(c["d3"])
    return [((v * c["d3"] + z) * c["h"] + y) * c["w"] + x for v in range(c["nv"]) for z in zs for y in range(0, c["h"], 3)
            for x in range(0, c["w"], 3)]


def reference(c, x, w, bias, res, rx, rw):
    """float64: conv64(rx(x), rw(w)) + bias + res, and S of the same operands"""
    xr, wr = rx(x).double(), rw(w).double()
    ref = conv64(xr, wr, c)
    return _epilogue(ref, bias, res), xr, wr


def _epilogue(ref, bias, res):
    for t in (bias, res):
        if t is not None:
            ref = ref + t.double()
    return ref


@functools.lru_cache(maxsize=2)
def _data(name, kind, p):
    c = by_name(name)
    mma = c["mma"]
    g = gen(sum(map(ord, name)), (ALL + ("stats", "overflow")).index(kind), p, 12)
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    bias = res = None
    if kind == "fixed":
        xi, wi = _ints((M, K), g, -3, 3), _ints((N, K, T), g, -3, 3)
        tx, tw = tie_channels(c) if K > 1 else ([0], [])
        for ch in tx:
            xi[:, ch] = _tie_ints((M,), g, TIE_BITS[mma])
        for ch in tw:
            wi[:, ch, :] = _tie_ints((N, T), g, TIE_BITS[mma])
        x, w = xi.float() * QX, wi.float() * QW
        if c["bias"]:
            bias = _ints((N,), g, -2 ** 18, 2 ** 18).float() * QUANT
        if c["res"]:
            res = _ints((M, N), g, -2 ** 18, 2 ** 18).float() * QUANT
    elif kind == "stats":
        px = min(0.5, (8.0 / (T * K)) ** 0.25)
        xi = _ints((M, K), g, -1, 1) * (torch.rand((M, K), generator=g) < 2 * px)
        wi = _ints((N, K, T), g, -1, 1) * (torch.rand((N, K, T), generator=g) < 2 * px)
        x, w = xi.float() * QX, wi.float() * QW
        if c["bias"]:
            bias = _ints((N,), g, -1, 1).float() * QUANT
    elif kind == "impulse":
        x = torch.zeros((M, K))
        rows = torch.tensor(impulse_rows(c))
        x[rows, torch.arange(len(rows)) % K] = 1.0
        w = _range_values((N, K, T), g, mma, 0.0)
    elif kind in ("select", "overflow"):
        x = _range_values((M, K), g, mma, 0.2)
        w = torch.zeros((N, K, T))
        order = list(range(T))
        if T == 27 and c["d3"] == 1:                  # volumes of one plane: the nine taps that see data come first in every pass
            order = order[9:18] + order[:9] + order[18:]
        for n in range(N):
            w[n, (7 * n + 3 + p) % K, order[(n + p * N) % T]] = (-1.0) ** n * 2.0 ** ((n + p) % 7 - 3)
        if kind == "overflow":                        # 65520 (the tie to infinity), 1e6, their negatives, and the largest values that stay finite
            for i, v in enumerate((65520.0, 1e6, -65520.0, -1e6, 65519.996, -65519.996, 3e38)):
                x[(5 * i + 2) % M, (3 * i + 1) % K] = v
    else:
        x = _wide_values((M, K), g, 3, 0.2)
        w = (_wide_values((N, K, T), g, 2, 0.0).double() / math.sqrt(K * T)).float()
        if mma == 1:
            x, w = x.clamp(-MAXH, MAXH), w.clamp(-MAXH, MAXH)
        if c["bias"]:
            bias = _wide_values((N,), g, 1, 0.0)
        if c["res"]:
            res = _wide_values((M, N), g, 3, 0.2)
    d = dict(x=x, w=w, bias=bias, res=res, kind=kind, p=p)
    if kind == "overflow":                            # (element-wise: a BLAS product need not propagate inf * 0 the IEEE way)
        xr, wr = RNE[mma](x).double(), RNE[mma](w).double()
        d["ref"] = (xr[:, None, :] * wr[None, :, :, 0]).sum(2)
        return d
    ref, xr, wr = reference(c, x, w, bias, res, RNE[mma], RNE[mma])
    d["ref"] = ref
    if kind == "wide":
        s = conv64(xr.abs(), wr.abs(), c)
        for t in (bias, res):
            if t is not None:
                s = s + t.double().abs()
        d["S"] = s
    return d


def data(c, kind, p=0):
    """the inputs and the float64 reference on the ROUNDED operands of one case and kind (pass p of the select kind); computed once,
    never modified.  Data-gradient cases: x is dY [M, N of the layer], w the logical mode-1 operand (conv_kernel_refs.forward_weight
    gives the layer's weight), and ref the same sums as float64 autograd (dgrad_autograd below)."""
    return _data(c["name"], kind, p)


def with_rules(c, d, rx, rw):
    """the float64 reference of the same inputs under other operand treatments (the unrounded one: ident, ident)"""
    return reference(c, d["x"], d["w"], d["bias"], d["res"], rx, rw)[0]


def unrounded(c, d):
    return with_rules(c, d, ident, ident)


def dgrad_autograd(c, d):
    """float64 autograd of the forward convolution with ROUNDED operands: the layer's weight rounded, the upstream gradient rounded"""
    rne = RNE[c["mma"]]
    x0 = torch.zeros((c["M"], c["n"]), dtype=torch.float64, requires_grad=True)
    y = conv64(x0, rne(R.forward_weight(d)).double(), c)
    return torch.autograd.grad(y, x0, rne(d["x"]).double())[0]


def select_passes(c):
    return R.select_passes(c)


def n_roundings(c):
    return c["taps"] * c["k"] + 2


def tol_wide(c, d):
    return gamma(n_roundings(c)) * d["S"] + U * d["ref"].abs()


def held(name, got, c, d):
    """the wide kind: err / derived bound (asserted <= 1 by the callers) and err / (3e-6 S_r) (printed only)"""
    r1, r2 = worst(got, d["ref"], tol_wide(c, d)), worst(got, d["ref"], MEASURED * d["S"])
    print(f"{name}: worst err / bound {r1:.4f}, err / (3e-6 S_r) {r2:.3f}")
    return r1, r2


def stats_tol(c, d, groups):
    """the BatchNorm partials of the wide kind, as conv_kernel_refs.stats_tol with this file's per-element bound: every output off by
    at most its own bound, the fp32 partial sums of at most Mg = M / G values in any order"""
    t, a = tol_wide(c, d), d["ref"].abs()
    gm = gamma(c["M"] // groups + 1)
    g = lambda v: v.view(groups, c["M"] // groups, -1).sum(1)
    e2 = t * (2 * a + t)
    return g(t) + gm * g(a + t), g(e2) + gm * g(a * a + e2)


def differs(a, b):
    """the share of the outputs on which two references differ"""
    return float((a != b).double().mean())


def emulate(c, d, ulps=0):
    """the wide kind in fp32 numpy: rounded operands, exact products (formed in float64: 22 or 16 bits), fp32 accumulation in k order,
    bias and residual in the epilogue.  ulps: a planted error - every accumulation lands that many ulps further from zero."""
    f32 = np.float32
    rne = RNE[c["mma"]]
    cols_ = im2col(rne(d["x"]), c).numpy().astype(np.float64)                # [M, T, K]
    w = rne(d["w"]).permute(0, 2, 1).contiguous().numpy().astype(np.float64)  # [N, T, K]
    M, T, K = cols_.shape
    acc = np.zeros((M, w.shape[0]), dtype=f32)
    for t in range(T):
        for k in range(K):
            acc = (acc.astype(np.float64) + cols_[:, t, k][:, None] * w[:, t, k][None, :]).astype(f32)
            for _ in range(ulps):
                acc = np.nextafter(acc, np.where(acc < 0, -np.inf, np.inf).astype(f32))
    if d["bias"] is not None:
        acc = (acc + d["bias"].numpy()[None, :]).astype(f32)
    if d["res"] is not None:
        acc = (acc + d["res"].numpy()).astype(f32)
    return torch.from_numpy(acc)
