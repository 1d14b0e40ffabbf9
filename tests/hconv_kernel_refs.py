"""Cases, inputs, float64 references, per-element bounds and comparison helpers shared by tests/test_hconv_kernels_gpu.py (every forward
and data-gradient route of the f16-storage convolutions: csrc/conv_h.hip and the f16 epilogue of conv3d_image_kernel<3> in igemm.hip,
mma 4, one route per test, called directly) and tests/test_hconv_kernels_cpu.py (the routes asserted through the host queries, the
input conditions, an fp32 emulation of the bounded kind inside the same bounds, planted errors).  Plain CPU torch / numpy only; nothing
here touches a GPU.  Built on tests/conv_kernel_refs.py (the fp32 and split-bf16 routes), whose helpers are imported, not copied.

A CASE names one route and its smallest shape: the kernel id (include/arco_hip.h) that the dispatcher must choose, which the GPU file
asserts through arco_conv_last_route and the CPU file through arco_conv_config_mma(..., 4) where the query describes the route (the two
streaming 1x1 kernels are launch-only: their dispatch conditions are restated in the CPU file).  Activations are f16 rows [M, K]
(channels last), M = nv * d3 * h * w; weights are in the torch layout [N, K, taps], packed by arco_pack_conv_weight(mode 4), the data
gradient by mode 1 | 4.  The one-channel volume (fam "image") takes an fp32 volume and the fp32 pack.  The tile thresholds of
hconv_dispatch2 / hconv_dispatch3 are HCONV_WANT_BLOCKS = 256 workgroups.

Kinds of input.  All values are f16-representable (except the fp32 volume and weights of the image family's wide kind):
  fixed     x = integers times QX = 2^-14, w[n] = integers times a per-channel power of two, (sum|x||w| + |b|) / quantum < 2^24 per
            output, quantum q_n = QX QW_n: every product and every partial sum in any order is exact in fp32, the float64 reference is
            exactly representable in fp32 (asserted), and the expected output is that reference rounded ONCE to f16, to nearest even.
            One input channel (the last, where K >= 2) holds odd 11-bit integers.  Output channels by flavour (even n exact, odd n in
            turn sub, tie, big):
              exact  at most 600 weights of +-1 off the 11-bit channel, |bias| <= 200 quanta: |ref| / q < 2^11 - the store is an
                     identity and the output equals float64 bit for bit;
              sub    q = 2^-28, |ref| < 2^14 q = 2^-14: every output lies in the f16 SUBNORMAL range (spacing 2^-24 = 16 q) and is
                     rounded there, ties (ref / q = 8 mod 16) among them;
              tie    the 11-bit channel times 3 plus small terms: |ref| / q in the thousands, where every odd multiple of q in
                     [2^11, 2^12) q is an exact tie between two f16 values;
              big    two 11-bit x 11-bit products per output and a bias of up to 2^18 quanta: up to 24 significant bits, |ref| < 65504.
            K = 1: the 1 -> N stream's only channel is the 11-bit one (exact channels: one weight of +-1, no bias); the one-channel volume
            keeps |x| <= 3 and puts the 11-bit integers into the weights of its tie and big channels.
  impulse   unit impulses against random weights over the whole f16 range (random finite bit patterns), subnormal weights and +-65504
            planted among them: every output is one weight or zero, bit for bit.
  select    one +-2^e weight per output channel (e = 0 .. 3: scaling up is exact, subnormals included), every tap used (several passes
            where N < taps), against activations of random bit patterns below 2^13, subnormals planted: the output is the scaled shifted
            input, zero past the border, bit for bit.  This is the kind that shows whether the f16 matrix-core path keeps subnormal
            operands.
  wide      four decades inside the normal range (non-zero magnitudes below 2^-14 are raised to 2^-14), 20 % exact zeros, rounded to
            f16: per ELEMENT |err| <= t32 + 2^-11 (|ref| + t32) + 2^-25, t32 = gamma_n(n) S, S = conv(|x|,|w|) + |b|, u = 2^-24.
  stats     the fixed kind shrunk into the subnormal range: x in {-1, 0, 1} 2^-14, w small integers times 2^-14, so every rounded output
            is an integer number of SQ = 2^-24 (the f16 subnormal spacing) and so is every BatchNorm slab; sum y^2 of the rounded and of
            the unrounded values differ (asserted), so a kernel that summed its fp32 accumulators fails the `==`.

Bound of the wide kind.  The kernel forms fp32 sums of products and rounds once to f16.  t32 bounds the fp32 sum: n roundings of
relative size u, each on a partial sum of magnitude <= S, gamma_n(n) S (wgrad_kernel_refs.gamma_n: gamma(n), or LAMBDA sqrt(n) u where
that is smaller).  The store rounds the fp32 value v, |v| <= |ref| + t32, to f16: relative 2^-11 in the normal range, absolute 2^-25
(half the subnormal spacing) below it.  n, the count of accumulations behind one output:
  MFMA routes (hconv_kernel, hconv_rw_kernel, hconv_fc_kernel)   taps K + 1: a product of two 11-bit significands has 22 bits and is exact
         in fp32, so each of the taps K products costs one rounding as it is accumulated, in whatever order the hardware adds the 32 k of
         one v_mfma_f32_16x16x32_f16; the zero rows and zero padding add exact zeros; + 1 for the bias in the epilogue.
  hconv1x1_narrow_out_kernel<Q>   x0 w0 exact (1 rounding as fp32), 7 fmaf, log2 Q butterfly additions, + bias: 9 + log2 Q <= K + 1
         (K = 8 Q); hconv1x1_narrow_in_kernel: K fmaf onto the bias: K (<= K + 1).
  one-channel volume (conv3d_image_kernel<3>, fp32 operands, v_mfma_f32_16x16x4f32)   a product of two fp32 values is not
         representable: at most one rounding for it and one for its accumulation, onto the bias: 2 taps + 1.
Nothing here is a measured figure.  BatchNorm partials of the wide kind: every output within its own bound, the fp32 sums of at most
Mg = M / G values in any order, gamma(Mg + 1) (stats_tol, as in conv_kernel_refs.py)."""
import functools
import math

import numpy as np
import torch

from conv_kernel_refs import (_ints, _wide_values, ceil_to, conv64, dgrad_autograd, forward_weight, im2col, impulse_positions,
                              representable, select_passes, slab_sums, stat_totals)
from loss_kernel_refs import gamma, gen, worst
from wgrad_kernel_refs import LAMBDA, gamma_n

ERR_ARG, ERR_UNSUPPORTED = -1, -3
ALL = ("fixed", "impulse", "select", "wide")
WANT = 256                                           # HCONV_WANT_BLOCKS
MAXH = 65504.0
SUBN = 2.0 ** -14                                    # smallest normal f16
SQ = 2.0 ** -24                                      # f16 subnormal spacing
FAMS = ("h2d", "h3d", "h1x1", "rw", "fc", "nout", "nin", "image")


def C(name, taps, nv, d3, h, w, k, n, route, fam, **opt):
    c = dict(name=name, taps=taps, nv=nv, d3=d3, h=h, w=w, k=k, n=n, route=route, fam=fam, in_pad=0, in_off=0, out_pad=0, out_shift=0,
             bias=False, stats=0, fl=None, launch_only=False, grouped=False, kinds=ALL, mma=4)
    assert set(opt) <= set(c), opt
    c.update(opt)
    c["M"] = nv * d3 * h * w
    c["ld_in"], c["ld_out"] = k + c["in_pad"], n + c["out_pad"]
    return c


# ---- hconv_kernel<9, BM, BN, .., DEPTH 1>: 3x3 on 2-D maps (hconv_dispatch2), all eight tiles ----------------------------------------
# blocks(bm, bn) = NB ceil(H / (bm / 16)) ceil(W / 16) ceil(Npad / bn) >= 256 picks the tile
H2D = [
    C("h2-128x16", 9, 3, 1, 90, 120, 16, 12, 9128016, "h2d", bias=True, out_pad=4, stats=1),       # 3 * 12 * 8 = 288; ragged in H, W, N
    C("h2-64x16", 9, 2, 1, 20, 19, 20, 2, 9064016, "h2d", in_pad=3, in_off=2, out_pad=1, stats=2),  # element-wise staging, scalar stores
    C("h2-256x32", 9, 3, 1, 90, 250, 16, 20, 9256032, "h2d", bias=True, out_pad=4),   # 3 * 6 * 16 = 288 tiles of 256 pixels
    C("h2-128x32", 9, 2, 1, 90, 180, 24, 32, 9128032, "h2d", in_pad=8, in_off=8, stats=2),   # 2 * 12 * 12 = 288 tiles of 128 pixels (and only 144 of 256)
    C("h2-64x32", 9, 1, 1, 11, 21, 48, 19, 9064032, "h2d", bias=True, out_pad=2),
    C("h2-64x32w", 9, 1, 1, 45, 250, 16, 64, 9064032, "h2d", bias=True),                            # Npad = 64: 192 of 64x64, 384 of 64x32
    C("h2-128x64", 9, 3, 1, 90, 120, 32, 64, 9128064, "h2d", bias=True, stats=1),   # 3 * 12 * 8 = 288 tiles of 128 pixels
    C("h2-64x64", 9, 2, 1, 45, 180, 16, 50, 9064064, "h2d", out_pad=2),                             # 2 * 12 * 12 = 288; N % 4 != 0, ld 52
    C("h2-32x32", 9, 1, 1, 3, 7, 20, 48, 9032032, "h2d", bias=True, in_pad=4, in_off=1, stats=1),  # a plane smaller than a tile
]
# ---- hconv_kernel<9, .., DEPTH 3>: rectangular (W % 16 == 0) and flat (W % 16 != 0, W + 2 <= 64) tiles, arco_conv3d_fl_set(0) ---------
H3D = [
    C("v128x16", 27, 1, 3, 20, 16, 16, 4, 9128016, "h3d", fl=0, bias=True, out_pad=4, stats=1),
    C("v256x32", 27, 1, 8, 64, 128, 16, 20, 9256032, "h3d", fl=0),   # 8 * 4 * 8 = 256 tiles of 256 voxels
    C("v128x32", 27, 1, 4, 64, 128, 16, 32, 9128032, "h3d", fl=0, bias=True),   # 4 * 8 * 8 = 256 tiles of 128 voxels (128 of 256)
    C("v64x32", 27, 1, 3, 6, 16, 24, 19, 9064032, "h3d", fl=0, bias=True, in_pad=8, in_off=8, out_pad=2),
    C("v128x64", 27, 1, 4, 64, 128, 16, 64, 9128064, "h3d", fl=0),   # 4 * 8 * 8 = 256 tiles of 128 voxels
    C("v64x64", 27, 1, 2, 64, 128, 16, 64, 9064064, "h3d", fl=0, bias=True),   # 2 * 16 * 8 = 256 tiles of 64 voxels (128 of 128)
    C("v64x32w", 27, 1, 1, 64, 128, 16, 64, 9064032, "h3d", fl=0, stats=1),                          # one plane; 128 of 64x64, 256 of 64x32
    C("v32x32", 27, 2, 2, 5, 16, 24, 48, 9032032, "h3d", fl=0, bias=True, stats=2),
    C("f128x16", 27, 1, 3, 9, 14, 16, 12, 9628016, "h3d", fl=0, bias=True, out_pad=4),
    C("f128x32", 27, 1, 32, 32, 30, 16, 32, 9628032, "h3d", fl=0),   # 32 * 8 = 256 flat tiles of 128 positions
    C("f64x32", 27, 1, 3, 7, 7, 32, 19, 9564032, "h3d", fl=0, bias=True, out_pad=5),
    C("f128x64", 27, 1, 32, 32, 30, 16, 64, 9628064, "h3d", fl=0, bias=True),   # 32 * 8 = 256 flat tiles of 128 positions
    C("f64x64", 27, 1, 16, 32, 30, 16, 64, 9564064, "h3d", fl=0),   # 16 * 16 = 256 flat tiles of 64 positions (128 of 128)
    C("f64x32w", 27, 1, 8, 32, 30, 16, 64, 9564032, "h3d", fl=0, bias=True),                         # 128 of 64x64, 256 of 64x32
    C("f32x32", 27, 1, 2, 5, 6, 24, 48, 9532032, "h3d", fl=0, in_pad=8, in_off=8, stats=1),
    C("f64x32-plane", 27, 2, 1, 7, 7, 32, 19, 9564032, "h3d", fl=0, out_pad=1, stats=2),            # volumes of ONE plane
]
# ---- hconv_kernel<1, ..>: 256x16 (Npad <= 16), 128x32 (Npad <= 32), 32x64 (fewer than 192 64x64 tiles, no stat groups), 64x64, 128x128 ---
H1X1 = [
    C("g256x16", 1, 1, 1, 3, 101, 20, 4, 1256016, "h1x1", bias=True, out_pad=4, stats=1),
    C("g256x16-n2", 1, 2, 1, 7, 23, 19, 2, 1256016, "h1x1", in_pad=5, in_off=3, out_pad=1),
    C("g128x32", 1, 2, 1, 9, 17, 48, 19, 1128032, "h1x1", in_pad=8, in_off=8, stats=2),            # M / 2 = 153: no multiple of 128 (m_lim)
    C("g32x64", 1, 1, 1, 5, 41, 48, 80, 1032064, "h1x1", bias=True),
    C("g64x64", 1, 1, 1, 61, 100, 48, 100, 1064064, "h1x1", bias=True, out_pad=4, stats=1),
    C("g64x64-groups", 1, 2, 1, 5, 41, 48, 80, 1064064, "h1x1", stats=2, launch_only=True, grouped=True),        # 8 tiles: 64x64 only because of the groups
    C("g128x128", 1, 1, 1, 200, 164, 24, 128, 1128128, "h1x1", bias=True),                          # M Npad = 4198400 > 4096 * 1024
]
# ---- hconv_rw_kernel<1,1,8>: K = N = 16, H % 8 == 0, W % 16 == 0 ------------------------------------------------------------------------
RW = [
    C("rw-plane", 27, 2, 1, 8, 16, 16, 16, 9408016, "rw", bias=True, stats=2),
    C("rw-odd", 27, 2, 5, 16, 32, 16, 16, 9408016, "rw", in_pad=8, in_off=8, out_pad=4, stats=1),  # S = 2: the last unit of a column holds one plane
    C("rw-rounds", 27, 2, 33, 64, 64, 16, 16, 9408016, "rw", bias=True),   # 64 tile columns x 17 units of S = 2 planes = 1088 units on 1024 slots: a ragged second round
]
# ---- hconv_fc_kernel<A_T, C_T> as the cost model picks it (arco_conv3d_fl_set(1), nothing forced): ids 9.26e6 + A_T 1e3 + 16 C_T ---------
FC = [
    C("fc-7-32-32", 27, 2, 2, 7, 7, 32, 32, 9261032, "fc", fl=1, bias=True, stats=2),                # a plane smaller than one tile
    C("fc-12-64-64", 27, 2, 4, 12, 12, 64, 64, 9261032, "fc", fl=1, in_pad=8, in_off=8, out_pad=4),
    C("fc-7-64-128", 27, 1, 4, 7, 7, 64, 128, 9261032, "fc", fl=1, bias=True, stats=1),
    C("fc-24-128-64", 27, 1, 8, 24, 24, 128, 64, 9262032, "fc", fl=1),   # K = 128 at the 24-wide plane
    C("fc-45-32-64", 27, 1, 4, 45, 45, 32, 64, 9263032, "fc", fl=1, bias=True, stats=1),
    C("fc-7-64-64-w", 27, 2, 32, 7, 7, 64, 64, 9261064, "fc", fl=1, stats=2),                        # the 64-wide tile
    C("fc-7-32-32-rounds", 27, 2, 150, 7, 7, 32, 32, 9261032, "fc", fl=1, bias=True),   # 300 tiles on 256 workgroups: a ragged second round
]
# ---- the streaming 1x1 kernels (launch-only: ids 1.8e6 + K 1e3 + 4 and 1900000), M = 257 * 257 = 66049 >= 65536 ---------------------------
STREAM = [
    C("nout-k8-n1", 1, 1, 1, 257, 257, 8, 1, 1808004, "nout", launch_only=True, bias=True),
    C("nout-k8-n4", 1, 1, 1, 257, 257, 8, 4, 1808004, "nout", launch_only=True, out_pad=4),
    C("nout-k16-n2", 1, 1, 1, 257, 257, 16, 2, 1816004, "nout", launch_only=True, in_pad=8, in_off=8, out_pad=1, bias=True),
    C("nout-k16-n3", 1, 1, 1, 257, 257, 16, 3, 1816004, "nout", launch_only=True),
    C("nout-k32-n4", 1, 1, 1, 257, 257, 32, 4, 1832004, "nout", launch_only=True, bias=True),
    C("nout-k32-n3", 1, 1, 1, 257, 257, 32, 3, 1832004, "nout", launch_only=True, out_pad=2),
    C("nin-k1-n8", 1, 1, 1, 257, 257, 1, 8, 1900000, "nin", launch_only=True, bias=True),
    C("nin-k2-n16", 1, 1, 1, 257, 257, 2, 16, 1900000, "nin", launch_only=True, in_pad=2, in_off=1, out_pad=8),
    C("nin-k3-n32", 1, 1, 1, 257, 257, 3, 32, 1900000, "nin", launch_only=True, bias=True),
    C("nin-k4-n8", 1, 1, 1, 257, 257, 4, 8, 1900000, "nin", launch_only=True),
]
# ... and one shape per kernel that misses exactly ONE condition and must therefore run on hconv_kernel<1,256,16> / <1,128,32>
NEAR = [
    C("nout-miss-m", 1, 1, 1, 255, 257, 16, 2, 1256016, "h1x1", bias=True),                          # M = 65535
    C("nout-miss-ld", 1, 1, 1, 257, 257, 8, 3, 1256016, "h1x1", in_pad=4),                            # ld_in = 12: no multiple of 8
    C("nin-miss-shift", 1, 1, 1, 257, 257, 2, 16, 1256016, "h1x1", bias=True, out_shift=4),           # the output 8 bytes off a 16-byte boundary
    C("nin-miss-m", 1, 1, 1, 255, 257, 4, 32, 1128032, "h1x1"),                                       # M = 65535
]
# ---- the one-channel volume in mma 4: conv3d_image_kernel<3> with the f16 epilogue (fp32 volume, fp32 pack) ------------------------------
IMAGE = [
    C("image3-plane", 27, 1, 1, 11, 13, 1, 16, 27701016, "image", bias=True, stats=1),
    C("image3", 27, 2, 5, 20, 19, 1, 12, 27701016, "image", out_pad=4, stats=2),
]

CASES = H2D + H3D + H1X1 + RW + FC + STREAM + NEAR + IMAGE
NAMES = [c["name"] for c in CASES]
assert len(set(NAMES)) == len(NAMES)
# the data gradient runs the same kernels on a mode 1 | 4 pack: one case per kernel template (dY has N channels, dX K).  nout-dgrad is
# the gradient of the V-Net's out_conv written as nin (2 -> 16 forward is 16 -> 2 backward), nin-dgrad the other way round
DGRAD = [
    C("dgrad-h2", 9, 1, 1, 11, 21, 19, 48, 9032032, "h2d", in_pad=1),
    C("dgrad-h3-rect", 27, 1, 3, 6, 16, 24, 19, 9064032, "h3d", fl=0),
    C("dgrad-h3-flat", 27, 1, 3, 7, 7, 32, 19, 9564032, "h3d", fl=0),
    C("dgrad-h1x1", 1, 1, 1, 5, 41, 80, 48, 1032064, "h1x1"),
    C("dgrad-rw", 27, 1, 3, 8, 16, 16, 16, 9408016, "rw"),
    C("dgrad-fc", 27, 1, 4, 12, 12, 64, 32, 9261032, "fc", fl=1),
    C("dgrad-nin-of-out-conv", 1, 1, 1, 257, 257, 2, 16, 1900000, "nin", launch_only=True),
    C("dgrad-nout-of-in-conv", 1, 1, 1, 257, 257, 16, 2, 1816004, "nout", launch_only=True),
]
# every route id this family can take (the issue's list); the CPU file asserts that each appears in a case
ROUTES = ([(9, 9000000 + t) for t in (128016, 64016, 256032, 128032, 64032, 128064, 64064, 32032)]
          + [(27, 9000000 + t) for t in (128016, 256032, 128032, 64032, 128064, 64064, 32032)]
          + [(27, 9500000 + t) for t in (128016, 128032, 64032, 128064, 64064, 32032)]
          + [(1, 1000000 + t) for t in (256016, 128032, 32064, 64064, 128128)]
          + [(27, 9408016), (1, 1808004), (1, 1816004), (1, 1832004), (1, 1900000), (27, 27701016)])


def by_name(name):
    return CASES[NAMES.index(name)]


def n_acc(c):
    """the count of accumulations behind one output (module docstring)"""
    return {"nout": c["k"] + 1, "nin": c["k"] + 1, "image": 2 * c["taps"] + 1}.get(c["fam"], c["taps"] * c["k"] + 1)


def spatial_tile(c):
    """hconv_dispatch2 / hconv_dispatch3 restated: the id of the largest tile that still gives WANT workgroups"""
    npad, nb, flat = ceil_to(c["n"], 16), c["nv"] * c["d3"], c["taps"] == 27 and c["w"] % 16 != 0 and c["w"] + 2 <= 64

    def blocks(bm, bn):
        per = -(-(c["h"] * (c["w"] + 2)) // bm) if flat else -(-c["h"] // (bm // 16)) * -(-c["w"] // 16)
        return nb * per * -(-npad // bn)
    if npad <= 16:
        order = [(128, 16)] if c["taps"] == 27 else [(128, 16), (64, 16)]
    elif npad <= 32:
        order = ([] if flat else [(256, 32)]) + [(128, 32), (64, 32)]
    else:
        order = [(128, 64), (64, 64), (64, 32), (32, 32)]
    bm, bn = next((t for t in order[:-1] if blocks(*t) >= WANT), order[-1])
    return 9000000 + (500000 if flat else 0) + bm * 1000 + bn


def rw_units(c, cus=256):
    """launch_hconv_rw restated: (S, segments per column, units, slots) - LDS of <1,1,8>: 27 * 16 + 1 weight rows and three 180-row plane
    tiles of 8 dwords, 2 * 4 * 16 floats of reduction space; per_cu = min(4, 160 KB / that); slots = CUs * per_cu"""
    lds = ((27 * 16 + 1) * 8 + 3 * 180 * 8 + 2 * 4 * 16) * 4
    slots = cus * max(1, min(4, 160 * 1024 // lds))
    cols = c["nv"] * (c["h"] // 8) * (c["w"] // 16)
    S = 8
    while S > 2 and cols * -(-c["d3"] // S) < 3 * slots:
        S >>= 1
    S = min(S, c["d3"])
    nseg = -(-c["d3"] // S)
    return S, nseg, cols * nseg, slots


# ======================================================================================================================================
# inputs
# ======================================================================================================================================
QX = 2.0 ** -14
QWF = {"exact": 2.0 ** 2, "sub": 2.0 ** -14, "tie": 2.0 ** -4, "big": 2.0 ** 4}


def flavour(n, N):
    if N == 1:
        return "sub"
    return "exact" if n % 2 == 0 else ("sub", "tie", "big")[(n // 2) % 3]


def _odd11(shape, g, lo=0):
    return (2 * _ints(shape, g, lo, 1023) + 1) * (2 * _ints(shape, g, 0, 1) - 1)


def _patterns(shape, g, max_exp):
    """random finite f16 bit patterns with an exponent field of at most max_exp (0: subnormals), as float32; no negative zero"""
    e, m, s = _ints(shape, g, 0, max_exp), _ints(shape, g, 0, 1023), _ints(shape, g, 0, 1)
    s = torch.where((e == 0) & (m == 0), torch.zeros_like(s), s)
    flat_e, flat_m = e.view(-1), m.view(-1)
    flat_e[0::7] = 0
    flat_m[0::7] = flat_m[0::7].clamp(min=1)                                                          # subnormals planted
    bits = (s << 15) | (e << 10) | m
    return (bits - (bits >= 32768).long() * 65536).to(torch.int16).view(torch.float16).float()


def _normal(v):
    """rounds to f16 and raises non-zero magnitudes below the normal range to 2^-14 (the wide kind stays inside the normal range)"""
    v = v.half().float()
    small = (v != 0) & (v.abs() < SUBN)
    return torch.where(small, torch.sign(v) * SUBN, v)


def _fixed(c, g):
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    kb = K - 1 if K >= 2 else (0 if T == 1 else None)          # (K = 1: the 1 -> N stream's only channel; the one-channel volume has none)
    xi = _ints((M, K), g, -3, 3)
    if kb is not None:
        xi[:, kb] = _odd11((M,), g)
    wi, bi, qw = torch.zeros((N, K, T), dtype=torch.int64), torch.zeros(N, dtype=torch.int64), torch.zeros(N, dtype=torch.float64)
    free = torch.ones((K, T), dtype=torch.bool)
    if kb is not None and K >= 2:
        free[kb] = False
    slots = torch.nonzero(free.view(-1)).view(-1)
    for n in range(N):
        f = flavour(n, N)
        qw[n] = QWF[f] * (2.0 ** -4 if f == "exact" and n % 4 == 2 else 1.0)
        if f == "exact":
            pick = slots[torch.randperm(slots.numel(), generator=g)[:600]]
            wi[n].view(-1)[pick] = 2 * _ints((pick.numel(),), g, 0, 1) - 1
            bi[n] = int(_ints((1,), g, -200, 200)) if K >= 2 or kb is None else 0                 # (K = 1 stream: |x| alone reaches 2047)
            continue
        lo = 1 if f == "sub" else 3
        wi[n] = _ints((K, T), g, -lo, lo)
        if kb is not None:
            wi[n, kb] = 0
            wi[n, kb, T // 2] = 1 if f == "sub" else 3
            if f == "big":
                wi[n, kb, T // 2] = int(_odd11((1,), g, 512))
                if T > 1:
                    wi[n, kb, 0] = int(_odd11((1,), g, 512))
        elif f != "sub":
            wi[n, 0] = _odd11((T,), g)
        bi[n] = int(_ints((1,), g, -1000, 1000)) if f != "big" else int(_ints((1,), g, -2 ** 18, 2 ** 18))
        if K == 1 and kb is not None:
            bi[n] |= 1                                                                                 # (ref / q = odd x + odd bias: ties need an even sum)
    x = (xi.double() * QX).float()
    w = (wi.double() * qw.view(N, 1, 1)).float()
    bias = (bi.double() * qw * QX).float() if c["bias"] else None
    return x, w, bias, qw * QX


def _stats(c, g):
    """the fixed kind shrunk: about 12 non-zero products per output, weights up to +-R: ref / q of a few tens, q = 2^-28 = SQ / 16"""
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    dens = min(1.0, math.sqrt(12.0 / (T * K)))
    R = max(4, math.ceil(12 / math.sqrt(T * K)))
    xi = _ints((M, K), g, -1, 1) * (torch.rand((M, K), generator=g) < dens * 1.5)
    wi = _ints((N, K, T), g, -R, R) * (torch.rand((N, K, T), generator=g) < dens)
    bias = (_ints((N,), g, -3, 3).double() * QX * QX).float() if c["bias"] else None
    return (xi.double() * QX).float(), (wi.double() * QX).float(), bias, torch.full((N,), QX * QX, dtype=torch.float64)


def finish(c, d):
    """adds the float64 reference and S to the inputs x, w, bias (fp32 tensors holding f16-representable values, or None)"""
    x, w = d["x"].double(), d["w"].double()
    ref = conv64(x, w, c)
    d["sxw"] = conv64(x.abs(), w.abs(), c) if d["kind"] not in ("impulse", "select") else ref.abs()      # (one product per output)
    s = d["sxw"].clone()
    if d["bias"] is not None:
        ref = ref + d["bias"].double()
        s = s + d["bias"].double().abs()
    d["ref"], d["S"] = ref, s
    return d


@functools.lru_cache(maxsize=4)
def _data(name, kind, p, dgrad):
    c = (DGRAD[[d["name"] for d in DGRAD].index(name)] if dgrad else by_name(name))
    g = gen(sum(map(ord, name)), (ALL + ("stats",)).index(kind), p, 4)
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    bias = q = None
    if kind == "fixed":
        x, w, bias, q = _fixed(c, g)
    elif kind == "stats":
        x, w, bias, q = _stats(c, g)
    elif kind == "impulse":
        x = torch.zeros((M, K))
        for i, m in enumerate(impulse_positions(c)):
            x[m, i % K] = 1.0
        w = _patterns((N, K, T), g, 30)
        w.view(-1)[3::11] = MAXH * (1 - 2 * (torch.arange(w.view(-1)[3::11].numel()) % 2)).float()    # +-65504 planted
    elif kind == "select":
        x = _patterns((M, K), g, 27)
        x[torch.rand((M, K), generator=g) < 0.2] = 0.0
        w = torch.zeros((N, K, T))
        for n in range(N):
            w[n, (7 * n + 3 + p) % K, (n + p * N) % T] = (-1.0) ** n * 2.0 ** ((n + p) % 4)
    else:
        if c["fam"] == "image":                                                                       # the fp32 volume and the fp32 pack
            x = _wide_values((M, K), g, 2, 0.2)
            w = (_wide_values((N, K, T), g, 2, 0.0).double() / math.sqrt(K * T)).float()
        else:
            x = _normal(_wide_values((M, K), g, 2, 0.2))
            w = _normal((_wide_values((N, K, T), g, 2, 0.0).double() / math.sqrt(K * T)).float())
        if c["bias"]:
            bias = _wide_values((N,), g, 1, 0.0)
    return finish(c, dict(x=x, w=w, bias=bias, kind=kind, p=p, q=q))


def data(c, kind, p=0, dgrad=False):
    """the inputs, the float64 reference and S of one case and kind (pass p of the select kind); computed once, never modified"""
    return _data(c["name"], kind, p, dgrad)


def f16_ok(t):
    """every value representable in f16"""
    return bool((t.half().float() == t).all()) and bool(torch.isfinite(t).all())


# ======================================================================================================================================
# comparisons
# ======================================================================================================================================
def expected_h(ref):
    """the float64 reference rounded ONCE to f16, to nearest even: the reference is exactly representable in fp32 (asserted), so the
    fp32 -> f16 conversion of torch is that single rounding"""
    assert representable(ref), "the reference is not exactly representable in fp32"
    assert float(ref.abs().max()) <= MAXH
    return ref.float().half()


def equal_h(got, ref):
    """the exact kinds: the kernel's f16 output equals the once-rounded float64 reference, torch.equal on the f16 values"""
    got = got.detach().cpu()
    return got.dtype == torch.float16 and got.shape == ref.shape and torch.equal(got, expected_h(ref))


def tol_wide(c, d):
    t32 = gamma_n(n_acc(c)) * d["S"]
    return t32 + 2.0 ** -11 * (d["ref"].abs() + t32) + 2.0 ** -25


def held(name, got, c, d):
    """the wide kind: worst err / derived bound per element, printed; must be <= 1"""
    r = worst(got.float(), d["ref"], tol_wide(c, d))
    print(f"{name}: worst err / bound {r:.4f}")
    return r


def ties(ref):
    """the outputs whose float64 reference lies exactly half way between two neighbouring f16 values"""
    a = ref.abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=SUBN)))                                             # binade; the subnormals share 2^-14's
    ulp = 2.0 ** (e - 10)
    r = a / ulp
    return (r - torch.floor(r)) == 0.5


def trunc_h(ref):
    """planted error: the fp32 value cut to f16 instead of rounded (towards zero)"""
    h = ref.float().half()
    over = h.double().abs() > ref.abs()
    step = torch.where(over, torch.ones_like(h.view(torch.int16)), torch.zeros_like(h.view(torch.int16)))
    return (h.view(torch.int16) - step).view(torch.float16)                                           # one ulp towards zero (sign-magnitude)


def bf16_then_h(ref):
    """planted error: rounded twice, fp32 -> 16-bit bf16 -> f16"""
    return ref.float().bfloat16().float().half()


def twice_h(ref, bits=13):
    """planted error: rounded twice, fp32 -> `bits` significant bits -> f16 (a tie made by the first rounding goes the wrong way)"""
    a = ref.double()
    e = torch.floor(torch.log2(torch.clamp(a.abs(), min=2.0 ** -40)))
    ulp = 2.0 ** (e - (bits - 1))
    return (torch.round(a / ulp) * ulp).float().half()                                                 # (torch.round: ties to even)


def flush_h(ref):
    """planted error: subnormal outputs flushed to zero"""
    h = ref.float().half()
    return torch.where(h.float().abs() < SUBN, torch.zeros_like(h), h)


# ---- BatchNorm partial sums of the epilogues ------------------------------------------------------------------------------------------
def stats_exact(c, ssum, ssq, nmb, groups, y):
    """the stats kind: y the ROUNDED f16 outputs [M, N]; every slab an integer number of SQ (SQ^2), every group's slab range equal to
    its own volumes' totals of y and y^2, with =="""
    if nmb % groups or ssum.shape != (c["n"], nmb) or ssq.shape != (c["n"], nmb):
        return False
    q1, q2 = ssum.double() / SQ, ssq.double() / (SQ * SQ)
    if not (bool((q1 == q1.round()).all()) and bool((q2 == q2.round()).all())):
        return False
    t1, t2 = stat_totals(c, y.double(), groups)
    return torch.equal(slab_sums(ssum, nmb, groups), t1) and torch.equal(slab_sums(ssq, nmb, groups), t2)


def stats_tol(c, d, groups):
    """wide kind: |sum over slabs - sum ref| <= sum tol_y + gamma(Mg + 1) sum(|ref| + tol_y); the squares with |y^2 - ref^2| <=
    tol (2 |ref| + tol) and one more rounding (conv_kernel_refs.stats_tol with this file's per-element bound)"""
    t = tol_wide(c, d)
    a = d["ref"].abs()
    gm = gamma(c["M"] // groups + 1)
    g = lambda v: v.view(groups, c["M"] // groups, -1).sum(1)
    e2 = t * (2 * a + t)
    return g(t) + gm * g(a + t), g(e2) + gm * g(a * a + e2)


# ======================================================================================================================================
# the fp32 emulation of the wide kind: exact products, fp32 accumulation in one fixed order, one rounding to f16
# ======================================================================================================================================
def emulate(c, d):
    f32, f64 = np.float32, np.float64
    cols_ = im2col(d["x"], c).numpy().astype(f64)                              # [M, T, K]
    w = d["w"].permute(0, 2, 1).contiguous().numpy().astype(f64)               # [N, T, K]
    M, T, K = cols_.shape
    N = w.shape[0]
    b = None if d["bias"] is None else d["bias"].numpy()[None, :]
    fam = c["fam"]
    if fam == "nout":                                                          # per 8-k lane: x0 w0, seven fmaf; the butterfly; + bias
        Q = K // 8
        parts = []
        for q in range(Q):
            p = (cols_[:, 0, 8 * q][:, None] * w[:, 0, 8 * q][None, :]).astype(f32)
            for e in range(1, 8):
                p = (cols_[:, 0, 8 * q + e][:, None] * w[:, 0, 8 * q + e][None, :] + p.astype(f64)).astype(f32)
            parts.append(p)
        off = 1
        while off < Q:
            parts = [(parts[q] + parts[q ^ off]).astype(f32) for q in range(Q)]
            off <<= 1
        acc = parts[0] if b is None else (parts[0] + b).astype(f32)
        return torch.from_numpy(acc).half()
    acc = np.zeros((M, N), dtype=f32)
    if fam in ("nin", "image") and b is not None:
        acc = acc + b
    for t in range(T):
        for k in range(K):
            acc = (cols_[:, t, k][:, None] * w[:, t, k][None, :] + acc.astype(f64)).astype(f32)
    if fam not in ("nin", "image") and b is not None:
        acc = (acc + b).astype(f32)
    return torch.from_numpy(acc).half()
