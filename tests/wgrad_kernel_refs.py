"""Cases, inputs, float64 references, per-element bounds and comparison helpers shared by tests/test_wgrad_kernels_gpu.py (every
weight-gradient route of csrc/wgrad.hip and conv_h.hip, the slab reductions, arco_colsum(_h) and arco_transpose2d, one route
per test, called directly) and tests/test_wgrad_kernels_cpu.py (the routes asserted through arco_wgrad_config, the slab sweep, the
input conditions, an fp32 emulation of the wide kind inside the same bounds, planted errors, the host-side rejections).  Plain CPU
torch / numpy only; nothing here touches a GPU.

A CASE names one route: the id (include/arco_hip.h, T*1e6 + F*1e5 + V*1e4 + COB*100 + CIB) that wgrad_plan must choose for its shape.
dZ is rows [M, Cout], the input rows [M, Cin] (channels last), M = nv * d3 * h * w; dW has the torch layout [Cout, Cin, taps]:
    dW[co, ci, tap] = sum_m dZ[m, co] * im2col(x)[m, tap, ci]        (zero padding 1; planes of one volume only)

Kinds of input per case:
  fixed     dZ in units of 2^-3, x of 2^-5, small integers; sum |dz||x| / 2^-8 < 2^24 per element (asserted): every product and every
            partial sum is exact in fp32 whatever the slab order, so dW must equal float64 bit for bit - also on the bf16-operand and
            f16 routes (integers up to 3: two significant bits).  On the
            split-bf16 routes a few pixels of a few channels hold 9-bit integers (257 .. 287, odd) on both operands: planes 0 and 1.
  impulse   dZ a unit impulse in its own channel at chosen pixels (first, last = last persistent round, corners, the ragged tile, the
            first and last plane of every volume) against full 24-bit x: dW[co][:, tap] is one shifted input row or zero, bit for bit
            (plane 2 of the split).  impulse_x exchanges the roles.  Not on the bf16-operand routes.
  wide      six decades of magnitudes (f16 operands: four, inside the normal range), 20 % exact zeros; |err| <= tol per element,
            tol = gamma(n) S + u |ref| (+ DROP S on the split routes, + BF16 S with bf16 operands), S = sum |dz||x|.

n, the longest chain of roundings behind one dW element, = r P tpw + cross + red (+ 1 with accumulate):
  r      roundings per product: 2 on the fp32 matrix cores (the product, its accumulation: the order inside an instruction is the
         hardware's), 1 for the fused multiply-add of himage_wgrad_kernel, 1 on the f16 and bf16-operand routes (a product of two
         11-bit / 8-bit values is exact in fp32), 6 on the split routes (six kept products per pair, each exact: 16 bits)
  P      pixels of one tile that feed ONE accumulator: wgrad_kernel 32 (each wave reduces 32 of 128), wgrad_q_kernel<64> 64 (a wave
         owns its quadrant for the whole tile), wgrad_halo2_kernel / wgrad_split_kernel 128 / WPS with WPS = 4 / (COB CIB / 256)
         pixel-split partner waves, wgrad_image3d_kernel 64 (256-voxel tiles over four waves), hwgrad_kernel 32 (K step = wave),
         himage_wgrad_kernel 256 (every thread walks the whole tile)
  tpw    tiles per workgroup = ceil(n_tiles / slabs) (the kernels stride their tiles by gridDim.x)
  cross  the partner waves summed once per launch: 2 ((a + b) + (c + d)), WPS - 1 in the halo / split kernels, 3 image, 0 q / himage
  red    the slab sum: ceil(slabs / (2 GR)) per accumulator, s0 + s1, the tree (a + b) + (c + d) and GR / 4 chained groups:
         ceil(slabs / (2 GR)) + 3 + GR / 4 with GR = 8 (<64,8>) or 32 (<16,32> and wgrad_reduce4_kernel, same order)
  DROP   wgrad_split_kernel keeps (z2,x0) (z0,x2) (z1,x1) (z1,x0) (z0,x1) (z0,x0) and drops (1,2) (2,1) (2,2): DROP of
         conv_kernel_refs.py relative to |dz||x|
  BF16   wgrad_halo2_kernel<.., 2> rounds both operands with to_bf16x4 (round to nearest even, 8 significant bits: 2^-8 each): (2^-7 + 2^-16) |dz||x|
  pro    arco_conv3d_wgrad_pro forms the activation in fp32: sub, mul, mul, add, slope, keep scale: gamma(6) (|z - mean| |istd gamma|
         + |beta|) scale per element of the activation, times |dz| summed
Long chains: gamma(n) grows with n, independent roundings add up as sqrt(n).  Where it is smaller, the bound uses Higham and Mary's
probabilistic constant (SIAM J. Sci. Comput. 41, 2019, theorem 2.4: roundings as mean-independent random variables of size <= u) instead:
  gamma~(n) = LAMBDA sqrt(n) u, which fails with probability <= 2 n exp(-LAMBDA^2 (1 - u)^2 / 2) per element; LAMBDA = 9 puts that below
  1e-12 for n <= 2^16, far below one in the ~10^6 elements all cases compare.  It is the smaller of the two from n = 82 on (wgrad_q_kernel,
  n = 1167: 307 u instead of 1167 u); it is a statement about roundings, not a measured figure.
Kinds per case: the consumer-side activation runs fixed and wide only (an impulse in z is no impulse in act(z), and the mask moves it); the
`ws-*`, `red-*` and threshold cases repeat routes whose impulse kinds run in their own cases and keep fixed and wide.
arco_colsum: a block sums its rows in fp32 - ceil(rows / rstep) per thread, then rstep partials - and the blocks are summed in float64,
rounded once: n = ceil(rpb / rstep) + rstep (+ 1 accumulate), rstep = 256 / (C / 4), 256 / C or 1 by branch."""
import functools
import math

import numpy as np
import torch

from conv_kernel_refs import DROP, ERR_ARG, _ints, _wide_values, bf16_rne, im2col, split_act
from loss_kernel_refs import U, gamma, gen, worst

BF16 = 2.0 ** -7 + 2.0 ** -16
QZ, QX = 2.0 ** -3, 2.0 ** -5
QUANT = QZ * QX
F_GEMM, F_Q, F_HALO, F_SPLIT, F_IMAGE, F_HGRAD, F_HIMAGE = range(7)
ALL = ("fixed", "impulse", "impulse_x", "wide")
TWO = ("fixed", "wide")


def rid(t, f, v, cob, cib):
    return t * 1000000 + f * 100000 + v * 10000 + cob * 100 + cib


def C(name, taps, mma, nv, d3, h, w, cin, cout, route, **opt):
    c = dict(name=name, taps=taps, mma=mma, nv=nv, d3=d3, h=h, w=w, k=cin, n=cout, route=route, dz_pad=0, dz_off=0, in_pad=0, in_off=0,
             entry=0, pro=0, drop=0, kinds=ALL, acc=0, table=False, red=0)
    assert set(opt) <= set(c), opt
    c.update(opt)
    c["M"] = nv * d3 * h * w
    c["ld_dz"], c["ld_in"] = cout + c["dz_pad"], cin + c["in_pad"]
    c["fam"] = (route // 100000) % 10
    c["var"] = (route // 10000) % 10
    c["cob"], c["cib"] = (route // 100) % 100, route % 100
    c["zh"] = mma == 4                                 # dZ is f16
    c["xh"] = mma == 4 and c["fam"] == F_HGRAD         # x is f16 (the one-channel volume and the fp32 image stay fp32)
    c["bf16"] = c["fam"] == F_HALO and c["var"] >= 2
    if c["bf16"]:
        c["kinds"] = tuple(k for k in c["kinds"] if not k.startswith("impulse"))
    return c


# ---- 1x1: wgrad_kernel<COB,CIB>, all nine tiles; M = 303: three tiles of 128, the last ragged ---------------------------------------
CASES = []
for i, (cob, cib, co, ci) in enumerate([(16, 16, 3, 3), (16, 32, 16, 20), (16, 64, 3, 64), (32, 16, 20, 16), (32, 32, 20, 20),
                                         (32, 64, 32, 68), (64, 16, 64, 3), (64, 32, 68, 20), (64, 64, 68, 68)]):
    CASES.append(C(f"g1-{cob}x{cib}", 1, 0, 1, 1, 3, 101, ci, co, rid(1, F_GEMM, 0, cob, cib), dz_pad=(4 if i % 2 else 0), dz_off=(4 if i % 2 else 0),
                   in_pad=(0 if i % 3 else 4), acc=i % 2))
CASES += [
    # 301 tiles on 128 workgroups (512 / (2 x 2 channel tiles)): three rounds, the last one ragged (45 tiles)
    C("g1-64x64-rounds", 1, 0, 1, 1, 5, 7681, 68, 68, rid(1, F_GEMM, 0, 64, 64), kinds=ALL),
    C("g1-m3-scalar", 1, 3, 1, 1, 3, 101, 19, 5, rid(1, F_GEMM, 0, 16, 32), dz_pad=1, in_pad=2, acc=1),
    # wgrad_q_kernel<64>: Cout, Cin >= 192 and M >= 32768; M = 32768 + 64 * 3 + 37
    C("q64", 1, 0, 1, 1, 1, 32997, 192, 192, rid(1, F_Q, 0, 0, 64), kinds=ALL),
    C("q64-below-m", 1, 0, 1, 1, 1, 32767, 192, 192, rid(1, F_GEMM, 0, 64, 64), kinds=TWO),
    C("q64-below-cin", 1, 0, 1, 1, 1, 32997, 188, 192, rid(1, F_GEMM, 0, 64, 64), kinds=TWO),
]
# ---- 3x3 / 3x3x3 wgrad_halo2_kernel ----------------------------------------------------------------------------------------------
T4 = [(16, 16, 12, 16), (16, 32, 16, 20), (32, 16, 20, 8), (32, 32, 19, 33)]      # (COB, CIB, Cout, Cin)
for i, ((cob, cib, co, ci), (h, w)) in enumerate(zip(T4, [(9, 16), (5, 67), (8, 32), (11, 80)])):       # rectangular: W % 16 == 0 or W + 2 > 64
    CASES.append(C(f"halo-rect-{cob}x{cib}", 9, 0, 2, 1, h, w, ci, co, rid(9, F_HALO, 0, cob, cib), dz_pad=4 * (i % 2), in_pad=4 * (i // 2), acc=i % 2))
for i, ((cob, cib, co, ci), w) in enumerate(zip(T4, [5, 20, 37, 62])):                                   # flat
    CASES.append(C(f"halo-flat-{cob}x{cib}", 9, 0, 3, 1, 7, w, ci, co, rid(9, F_HALO, 1, cob, cib), dz_off=4 * (i % 2), dz_pad=4 * (i % 2), acc=(i + 1) % 2))
for i, (cob, cib, co, ci) in enumerate(T4):                                                             # bf16 operands: taps 27, mma 1 and 2
    CASES.append(C(f"halo-bf16-rect-{cob}x{cib}", 27, 1 + i % 2, 2, 3, 6, 16, ci, co, rid(9, F_HALO, 2, cob, cib), in_pad=4 * (i % 2)))
    CASES.append(C(f"halo-bf16-flat-{cob}x{cib}", 27, 2 - i % 2, 2, 3, 6, [5, 20, 37, 62][i], ci, co, rid(9, F_HALO, 3, cob, cib), acc=i % 2))
CASES += [
    # mma 3 falls back to the fp32 halo kernel when ld_dz or a channel count is no multiple of 4
    C("halo-m3-ldz-odd", 9, 3, 2, 1, 9, 16, 16, 16, rid(9, F_HALO, 0, 16, 16), dz_pad=1),
    C("halo-m3-cin-odd", 9, 3, 2, 1, 9, 40, 18, 16, rid(9, F_HALO, 1, 16, 32), in_pad=2),
    C("halo-m3-narrow", 9, 3, 2, 1, 9, 9, 16, 16, rid(9, F_HALO, 1, 16, 16)),                      # W = 9 < 10: flat instead of the split tiles
    # volume geometry, taps 27 in mma 0: one plane, two planes, two volumes of three planes
    C("halo-vol-d1", 27, 0, 1, 1, 9, 16, 16, 16, rid(9, F_HALO, 0, 16, 16)),
    C("halo-vol-d2", 27, 0, 1, 2, 7, 20, 16, 16, rid(9, F_HALO, 1, 16, 16)),
    C("halo-vol-nv2", 27, 0, 2, 3, 9, 16, 20, 20, rid(9, F_HALO, 0, 32, 32), acc=1),
]
# ---- wgrad_split_kernel (mma 3): W = 10 the smallest rectangular-split width, 40, 250; taps 9 and 27 ------------------------------
T4S = [(16, 16, 12, 16), (16, 32, 16, 20), (32, 16, 20, 8), (32, 32, 20, 36)]
for i, ((cob, cib, co, ci), w) in enumerate(zip(T4S, [10, 40, 250, 16])):
    CASES.append(C(f"split-{cob}x{cib}-w{w}", 9, 3, 2, 1, 9, w, ci, co, rid(9, F_SPLIT, 0, cob, cib), dz_pad=4 * (i % 2), in_pad=4 * (i // 2), in_off=4 * (i // 2), acc=i % 2))
    CASES.append(C(f"split3d-{cob}x{cib}", 27, 3, 2, 3, 5, [40, 10, 16, 250][i], ci, co, rid(9, F_SPLIT, 0, cob, cib), acc=(i + 1) % 2))
CASES += [
    C("split-vol-d1", 27, 3, 1, 1, 9, 16, 16, 16, rid(9, F_SPLIT, 0, 16, 16)),
    C("split-vol-d2", 27, 3, 1, 2, 7, 20, 16, 16, rid(9, F_SPLIT, 0, 16, 16)),
    # 2 x 97 x 4 = 776 tiles on 768 workgroups (16-channel inputs: target 768), 2 x 65 x 4 = 520 on 512 (32-channel inputs): a ragged second round
    C("split-rounds", 9, 3, 2, 1, 770, 64, 16, 16, rid(9, F_SPLIT, 0, 16, 16), kinds=ALL),
    C("split-rounds-32", 9, 3, 2, 1, 520, 64, 32, 16, rid(9, F_SPLIT, 0, 16, 32), kinds=TWO),
    C("halo-rounds", 9, 0, 2, 1, 770, 16 * 4, 16, 16, rid(9, F_HALO, 0, 16, 16), kinds=ALL),   # 2 x 97 x 4 = 776 tiles on 768 workgroups
]
# ---- arco_conv3d_wgrad_pro: the tiles arco_conv_pro_ok admits at small shapes (taps 9, mma 3, W % 16 == 0, H % 16 == 0, Cin % 16 == 0 and
# Cout = 16 or 48: conv_sp.hip's launch_sp<4,1>; its other forms need 192 tiles) -------------------------------------------------
CASES += [
    C("pro-16x16-g2", 9, 3, 4, 1, 16, 16, 16, 16, rid(9, F_SPLIT, 1, 16, 16), pro=2, drop=0, kinds=TWO),
    C("pro-16x16-drop", 9, 3, 2, 1, 16, 32, 16, 16, rid(9, F_SPLIT, 1, 16, 16), pro=2, drop=1, kinds=TWO, dz_pad=4),
    C("pro-16x32-drop", 9, 3, 4, 1, 16, 16, 32, 16, rid(9, F_SPLIT, 1, 16, 32), pro=4, drop=1, kinds=TWO),
    C("pro-32x16", 9, 3, 2, 1, 16, 16, 16, 48, rid(9, F_SPLIT, 1, 32, 16), pro=2, drop=0, kinds=TWO, acc=1),
    C("pro-32x32-drop", 9, 3, 2, 1, 16, 16, 48, 48, rid(9, F_SPLIT, 1, 32, 32), pro=2, drop=1, kinds=TWO, in_pad=16),
]
# ---- wgrad_image3d_kernel<1|3>: one input channel, Cout in {4, 8, 12, 16}; planes smaller than a tile and ragged --------------------
for i, co in enumerate((4, 8, 12, 16)):
    CASES.append(C(f"image1-n{co}", 9, 0, 3, 1, *[(5, 3), (20, 37)][i % 2], 1, co, rid(9, F_IMAGE, 1, 16, 16), dz_pad=4 * (i % 2), in_pad=i, acc=i % 2))
    CASES.append(C(f"image3-n{co}", 27, 0, 2, 3, *[(20, 37), (5, 3)][i % 2], 1, co, rid(9, F_IMAGE, 3, 16, 16), in_pad=3 - i, acc=(i + 1) % 2))
CASES += [
    C("image1-n6-halo", 9, 0, 3, 1, 5, 3, 1, 6, rid(9, F_HALO, 1, 16, 16)),
    C("image3-ldz-odd-halo", 27, 0, 2, 3, 5, 16, 1, 8, rid(9, F_HALO, 0, 16, 16), dz_pad=1),
    C("image3-d1", 27, 0, 1, 1, 20, 37, 1, 16, rid(9, F_IMAGE, 3, 16, 16)),
    # the Cin = 1 fp32-volume exception of mma 4: f16 dZ against the fp32 volume
    C("image3-m4", 27, 4, 2, 3, 20, 37, 1, 16, rid(9, F_IMAGE, 3, 16, 16), acc=1),
    C("image1-m4", 9, 4, 2, 1, 5, 3, 1, 8, rid(9, F_IMAGE, 1, 16, 16), dz_pad=4),
]
# ---- hwgrad_kernel (mma 4, f16 operands): <.,.,9> four tiles at taps 9 and 27, <.,.,1> nine tiles -------------------------------------
T4H = [(16, 16, 12, 16), (16, 32, 16, 24), (32, 16, 19, 8), (32, 32, 20, 40)]
for i, ((cob, cib, co, ci), (h, w)) in enumerate(zip(T4H, [(9, 16), (5, 37), (8, 20), (11, 33)])):
    CASES.append(C(f"h9-{cob}x{cib}", 9, 4, 2, 1, h, w, ci, co, rid(9, F_HGRAD, 0, cob, cib), dz_pad=(0, 8, 0, 4)[i], in_pad=8 * (i % 2), acc=i % 2))
    CASES.append(C(f"h27-{cob}x{cib}", 27, 4, 2, 3, h if h < 9 else 5, w, ci, co + (co & 1), rid(9, F_HGRAD, 0, cob, cib), in_pad=8 * (i // 2), acc=(i + 1) % 2))
for i, (cob, cib, co, ci) in enumerate([(16, 16, 3, 8), (16, 32, 16, 24), (16, 64, 4, 64), (32, 16, 20, 16), (32, 32, 18, 32),
                                         (32, 64, 32, 72), (64, 16, 64, 8), (64, 32, 68, 24), (64, 64, 68, 72)]):
    CASES.append(C(f"h1-{cob}x{cib}", 1, 4, 1, 1, 3, 101, ci, co, rid(1, F_HGRAD, 0, cob, cib), dz_pad=(1 if co & 1 else 2 * (i % 2)), in_pad=8 * (i % 2), acc=i % 2))
CASES += [
    C("h9-head19", 9, 4, 2, 1, 20, 37, 16, 19, rid(9, F_HGRAD, 0, 32, 16)),                       # the 19-class head: ld_dz odd, 2-D
    C("h27-vol-d1", 27, 4, 1, 1, 9, 16, 16, 16, rid(9, F_HGRAD, 0, 16, 16)),
    C("h27-vol-d2", 27, 4, 1, 2, 7, 20, 16, 16, rid(9, F_HGRAD, 0, 16, 16)),
    C("h9-rounds", 9, 4, 2, 1, 520, 64, 16, 16, rid(9, F_HGRAD, 0, 16, 16), kinds=ALL),           # 2 x 65 x 4 = 520 tiles on 512 workgroups
]
# ---- himage_wgrad_kernel (arco_conv3x3_image_wgrad_h): K = 1 .. 4, ld_in > K, planes 5 x 3 and 33 x 16 ---------------------------------
for k in (1, 2, 3, 4):
    CASES.append(C(f"himage-k{k}", 9, 4, 3, 1, *[(5, 3), (33, 16)][k % 2], k, 16, rid(9, F_HIMAGE, 0, 16, k), entry=1, in_pad=(k % 3), dz_pad=8 * (k % 2), acc=k % 2))
# ---- the shapes whose tile count is above the slab reservation (many small planes): the workspace guard ------------------------------
CASES += [
    C("ws-256x1x16", 9, 0, 256, 1, 1, 16, 16, 16, rid(9, F_HALO, 0, 16, 16), table=True, kinds=TWO),
    C("ws-200x4x4-m3", 9, 3, 200, 1, 4, 4, 16, 16, rid(9, F_HALO, 1, 16, 16), table=True, kinds=TWO),
    C("ws-200x4x4-m4", 9, 4, 200, 1, 4, 4, 16, 16, rid(9, F_HGRAD, 0, 16, 16), table=True, kinds=TWO),
    C("ws-200x4x4-image", 9, 0, 200, 1, 4, 4, 1, 8, rid(9, F_IMAGE, 1, 16, 16), table=True, kinds=TWO),
    C("ws-300x2x2-m3", 27, 3, 1, 300, 2, 2, 16, 16, rid(9, F_HALO, 1, 16, 16), table=True, kinds=TWO),
    C("ws-512x1x16", 9, 0, 512, 1, 1, 16, 32, 32, rid(9, F_HALO, 0, 32, 32), table=True, kinds=TWO),
]
# ---- the three slab reductions (red: 1 wgrad_reduce_kernel<64,8>, 2 <16,32>, 3 wgrad_reduce4_kernel), one plane of one tile per slab:
# 1, 16 and 17 slabs; wgrad_reduce4_kernel needs more than 16 slabs, Cin % 4 == 0 and Cout Cin taps >= 4096 - one case just below each
CASES += [
    C("red-s1", 9, 0, 1, 1, 8, 16, 16, 16, rid(9, F_HALO, 0, 16, 16), kinds=TWO, red=1),
    C("red-s16", 9, 0, 16, 1, 8, 16, 16, 16, rid(9, F_HALO, 0, 16, 16), kinds=TWO, red=1, acc=1),
    C("red-s17", 9, 0, 17, 1, 8, 16, 16, 16, rid(9, F_HALO, 0, 16, 16), kinds=TWO, red=2),
    C("red4-s17", 9, 0, 17, 1, 8, 16, 16, 32, rid(9, F_HALO, 0, 32, 16), kinds=TWO, red=3, acc=1),
    C("red4-s16", 9, 0, 16, 1, 8, 16, 16, 32, rid(9, F_HALO, 0, 32, 16), kinds=TWO, red=1),
    C("red-s17-below-4096", 9, 0, 17, 1, 8, 16, 16, 28, rid(9, F_HALO, 0, 32, 16), kinds=TWO, red=2, acc=1),
    C("red-s17-cin18", 9, 0, 17, 1, 8, 16, 18, 32, rid(9, F_HALO, 0, 32, 32), kinds=TWO, red=2),
    C("h-red-s1", 9, 4, 1, 1, 8, 16, 16, 16, rid(9, F_HGRAD, 0, 16, 16), kinds=TWO, red=1, acc=1),
    C("h-red-s17", 9, 4, 17, 1, 8, 16, 16, 16, rid(9, F_HGRAD, 0, 16, 16), kinds=TWO, red=2),
    C("h-red4-s17", 9, 4, 17, 1, 8, 16, 16, 32, rid(9, F_HGRAD, 0, 32, 16), kinds=TWO, red=3),
    C("g1-red-s1", 1, 0, 1, 1, 1, 100, 64, 64, rid(1, F_GEMM, 0, 64, 64), kinds=TWO, red=1),
    C("g1-red-s16", 1, 0, 1, 1, 1, 2048, 64, 64, rid(1, F_GEMM, 0, 64, 64), kinds=TWO, red=1),
    C("g1-red4-s17", 1, 0, 1, 1, 1, 2171, 64, 64, rid(1, F_GEMM, 0, 64, 64), kinds=TWO, red=3, acc=1),
    C("g1-red-s17-cout63", 1, 0, 1, 1, 1, 2171, 64, 63, rid(1, F_GEMM, 0, 32, 64), kinds=TWO, red=2),
]
NAMES = [c["name"] for c in CASES]
assert len(set(NAMES)) == len(NAMES)
FAMILY = {F_GEMM: "wgrad_kernel", F_Q: "wgrad_q_kernel", F_HALO: "wgrad_halo2_kernel", F_SPLIT: "wgrad_split_kernel",
          F_IMAGE: "wgrad_image3d_kernel", F_HGRAD: "hwgrad_kernel", F_HIMAGE: "himage_wgrad_kernel"}
# arco_conv3d_wgrad_pro: the statuses it must answer ARCO_ERR_UNSUPPORTED with (taps, mma, nv, d3, h, w, cin, cout, ld_dz, groups)
PRO_UNSUPPORTED = [("taps27", 27, 3, 2, 2, 16, 16, 16, 16, 16, 2), ("flat", 9, 3, 2, 1, 16, 9, 16, 16, 16, 2),
                   ("mma0", 9, 0, 2, 1, 16, 16, 16, 16, 16, 2), ("mma4", 9, 4, 2, 1, 16, 16, 16, 16, 16, 2),
                   ("ldz-odd", 9, 3, 2, 1, 16, 16, 16, 16, 17, 2), ("groups", 9, 3, 3, 1, 16, 16, 16, 16, 16, 2)]
# hwgrad_dispatch / arco_conv3x3_image_wgrad_h rejections (taps, cin, cout, ld_dz, ld_in)
H_UNSUPPORTED = [("cin&7", 9, 12, 16, 16, 16), ("ld_in&7", 9, 16, 16, 16, 20), ("ldz-odd-27", 27, 16, 19, 19, 16), ("ldz-odd-1", 1, 16, 19, 19, 16),
                 ("cin1-cout20", 9, 1, 20, 20, 1), ("cin1-ldz-odd", 27, 1, 16, 18, 1)]      # f16 dZ, fp32 volume: wgrad_image3d_kernel or nothing


def by_name(name):
    return CASES[NAMES.index(name)]


# ======================================================================================================================================
# geometry restated from the dispatcher (what the bounds need) and the documented slab targets
# ======================================================================================================================================
def n_tiles(c):
    NB, H, W, M, f = c["nv"] * c["d3"], c["h"], c["w"], c["M"], c["fam"]
    if f == F_GEMM or (f == F_HGRAD and c["taps"] == 1):
        return -(-M // 128)
    if f == F_Q:
        return -(-M // 64)
    if f in (F_IMAGE, F_HIMAGE):
        return NB * -(-H // 16) * -(-W // 16)
    if f == F_HALO and c["var"] & 1:
        return NB * -(-(H * (W + 2)) // 128)
    return NB * -(-H // 8) * -(-W // 16)


def pads(c):
    """(CoutPad, CinPad) of the slabs"""
    f = c["fam"]
    if f in (F_IMAGE, F_HIMAGE):
        return 16, 16
    if f == F_Q:
        return -(-c["n"] // 128) * 128, -(-c["k"] // 128) * 128
    return -(-c["n"] // c["cob"]) * c["cob"], -(-c["k"] // c["cib"]) * c["cib"]


def slab_floats(c):
    a, b = pads(c)
    return c["taps"] * a * b


def target_slabs(c):
    """the dispatcher's documented slab target: 768 (halo kernels, and the split kernel on 16-channel inputs) or 512 (image, hwgrad,
    1x1), divided by ydim * zdim - the most slabs any version of the dispatcher writes, whatever the tile count"""
    f, (a, b) = c["fam"], pads(c)
    if f in (F_IMAGE, F_HIMAGE):
        return 512
    if f == F_Q:
        return max(1, 512 // ((a // 128) * (b // 128)))
    y = (a // c["cob"]) * (b // c["cib"])
    if f in (F_HALO, F_SPLIT):
        return max(1, 768 // (y * (c["taps"] // 9)))
    if f == F_HGRAD and c["taps"] >= 9:
        return max(1, 512 // (y * (c["taps"] // 9)))
    return max(1, 512 // (y * (c["taps"] if f == F_GEMM else 1)))


def n_reduce(slabs, kind):
    gr = 8 if kind == 1 else 32
    return -(-slabs // (2 * gr)) + 3 + gr // 4


def chain(c):
    """(r, P, cross) of the route, see the docstring"""
    f = c["fam"]
    wps = max(1, 4 // ((c["cob"] // 16) * (c["cib"] // 16))) if f in (F_HALO, F_SPLIT) else 4
    if f == F_GEMM:
        return 2, 32, 2
    if f == F_Q:
        return 2, 64, 0
    if f == F_HALO:
        return (1 if c["bf16"] else 2), 128 // wps, wps - 1
    if f == F_SPLIT:
        return 6, 128 // wps, wps - 1
    if f == F_IMAGE:
        return 2, 64, 3
    if f == F_HGRAD:
        return 1, 32, 2
    return 1, 256, 0


def n_roundings(c, slabs, kind):
    r, P, cross = chain(c)
    return r * P * -(-n_tiles(c) // slabs) + cross + n_reduce(slabs, kind) + c["acc"]


# ======================================================================================================================================
# the float64 weight gradient
# ======================================================================================================================================
def wgrad64(dz, x, c):
    """dz [M, Cout], x [M, Cin] float64 -> dW [Cout, Cin, taps]"""
    return torch.einsum("mo,mtk->okt", dz, im2col(x, c))


def finish(c, d):
    dz, x = d["dz"].double(), d["x"].double()
    a = d.get("act64", x)                                                  # (pro: the float64 activation of z = x)
    d["ref0"] = wgrad64(dz, a, c)
    d["S"] = wgrad64(dz.abs(), a.abs(), c) if d["kind"] in ("fixed", "wide") else d["ref0"].abs()
    d["ref"] = d["ref0"] + d["dw0"].double() if c["acc"] else d["ref0"]
    d["Sacc"] = d["S"] + d["dw0"].double().abs() if c["acc"] else d["S"]
    return d


def _operand(v, half):
    """values as the kernel sees them: f16 operands are GENERATED as f16 (the reference reads the same numbers)"""
    if not half:
        return v.float()
    h = v.to(torch.float16)
    h[h.float().abs() < 2.0 ** -14] = 0                                    # (inside the normal range of f16)
    return h


def impulse_pixels(c):
    """first, last (the last persistent round), both other corners of the first plane, a pixel of the ragged last tile, the first and
    last plane of every volume: at most `n` of them, each gets its own channel"""
    NB, H, W = c["nv"] * c["d3"], c["h"], c["w"]
    px = lambda b, y, x: (b * H + y) * W + x
    want = [px(0, 0, 0), px(NB - 1, H - 1, W - 1), px(0, 0, W - 1), px(0, H - 1, 0)]
    for v in range(c["nv"]):
        want += [px(v * c["d3"], H // 2, W // 2), px(v * c["d3"] + c["d3"] - 1, H - 1, W - 1), px(v * c["d3"] + c["d3"] - 1, 0, min(1, W - 1))]
    want += [px(NB // 2, H - 1, W - 1), px(NB - 1, 0, 0), px(NB // 2, H // 2, 0)]
    out = []
    for p in want:
        if p not in out:
            out.append(p)
    return out


def wide9(shape, g):
    return (257 + 2 * _ints(shape, g, 0, 15)) * (2 * _ints(shape, g, 0, 1) - 1)


@functools.lru_cache(maxsize=2)
def _data(name, kind):
    c = by_name(name)
    g = gen(sum(map(ord, name)), len(kind), ALL.index(kind))
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    d = dict(kind=kind)
    if kind == "fixed":
        zi, xi = _ints((M, N), g, -3, 3), _ints((M, K), g, -3, 3)
        if c["fam"] == F_SPLIT and not c["pro"]:                           # 9-bit values on both operands, a few pixels of a few channels
            rows = torch.tensor(impulse_pixels(c)[:8])
            for ch in {0, N - 1}:
                zi[rows, ch] = wide9((len(rows),), g)
            for ch in {0, K - 1}:
                xi[rows, ch] = wide9((len(rows),), g)
        dz, x = zi.double() * QZ, xi.double() * QX
        dw0 = _ints((N, K, T), g, -2 ** 12, 2 ** 12).float() * QUANT
    elif kind in ("impulse", "impulse_x"):
        rnd, n_imp = _wide_values, (N if kind == "impulse" else K)
        pos = impulse_pixels(c)[:n_imp]
        unit = torch.zeros((M, n_imp), dtype=torch.float64)                # (channels past the last impulse stay zero)
        for i, m in enumerate(pos):
            unit[m, i] = 1.0
        full = rnd((M, K if kind == "impulse" else N), g, 2 if (c["xh"] or c["zh"]) else 3, 0.2).double()
        dz, x = (unit, full) if kind == "impulse" else (full, unit)
        d["pos"] = pos
        dw0 = torch.zeros((N, K, T))
    else:
        dec = 2 if (c["xh"] or c["zh"]) else 3
        dz, x = _wide_values((M, N), g, dec, 0.2).double(), _wide_values((M, K), g, dec, 0.2).double()
        dw0 = _wide_values((N, K, T), g, 2, 0.0)
    d["dz"], d["x"], d["dw0"] = _operand(dz, c["zh"]), _operand(x, c["xh"]), dw0
    if c["pro"]:
        return d                                                           # (the GPU file adds the mask, then pro_finish)
    return finish(c, d)


def data(c, kind):
    """the inputs, the float64 reference and S of one case and kind; computed once, never modified"""
    return _data(c["name"], kind)


def exactness_budget(c, d):
    """fixed kind: the largest sum |dz||x| (+ |dW0|) of any element, in quanta - below 2^24 every partial sum is an exact integer
    (consumer-side activation: the activation is a multiple of 2^-9, the quantum 2^-12)"""
    return float(d["Sacc"].max()) / (QUANT / 16 if c["pro"] else QUANT)


# ---- the consumer-side activation ---------------------------------------------------------------------------------------------------
SLOPE, P_DROP = 0.25, 0.5                                                  # (exact in fp32: slope 2^-2, keep scale 1 / (1 - p) = 2)


def pro_params(c, kind):
    """mean, istd [groups, K], gamma, beta [K] fp32.  fixed kind: integers and powers of two, so that the fp32 arithmetic of the loader is
    exact (z - mean an integer of 2^-5, times 2^a, times +-2^b, plus an integer of 2^-5; slope 2^-2; keep scale 2)"""
    g = gen(sum(map(ord, c["name"])), 99, len(kind))
    G, K = c["pro"], c["k"]
    if kind == "fixed":
        mean = _ints((G, K), g, -2, 2).float() * QX
        istd = 2.0 ** _ints((G, K), g, -1, 1).float()
        gam = (2 * _ints((K,), g, 0, 1) - 1).float() * 2.0 ** _ints((K,), g, -1, 0).float()
        beta = _ints((K,), g, -2, 2).float() * QX
    else:
        mean = torch.randn((G, K), generator=g) * 0.3
        istd = torch.rand((G, K), generator=g) + 0.5
        gam = torch.randn((K,), generator=g)
        beta = torch.randn((K,), generator=g) * 0.2
    return mean, istd, gam, beta


def pro_act64(c, z, prm, keep):
    """float64 dropout(lrelu((z - mean) * istd * gamma + beta)) from the fp32 operands; keep [M, K] bool or None; also the bound of the
    loader's own fp32 error per element (six roundings)"""
    mean, istd, gam, beta = (t.double() for t in prm)
    G, K = c["pro"], c["k"]
    zg = z.double().view(G, c["M"] // G, K)
    v = (zg - mean[:, None, :]) * istd[:, None, :] * gam[None, None, :] + beta[None, None, :]
    mag = (zg - mean[:, None, :]).abs() * (istd[:, None, :] * gam[None, None, :]).abs() + beta.abs()[None, None, :]
    a = torch.where(v >= 0, v, v * SLOPE).view(c["M"], K)
    mag = mag.view(c["M"], K)
    if keep is not None:
        scale = 1.0 / (1.0 - P_DROP)
        a, mag = a * keep * scale, mag * keep * scale
    return a, gamma(6) * mag


def pro_finish(c, d, prm, keep):
    d["act64"], aerr = pro_act64(c, d["x"], prm, keep)
    finish(c, d)
    d["Spro"] = wgrad64(d["dz"].double().abs(), aerr, c)
    return d


# ======================================================================================================================================
# bounds and comparisons
# ======================================================================================================================================
LAMBDA = 9.0


def gamma_n(n):
    """the smaller of the worst-case constant gamma(n) and the probabilistic LAMBDA sqrt(n) u (see the docstring)"""
    return min(gamma(n), LAMBDA * math.sqrt(n) * U)


def tol_wide(c, d, slabs, kind):
    t = gamma_n(n_roundings(c, slabs, kind)) * d["Sacc"] + U * d["ref"].abs()
    if c["fam"] == F_SPLIT:
        t = t + DROP * d["S"]
    if c["bf16"]:
        t = t + BF16 * d["S"]
    if c["pro"]:
        t = t + d["Spro"]
    return t


def held(name, got, c, d, slabs, kind):
    r = worst(got, d["ref"], tol_wide(c, d, slabs, kind))
    print(f"{name} [{FAMILY[c['fam']]}]: worst err / bound {r:.4f} (n = {n_roundings(c, slabs, kind)})")
    return r


def impulse_expected(c, d):
    """the impulse kinds restated without a matrix product: every dW row is one shifted operand row or zero"""
    T, (N, K) = c["taps"], (c["n"], c["k"])
    cols_ = im2col(d["x"].double(), c)                                    # [M, T, K]
    out = torch.zeros((N, K, T), dtype=torch.float64)
    if d["kind"] == "impulse":
        for i, m in enumerate(d["pos"]):
            out[i] = cols_[m].t()
    else:
        dz = d["dz"].double()
        for i, m in enumerate(d["pos"]):                                  # x has its impulse at pixel m, channel i: dW[:, i, t] = dz[m'] with m' + t = m
            hit = cols_[:, :, i]                                          # [M, T] one where pixel m' + tap t is the impulse
            for t in range(T):
                rows = torch.nonzero(hit[:, t]).flatten()
                assert len(rows) <= 1
                if len(rows):
                    out[:, i, t] = dz[rows[0]]
    return out


# ---- fp32 emulation of the wide kind: chains of P pixels, the partials summed as a balanced tree ----------------------------------------
def emulate(c, d, slabs, kind):
    f32 = np.float32
    r, P, cross = chain(c)
    a = d.get("act64")
    x = d["x"].float() if a is None else a.float()                          # (pro: the activation rounded once - inside its gamma(6) term)
    cols_ = im2col(x, c).numpy().astype(f32)                                # [M, T, K]
    dz = d["dz"].float().numpy()
    M = dz.shape[0]
    if c["bf16"]:
        cols_, dz = bf16_rne(cols_), bf16_rne(dz)
    parts = []
    for m0 in range(0, M, P):
        acc = np.zeros((c["n"], c["taps"], c["k"]), dtype=f32)
        for m in range(m0, min(M, m0 + P)):
            if c["fam"] == F_SPLIT:
                zs, xs = split_act(dz[m]), split_act(cols_[m])
                for i, j in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
                    acc = (acc.astype(np.float64) + zs[i].astype(np.float64)[:, None, None] * xs[j].astype(np.float64)[None]).astype(f32)
            elif r == 2:
                acc = (acc + (dz[m][:, None, None] * cols_[m][None]).astype(f32)).astype(f32)
            else:
                acc = (acc.astype(np.float64) + dz[m].astype(np.float64)[:, None, None] * cols_[m].astype(np.float64)[None]).astype(f32)
        parts.append(acc)
    depth = 0
    while len(parts) > 1:
        parts = [(parts[i] + parts[i + 1]).astype(f32) if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        depth += 1
    assert depth <= cross + n_reduce(slabs, kind), "the emulation's tree is deeper than the route's own"
    out = torch.from_numpy(parts[0]).permute(0, 2, 1).contiguous()
    return (out + d["dw0"]).float() if c["acc"] else out


# ======================================================================================================================================
# arco_colsum / arco_colsum_h and arco_transpose2d
# ======================================================================================================================================
def CS(name, M, Cc, pad=0, half=False, acc=0):
    return dict(name=name, M=M, C=Cc, ldx=Cc + pad, half=half, acc=acc)


COLSUM = [CS(f"c{Cc}-m{M}{'-h' if half else ''}", M, Cc, pad, half, acc) for (M, Cc, pad, half, acc) in [
    (511, 12, 0, False, 0), (513, 12, 4, True, 1), (1, 1024, 0, False, 1), (513, 1024, 4, True, 0), (511, 64, 8, False, 1),     # C % 4 == 0 <= 1024
    (511, 2, 0, False, 1), (513, 19, 2, True, 0), (1, 255, 0, False, 0), (513, 255, 3, False, 1), (511, 20, 1, True, 1),        # odd C or ldx, <= 256
    (511, 257, 0, True, 0), (513, 1028, 0, False, 1), (1, 257, 3, False, 0),                                                    # C > 256 odd, C > 1024
    (1024 * 512 + 1, 4, 0, False, 0), (1024 * 512 + 1, 2, 1, True, 1), (1024 * 600 + 77, 12, 4, False, 1)]]                     # blocks of > 512 rows; the last ones empty
TRANSPOSE = [(r, cl, pr, pc) for r in (1, 31, 32, 33, 100) for (cl, pr, pc) in ((1, 0, 3), (31, 5, 0), (32, 1, 1), (33, 0, 0), (100, 7, 2))]


def colsum_blocks(M):
    nblk = min(1024, max(1, -(-M // 512)))
    rpb = -(-M // nblk)
    return nblk, rpb


def colsum_n(cs):
    Cc, ldx = cs["C"], cs["ldx"]
    nblk, rpb = colsum_blocks(cs["M"])
    if Cc % 4 == 0 and ldx % 4 == 0 and Cc <= 1024:
        rstep = 256 // (Cc // 4)
    elif Cc <= 256:
        rstep = 256 // Cc
    else:
        rstep = 1
    return -(-rpb // rstep) + rstep + cs["acc"]


@functools.lru_cache(maxsize=2)
def _colsum_data(name, kind):
    cs = COLSUM[[c["name"] for c in COLSUM].index(name)]
    g = gen(sum(map(ord, name)), len(kind))
    M, Cc = cs["M"], cs["C"]
    if kind == "fixed":
        x = _ints((M, Cc), g, -7, 7).double() * QZ                         # (M * 7 < 2^24 quanta)
        out0 = _ints((Cc,), g, -2 ** 10, 2 ** 10).float() * QZ
    else:
        x = _wide_values((M, Cc), g, 2 if cs["half"] else 3, 0.2).double()
        out0 = _wide_values((Cc,), g, 2, 0.0)
    x = _operand(x, cs["half"])
    ref = x.double().sum(0)
    S = x.double().abs().sum(0)
    if cs["acc"]:
        ref, S = ref + out0.double(), S + out0.double().abs()
    return dict(x=x, out0=out0, ref=ref, S=S, kind=kind)


def colsum_data(cs, kind):
    return _colsum_data(cs["name"], kind)


def colsum_emulate(cs, d):
    """colsum_partial_kernel's own order in fp32: per block rstep chains of every rstep-th row, then the rstep partials in turn; the
    blocks in float64, rounded once; accumulate in fp32"""
    f32 = np.float32
    x = d["x"].float().numpy()
    M, Cc = x.shape
    nblk, rpb = colsum_blocks(M)
    n = colsum_n(cs) - cs["acc"]
    rstep = 1 if (Cc > 256 and not (Cc % 4 == 0 and cs["ldx"] % 4 == 0 and Cc <= 1024)) else (256 // (Cc // 4) if (Cc % 4 == 0 and cs["ldx"] % 4 == 0) else 256 // Cc)
    assert n == -(-rpb // rstep) + rstep
    total = np.zeros(Cc, dtype=np.float64)
    for b in range(nblk):
        r0, r1 = b * rpb, min(M, (b + 1) * rpb)
        a = np.zeros(Cc, dtype=f32)
        for tr in range(rstep):
            s = np.zeros(Cc, dtype=f32)
            for r in range(r0 + tr, r1, rstep):
                s = (s + x[r]).astype(f32)
            a = (a + s).astype(f32)
        total += a.astype(np.float64)
    out = total.astype(f32)
    if cs["acc"]:
        out = (d["out0"].numpy() + out).astype(f32)
    return torch.from_numpy(out)


def colsum_tol(cs, d):
    return gamma(colsum_n(cs)) * d["S"] + 2 * U * d["ref"].abs()           # (the float64 total rounded to fp32, and the accumulate)
