"""Cases, inputs, float64 references, per-element bounds and comparison helpers shared by tests/test_conv_kernels_gpu.py (every forward
convolution route of csrc/igemm.hip, conv_sp.hip, gemm_sp.hip and conv3d_fl.hip, one route per test, called directly) and
tests/test_conv_kernels_cpu.py (the routes asserted through the host queries, the input conditions, an fp32 emulation of the bounded
kind inside the same bounds, planted errors).  Plain CPU torch / numpy only; nothing here touches a GPU.

A CASE names one route: the kernel id (include/arco_hip.h) that the dispatcher must choose for its shape, which the GPU file asserts
through arco_conv_last_route and the CPU file through arco_conv_config_mma where the query describes the route.  Activations are rows
[M, K] (channels last), M = nv * d3 * h * w; weights are in the torch layout [N, K, taps] and packed by arco_pack_conv_weight.

Three kinds of input per case (the issue's (a), (b), (c)):
  fixed     every x, w, bias and residual an integer multiple of a power of two, (sum|x||w| + |b| + |r|) / quantum < 2^24 per output:
            every product and every partial sum in any order is exact in fp32 - the kernel must equal the float64 convolution bit for
            bit.  WIDE channels hold 9-bit integers (257 .. 287, odd) on BOTH operands: two non-zero bf16 terms each, so all four of
            their cross products (planes 0 and 1 of both operands) are among the six the split-bf16 kernels keep.
  impulse   full 24-bit random w against unit impulses (each in its own channel, more than the kernel extent apart): every output is
            one weight or zero, bit for bit - plane 2 of the weights.
  select    full 24-bit random x against weights with one entry +-2^e per output channel, every tap used (several passes where
            N < taps): the output is the scaled shifted input, zero past the border, bit for bit - plane 2 of the activations.
  wide      six decades of magnitudes, 20 % exact zeros: |err| <= tol per element, tol derived below, and the measured figure
            |err| <= 3e-6 S of tests/test_split_mma_gpu.py, S = conv(|x|, |w|) + |bias| + |res|.

Bounds of the wide kind (u = 2^-24, gamma(n) = n u / (1 - n u); tol = gamma(n) S + u |ref|, + (2^-23 + 2^-24) conv(|x|,|w|) for mma 3):
  nout   conv1x1_narrow_out_kernel<Q>: x0 w0 (1 rounding), three fmaf (3), log2 Q butterfly additions, + bias (1): n = 5 + log2 Q; the
         split pack's three terms are summed back (b0 + b1) + b2 without rounding (b0 + b1 is w rounded to 16 bits).
  nin    conv1x1_narrow_in_kernel: K fmaf onto the bias, + residual: n = K + 1.
  image  conv3x3_image_kernel / conv3d_image_kernel<D>: acc = bias; acc += w x over taps K terms - one rounding each as a fused
         multiply-add, two as a product and a sum; the compiler chooses, n = 2 taps K covers both.
  mfma0  the fp32 matrix-core kernels (igemm_kernel, conv3x3_halo_kernel; mma 0): a product of two fp32 values is not representable; at
         most one rounding for it and one for its accumulation, in whatever order the hardware adds the 4 k of an instruction: n =
         2 taps K + 2 (bias, residual in the epilogue).  Zero padding adds exact zeros.
  mfma3  the split-bf16 kernels (mma 3: igemm_kernel, conv_sp.hip, gemm_sp.hip, conv3d_fl.hip): a product of two bf16 terms has 16
         bits and is exact; every kept product is one accumulation: n = 6 taps K + 2.  The three dropped products are bounded by
         (2^-23 + 2^-24) |x||w| (split_bf16.h).  Rigorous and loose at large K; the measured 3e-6 S is what binds there."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from loss_kernel_refs import U, gamma, gen, worst

DROP = 2.0 ** -23 + 2.0 ** -24                       # the dropped (1,2), (2,1), (2,2) term products of mma 3, relative to |x||w|
MEASURED = 3e-6                                      # tests/test_split_mma_gpu.py: |err| / sum|x||w|, a measured figure
ERR_ARG, ERR_UNSUPPORTED = -1, -3
ALL = ("fixed", "impulse", "select", "wide")


def C(name, taps, mma, nv, d3, h, w, k, n, route, fam, **opt):
    c = dict(name=name, taps=taps, mma=mma, nv=nv, d3=d3, h=h, w=w, k=k, n=n, route=route, fam=fam, in_pad=0, in_off=0, out_pad=0,
             bias=False, res=False, res_pad=0, gsp=False, fl0=False, launch_only=False, kinds=ALL, stats=0)
    assert set(opt) <= set(c), opt
    c.update(opt)
    c["M"] = nv * d3 * h * w
    c["ld_in"], c["ld_out"], c["ld_res"] = k + c["in_pad"], n + c["out_pad"], (n + c["res_pad"] if c["res"] else 0)
    return c


def _modes(name, taps, nv, d3, h, w, k, n, route, **opt):
    """the same shape in mma 0 and mma 3 (the igemm_kernel tiles: one instantiation id for both modes)"""
    return [C(f"{name}-m{m}", taps, m, nv, d3, h, w, k, n, route, "mfma3" if m == 3 else "mfma0", **opt) for m in (0, 3)]


TWO = ("fixed", "wide")                              # the largest 3x3x3 tiles (their float64 references take a second each): two kinds
# ---- 1x1 ---------------------------------------------------------------------------------------------------------------------------
# conv1x1_stream_dispatch: M >= 65536, no statistics; narrow-out K in {4, 8, 16, 32}, N <= 4, no residual, both pack formats;
# narrow-in mma 0, K <= 4, N in {4, 8, 16, 32}.  M = 257 * 257 = 66049: 513 past the threshold, odd, a ragged last workgroup.
CASES_1X1 = [
    C("nout-q1-n1-m0", 1, 0, 1, 1, 257, 257, 4, 1, 1604004, "nout", launch_only=True, bias=True),
    C("nout-q1-n4-m3", 1, 3, 1, 1, 257, 257, 4, 4, 1604004, "nout", launch_only=True, out_pad=4),
    C("nout-q2-n2-m3", 1, 3, 1, 1, 257, 257, 8, 2, 1608004, "nout", launch_only=True, in_pad=8, in_off=4, out_pad=2),
    C("nout-q2-n3-m0", 1, 0, 1, 1, 257, 257, 8, 3, 1608004, "nout", launch_only=True),
    C("nout-q4-n3-m0", 1, 0, 1, 1, 257, 257, 16, 3, 1616004, "nout", launch_only=True, bias=True, out_pad=1),
    C("nout-q4-n2-m3", 1, 3, 1, 1, 257, 257, 16, 2, 1616004, "nout", launch_only=True, bias=True),
    C("nout-q8-n4-m3", 1, 3, 1, 1, 257, 257, 32, 4, 1632004, "nout", launch_only=True, bias=True, in_pad=4),
    C("nout-q8-n1-m0", 1, 0, 1, 1, 257, 257, 32, 1, 1632004, "nout", launch_only=True),
    C("nin-k1-n4", 1, 0, 1, 1, 257, 257, 1, 4, 1700000, "nin", launch_only=True, bias=True),
    C("nin-k2-n8-res", 1, 0, 1, 1, 257, 257, 2, 8, 1700000, "nin", launch_only=True, res=True, res_pad=4, in_pad=2),
    C("nin-k3-n16-both", 1, 0, 1, 1, 257, 257, 3, 16, 1700000, "nin", launch_only=True, bias=True, res=True, out_pad=4),
    C("nin-k4-n32", 1, 0, 1, 1, 257, 257, 4, 32, 1700000, "nin", launch_only=True, in_pad=4, in_off=4),
    # gemm_sp_kernel<false> with arco_gemm_sp_set(1, 1): taken from Npad >= 208 on (a 256-wide tile may waste a fifth at most), so
    # N = 64 stays on igemm_kernel<1,32,64> whatever the tile threshold - asserted as such
    C("gsp-n208-k32", 1, 3, 1, 1, 1, 333, 32, 208, 1464256, "mfma3", launch_only=True, gsp=True, bias=True, res=True, res_pad=4),
    C("gsp-n496-k100", 1, 3, 1, 1, 3, 67, 100, 496, 1464256, "mfma3", launch_only=True, gsp=True, res=True, in_pad=4, out_pad=4),
    C("gsp-n496-k32-bias", 1, 3, 1, 1, 1, 8333, 32, 496, 1464256, "mfma3", launch_only=True, gsp=True, bias=True),
    C("gsp-n64-refused", 1, 3, 1, 1, 1, 333, 32, 64, 1032064, "mfma3", gsp=True, bias=True, res=True),
]
# igemm_kernel<1, BM, BN>: 256x16 (Npad <= 16), 128x32 (Npad <= 32), 32x64 (fewer than 192 64x64 tiles), 64x64, 64x224 (N = 192 / 448 and
# M Npad > 4096 * 1024), 128x128
CASES_1X1 += (
    _modes("g256x16", 1, 1, 1, 3, 101, 20, 4, 1256016, bias=True, out_pad=4)
    + [C("g256x16-scalar-k19-m0", 1, 0, 2, 1, 7, 23, 19, 2, 1256016, "mfma0", res=True)]
    + _modes("g128x32", 1, 2, 1, 9, 17, 48, 19, 1128032, res=True, res_pad=5, in_pad=4, in_off=4)
    + _modes("g32x64", 1, 1, 1, 5, 41, 48, 80, 1032064, bias=True, res=True)
    + _modes("g64x64", 1, 1, 1, 61, 100, 48, 100, 1064064, bias=True)
    + _modes("g64x224", 1, 1, 1, 150, 146, 32, 192, 1064224, res=True)
    + _modes("g128x128", 1, 1, 1, 200, 164, 20, 128, 1128128, bias=True))

# ---- 3x3 ---------------------------------------------------------------------------------------------------------------------------
CASES_3X3 = [
    C("image1-k1", 9, 0, 3, 1, 20, 37, 1, 16, 9701016, "image", bias=True, out_pad=4),
    C("image1-k1-small", 9, 0, 1, 1, 5, 3, 1, 12, 9701016, "image"),
    C("image-k3", 9, 0, 3, 1, 20, 37, 3, 16, 9803016, "image", bias=True),
    C("image-k4-n12", 9, 0, 2, 1, 33, 16, 4, 12, 9804016, "image", in_pad=4, out_pad=4),
    C("halo-16-16", 9, 0, 2, 1, 20, 37, 16, 16, 9916016, "mfma0", bias=True),
    C("halo-16-32", 9, 0, 2, 1, 20, 37, 16, 20, 9916032, "mfma0", res=True, res_pad=4, out_pad=4),
    C("halo-32-16", 9, 0, 1, 1, 5, 7, 32, 12, 9932016, "mfma0", in_pad=8, in_off=4),
    C("halo-32-32", 9, 0, 3, 1, 9, 50, 32, 32, 9932032, "mfma0", bias=True, res=True),
]
# dispatch_spatial<1>: every tile in both modes; K = 20 keeps mma 0 off the halo kernel, W = 250 keeps mma 3 off conv_sp.hip; the
# thresholds are want_blocks = 512 workgroups
CASES_3X3 += (
    _modes("s256x16", 9, 2, 1, 256, 250, 20, 4, 9256016, bias=True)
    + _modes("s128x16", 9, 1, 1, 256, 250, 20, 8, 9128016)
    + _modes("s64x16", 9, 1, 1, 20, 19, 20, 2, 9064016, bias=True, res=True, out_pad=2)
    + _modes("s128x32", 9, 2, 1, 128, 250, 20, 20, 9128032, res=True)
    + _modes("s64x32", 9, 2, 1, 11, 21, 48, 19, 9064032, bias=True, in_pad=4, in_off=4, out_pad=5)
    + _modes("s128x64", 9, 2, 1, 128, 250, 16, 64, 9128064, bias=True)
    + _modes("s64x64", 9, 1, 1, 128, 250, 16, 64, 9064064)
    + _modes("s64x32w", 9, 1, 1, 64, 250, 16, 64, 9064032, res=True)
    + _modes("s32x32", 9, 1, 1, 7, 5, 20, 48, 9032032, bias=True, res=True, res_pad=4))
# the persistent kernels with more tiles than workgroups (256 CUs: 800 > 768, 528 > 512, 1200 > 1024 tiles) and a ragged last round
CASES_3X3 += [
    C("halo-16-16-rounds", 9, 0, 2, 1, 128, 800, 16, 16, 9916016, "mfma0", bias=True, stats=1),
    C("halo-32-32-rounds", 9, 0, 2, 1, 64, 520, 32, 32, 9932032, "mfma0", res=True, stats=2),
    C("image-k3-rounds", 9, 0, 5, 1, 240, 250, 3, 16, 9803016, "image", bias=True, stats=1),
]
# conv_sp.hip (mma 3): launch_sp<A_T, C_T> (ids 9.3e6 + A_T 1e3 + 16 C_T) needs CONV_SP_MIN_TILES = 192 work items; C_T = 1 exists only
# with A_T = 4 (dispatch_rows<1> is never called: <2,1> and <1,1> are unreachable).  launch_rw: 9.35e6 + rows / 4 * 1e3 + BN.
CASES_3X3 += [
    C("sp-4-4", 9, 3, 5, 1, 128, 128, 16, 64, 9304064, "mfma3", bias=True, stats=1),
    C("sp-2-4", 9, 3, 5, 1, 64, 128, 16, 64, 9302064, "mfma3", res=True, res_pad=4),
    C("sp-1-4", 9, 3, 3, 1, 32, 128, 32, 64, 9301064, "mfma3", bias=True, res=True, in_pad=16, in_off=4, out_pad=4),
    C("sp-4-2", 9, 3, 2, 1, 128, 128, 16, 96, 9304032, "mfma3"),
    C("sp-2-2", 9, 3, 1, 1, 64, 128, 48, 96, 9302032, "mfma3", bias=True),
    C("sp-1-2", 9, 3, 1, 1, 32, 128, 16, 96, 9301032, "mfma3", res=True),
    C("sp-4-1-small", 9, 3, 1, 1, 16, 16, 16, 48, 9304016, "mfma3", bias=True, stats=1),
    C("rw-418-16-16", 9, 3, 5, 1, 128, 256, 16, 16, 9358016, "mfma3", bias=True, stats=1),
    C("rw-418-16-4", 9, 3, 3, 1, 128, 256, 16, 4, 9358016, "mfma3", out_pad=4),
    C("rw-418-4-16", 9, 3, 5, 1, 128, 256, 4, 16, 9358016, "mfma3", res=True, in_pad=4),
    C("rw-418-32-16", 9, 3, 3, 1, 128, 256, 32, 16, 9358016, "mfma3", bias=True, res=True),
    C("rw-228", 9, 3, 6, 1, 128, 128, 32, 32, 9354032, "mfma3", bias=True, res=True, stats=2),
    C("rw-228-k16", 9, 3, 3, 1, 128, 128, 16, 32, 9354032, "mfma3"),
]

# ---- 3x3x3 -------------------------------------------------------------------------------------------------------------------------
CASES_3D = [
    C("image3", 27, 0, 2, 5, 20, 19, 1, 16, 27701016, "image", bias=True, stats=2),
    C("image3-small", 27, 0, 1, 2, 3, 5, 1, 8, 27701016, "image", out_pad=4),
    # one volume of ONE plane (NV D3 == 1): both depth taps fall outside, the plane ring and the depth loaders read nothing around it
    C("image3-plane", 27, 0, 1, 1, 20, 19, 1, 16, 27701016, "image", bias=True, stats=1),
    C("rw16-plane", 27, 3, 1, 1, 16, 32, 16, 16, 9450016, "mfma3", bias=True, stats=1),
    C("fl-14-32-32-plane", 27, 3, 1, 1, 14, 14, 32, 32, 9291032, "mfma3", res=True, stats=1),
    # conv3d_rw16_kernel: 16 -> 16, H and W multiples of 16; the segment length falls to 2 on a small volume: D3 = 5 leaves a ragged one
    C("rw16", 27, 3, 1, 5, 16, 32, 16, 16, 9450016, "mfma3", bias=True, stats=1),
    C("rw16-nv2", 27, 3, 2, 3, 32, 16, 16, 16, 9450016, "mfma3", in_pad=4, out_pad=4),
    # conv3d_fl.hip: whatever fl_cost picks at the V-Net plane widths (asserted as the query reports it)
    C("fl-56-32-32-d4", 27, 3, 1, 4, 56, 56, 32, 32, 9291032, "mfma3", bias=True, stats=1),
    C("fl-56-32-32-d8", 27, 3, 1, 8, 56, 56, 32, 32, 9292032, "mfma3", res=True),
    C("fl-56-32-32-d16", 27, 3, 2, 8, 56, 56, 32, 32, 9294032, "mfma3", kinds=TWO),
    C("fl-56-32-64-d16", 27, 3, 1, 16, 56, 56, 32, 64, 9274064, "mfma3", bias=True, kinds=TWO),
    C("fl-28-64-64-d16", 27, 3, 2, 8, 28, 28, 64, 64, 9292032, "mfma3", bias=True, res=True),
    C("fl-28-64-64-d32", 27, 3, 1, 32, 28, 28, 64, 64, 9292064, "mfma3", kinds=TWO),
    C("fl-14-32-64-d4", 27, 3, 1, 4, 14, 14, 32, 64, 9291032, "mfma3", in_pad=4, in_off=4, out_pad=4, res=True, res_pad=4),
    C("fl-7-64-32-d4", 27, 3, 2, 2, 7, 7, 64, 32, 9291032, "mfma3", bias=True, stats=2),
    # ... and with more tiles than workgroups: 600, 520 tiles on 256 CUs
    C("fl-7-64-64-d300", 27, 3, 2, 150, 7, 7, 64, 64, 9291032, "mfma3", bias=True, res=True, stats=2),
    C("fl-7-32-64-d520", 27, 3, 1, 520, 7, 7, 32, 64, 9291064, "mfma3", out_pad=4),
    C("fl-28-32-32-d40", 27, 3, 1, 40, 28, 28, 32, 32, 9293032, "mfma3", bias=True),
    C("fl-14-32-64-d150", 27, 3, 1, 150, 14, 14, 32, 64, 9274064, "mfma3", res=True),
    C("rw16-rounds", 27, 3, 1, 37, 64, 64, 16, 16, 9450016, "mfma3", bias=True, stats=1),
    C("image3-rounds", 27, 0, 1, 33, 128, 120, 1, 16, 27701016, "image", bias=True, kinds=TWO),
]
# dispatch_spatial<3> (W a multiple of 16) and dispatch_flat3 (ids + 5e5; W + 2 <= 63 and no multiple of 16): every tile, both modes, with
# arco_conv3d_fl_set(0).  K = 16 -> 16 with H, W multiples of 16 would go to conv3d_rw16_kernel in mma 3: the 16-wide tiles use N = 4 / 12.
CASES_3D += (
    _modes("v128x16", 27, 1, 3, 20, 16, 16, 4, 9128016, fl0=True, bias=True, out_pad=4)
    + _modes("v128x32", 27, 1, 8, 64, 128, 16, 20, 9128032, fl0=True, kinds=TWO)
    + _modes("v64x32", 27, 1, 3, 6, 16, 20, 19, 9064032, fl0=True, bias=True, res=True, out_pad=1)
    + _modes("v128x64", 27, 1, 8, 64, 128, 16, 64, 9128064, fl0=True, kinds=TWO)
    + _modes("v64x64", 27, 1, 4, 64, 128, 16, 64, 9064064, fl0=True, bias=True, kinds=TWO)
    + _modes("v64x32w", 27, 1, 2, 64, 128, 16, 64, 9064032, fl0=True, res=True)
    + _modes("v32x32", 27, 2, 2, 5, 16, 20, 48, 9032032, fl0=True, bias=True, in_pad=4, in_off=4)
    + _modes("f128x16", 27, 1, 3, 9, 14, 16, 12, 9628016, fl0=True, bias=True, res=True, res_pad=4)
    + _modes("f128x32", 27, 2, 32, 32, 30, 16, 32, 9628032, fl0=True, kinds=TWO)
    + _modes("f64x32", 27, 1, 3, 7, 7, 32, 19, 9564032, fl0=True, bias=True, out_pad=5)
    + _modes("f128x64", 27, 2, 32, 32, 30, 16, 64, 9628064, fl0=True, kinds=TWO)
    + _modes("f64x64", 27, 1, 32, 32, 30, 16, 64, 9564064, fl0=True, kinds=TWO)
    + _modes("f64x32w", 27, 1, 16, 32, 30, 16, 64, 9564032, fl0=True, bias=True)
    + _modes("f32x32", 27, 1, 2, 5, 6, 20, 48, 9532032, fl0=True, res=True)
    + _modes("v64x32-plane", 27, 1, 1, 6, 16, 20, 19, 9064032, fl0=True, bias=True)
    + _modes("f64x32-plane", 27, 1, 1, 7, 7, 32, 19, 9564032, fl0=True, res=True))

CASES = CASES_1X1 + CASES_3X3 + CASES_3D
NAMES = [c["name"] for c in CASES]
assert len(set(NAMES)) == len(NAMES)
FAMILY = {1: "1x1", 9: "3x3", 27: "3x3x3"}
# the data gradient runs the same kernels on a mode-1 pack: one case per family (dY has N channels, dX K)
DGRAD = [C("dgrad-1x1", 1, 3, 1, 1, 5, 41, 80, 48, 1032064, "mfma3"),
         C("dgrad-3x3-halo", 9, 0, 2, 1, 20, 37, 16, 16, 9916016, "mfma0"),
         C("dgrad-3x3-sp", 9, 3, 1, 1, 16, 16, 48, 16, 9304016, "mfma3"),
         C("dgrad-3x3x3-fl", 27, 3, 1, 4, 14, 14, 64, 32, 9291032, "mfma3")]


def by_name(name):
    return CASES[NAMES.index(name)]


# ======================================================================================================================================
# the float64 convolution of rows
# ======================================================================================================================================
def conv64(x, w, c):
    """x [M, K], w [N, K, taps] (torch tap order) float64 -> [M, N]: cross-correlation with zero padding 1, as nn.Conv2d / nn.Conv3d"""
    K, N, T = x.shape[1], w.shape[0], c["taps"]
    if T == 1:
        return x @ w[:, :, 0].t()
    if T == 9:
        xi = x.view(c["nv"] * c["d3"], c["h"], c["w"], K).permute(0, 3, 1, 2)
        return F.conv2d(xi, w.view(N, K, 3, 3), padding=1).permute(0, 2, 3, 1).reshape(-1, N)
    xi = x.view(c["nv"], c["d3"], c["h"], c["w"], K).permute(0, 4, 1, 2, 3)
    return F.conv3d(xi, w.view(N, K, 3, 3, 3), padding=1).permute(0, 2, 3, 4, 1).reshape(-1, N)


def finish(c, d):
    """adds the float64 reference and S to the inputs x, w, bias, res (fp32 tensors or None)"""
    x, w = d["x"].double(), d["w"].double()
    ref = conv64(x, w, c)
    d["sxw"] = conv64(x.abs(), w.abs(), c) if d.get("kind") not in ("impulse", "select") else ref.abs()      # (one product per output)
    s = d["sxw"].clone()
    for t in (d["bias"], d["res"]):
        if t is not None:
            ref = ref + t.double()
            s = s + t.double().abs()
    d["ref"], d["S"] = ref, s
    return d


def _wide_values(shape, g, decades, zeros):
    v = torch.randn(shape, generator=g, dtype=torch.float64) * 10.0 ** ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * decades)
    v[torch.rand(shape, generator=g) < zeros] = 0.0
    return v.float()


def wide_channels(c):
    """the channels that hold 9-bit values in the fixed kind: as many as the 2^24 budget allows (287^2 per product), spread over K"""
    nw = max(1, min(c["k"], 2 ** 23 // (c["taps"] * 287 * 287)))
    return sorted(set((np.arange(nw) * c["k"]) // nw + (c["k"] // nw) // 2))


QX, QW = 2.0 ** -3, 2.0 ** -5                       # the fixed kind: x in units of 2^-3, w of 2^-5, outputs of QUANT = 2^-8
QUANT = QX * QW


def _ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _wide_ints(shape, g):
    return (257 + 2 * _ints(shape, g, 0, 15)) * (2 * _ints(shape, g, 0, 1) - 1)


@functools.lru_cache(maxsize=2)
def _data(name, kind, p, dgrad):
    c = (DGRAD[[d["name"] for d in DGRAD].index(name)] if dgrad else by_name(name))
    g = gen(sum(map(ord, name)), ALL.index(kind) if kind in ALL else 7, p)
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    bias = res = None
    if kind == "fixed":
        xi, wi = _ints((M, K), g, -3, 3), _ints((N, K, T), g, -3, 3)
        for ch in wide_channels(c):
            xi[:, ch] = _wide_ints((M,), g)
            wi[:, ch, :] = _wide_ints((N, T), g)
        x, w = xi.float() * QX, wi.float() * QW
        if c["bias"]:
            bias = _ints((N,), g, -2 ** 18, 2 ** 18).float() * QUANT
        if c["res"]:
            res = _ints((M, N), g, -2 ** 18, 2 ** 18).float() * QUANT
    elif kind == "stats":                             # the fixed kind shrunk: sum y^2 per channel below 2^24 quanta
        px = min(0.5, (8.0 / (T * K)) ** 0.25)
        xi = _ints((M, K), g, -1, 1) * (torch.rand((M, K), generator=g) < 2 * px)
        wi = _ints((N, K, T), g, -1, 1) * (torch.rand((N, K, T), generator=g) < 2 * px)
        x, w = xi.float() * QX, wi.float() * QW
        if c["bias"]:
            bias = _ints((N,), g, -1, 1).float() * QUANT
    elif kind == "impulse":
        x = torch.zeros((M, K))
        pos = impulse_positions(c)
        for i, m in enumerate(pos):
            x[m, i % K] = 1.0
        w = _wide_values((N, K, T), g, 2, 0.0)
    elif kind == "select":
        x = _wide_values((M, K), g, 3, 0.2)
        w = torch.zeros((N, K, T))
        for n in range(N):
            w[n, (7 * n + 3 + p) % K, (n + p * N) % T] = (-1.0) ** n * 2.0 ** ((n + p) % 7 - 3)
    else:
        x = _wide_values((M, K), g, 3, 0.2)
        w = (_wide_values((N, K, T), g, 2, 0.0).double() / math.sqrt(K * T)).float()
        if c["bias"]:
            bias = _wide_values((N,), g, 1, 0.0)
        if c["res"]:
            res = _wide_values((M, N), g, 3, 0.2)
    return finish(c, dict(x=x, w=w, bias=bias, res=res, kind=kind, p=p))


def data(c, kind, p=0, dgrad=False):
    """the inputs, the float64 reference and S of one case and kind (pass p of the select kind); computed once, never modified"""
    return _data(c["name"], kind, p, dgrad)


def forward_weight(d):
    """data gradient: the forward layer's weight W [cout = K, cin = N, taps] whose mode-1 pack (flipped, transposed) is d["w"]"""
    return d["w"].flip(2).permute(1, 0, 2).contiguous()


def dgrad_autograd(c, d):
    """float64 autograd of F.conv2d / F.conv3d (conv64) with respect to its input, for the upstream gradient d["x"]"""
    x = torch.zeros((c["M"], c["n"]), dtype=torch.float64, requires_grad=True)
    y = conv64(x, forward_weight(d).double(), c)
    return torch.autograd.grad(y, x, d["x"].double())[0]


def select_passes(c):
    return -(-c["taps"] // c["n"])


def _axis(size, step):
    a = list(range(0, size, step))
    if a[-1] != size - 1 and len(a) > 1:
        a[-1] = size - 1                              # (moves the last one away from its neighbour: the far border is always used)
    elif a[-1] != size - 1 and size - 1 >= step:
        a.append(size - 1)
    return a


def impulse_positions(c):
    """rows of the impulses: a grid more than the kernel extent apart in every axis the kernel spans, first and last position included,
    the list thinned evenly to at most max(K, 16) entries"""
    if c["taps"] == 1:
        rows = _axis(c["M"], 2)
    else:
        zs = _axis(c["d3"], 4) if c["taps"] == 27 else list(range(c["d3"]))
        rows = [((v * c["d3"] + z) * c["h"] + y) * c["w"] + x for v in range(c["nv"]) for z in zs for y in _axis(c["h"], 4)
                for x in _axis(c["w"], 4)]
    want = max(c["k"], 16)                            # (fewer than 16 channels: they take the impulses in turn)
    if len(rows) > want:
        rows = [rows[(i * (len(rows) - 1)) // (want - 1)] for i in range(want)]
    return rows


# ======================================================================================================================================
# bounds
# ======================================================================================================================================
def n_roundings(c):
    K, T = c["k"], c["taps"]
    return {"nout": 5 + int(math.log2(max(1, K // 4))), "nin": K + 1, "image": 2 * T * K, "mfma0": 2 * T * K + 2, "mfma3": 6 * T * K + 2}[c["fam"]]


def tol_wide(c, d):
    t = gamma(n_roundings(c)) * d["S"] + U * d["ref"].abs()
    if c["fam"] == "mfma3":
        t = t + DROP * d["sxw"]
    return t


def held(name, got, c, d):
    """the two ratios of the wide kind: err / derived bound, err / (3e-6 S); both printed, both must be <= 1"""
    r1, r2 = worst(got, d["ref"], tol_wide(c, d)), worst(got, d["ref"], MEASURED * d["S"])
    print(f"{name}: worst err / bound {r1:.4f}, err / (3e-6 S) {r2:.3f}")
    return r1, r2


def representable(t):
    return bool((t.float().double() == t).all())


def equal_bits(got, ref):
    """the exact kinds: the float64 reference is representable in fp32 (asserted) and the kernel's output equals it, torch.equal"""
    assert representable(ref), "the reference is not exactly representable in fp32"
    got = got.detach().cpu()
    return got.shape == ref.shape and torch.equal(got, ref.float())


# ---- BatchNorm partial sums of the epilogues ------------------------------------------------------------------------------------------
def stat_totals(c, y, groups):
    """float64 per-group, per-channel sum y and sum y^2 of rows y [M, N]: group g owns the volumes [g nv / G, (g + 1) nv / G)"""
    yg = y.double().view(groups, c["M"] // groups, -1)
    return yg.sum(1), (yg * yg).sum(1)


def slab_sums(slabs, nmb, groups):
    """slabs [N, nmb] -> [groups, N] float64 host sums: group g owns the slabs [g nmb / G, (g + 1) nmb / G)"""
    return slabs.double().view(-1, groups, nmb // groups).sum(2).t()


def stats_exact(c, ssum, ssq, nmb, groups, y):
    """the stats kind: every slab an integer number of quanta, every group's slab range equal to its own volumes' totals"""
    if nmb % groups or ssum.shape != (c["n"], nmb) or ssq.shape != (c["n"], nmb):
        return False
    q1, q2 = ssum.double() / QUANT, ssq.double() / (QUANT * QUANT)
    if not (bool((q1 == q1.round()).all()) and bool((q2 == q2.round()).all())):
        return False
    t1, t2 = stat_totals(c, y, groups)
    return torch.equal(slab_sums(ssum, nmb, groups), t1) and torch.equal(slab_sums(ssq, nmb, groups), t2)


def stats_tol(c, d, groups):
    """wide kind: |sum over slabs - sum ref| <= sum tol_y + gamma(Mg) sum(|ref| + tol_y): every output off by at most its own bound, the fp32
    partial sums of at most Mg = M / G values in any order; the squares with |y^2 - ref^2| <= tol (2 |ref| + tol) and one more rounding"""
    t = tol_wide(c, d)
    a = d["ref"].abs()
    gm = gamma(c["M"] // groups + 1)
    g = lambda v: v.view(groups, c["M"] // groups, -1).sum(1)
    e2 = t * (2 * a + t)
    return g(t) + gm * g(a + t), g(e2) + gm * g(a * a + e2)


# ======================================================================================================================================
# the two split rules (split_bf16.h: the activation split; igemm.hip store_split3: the all-round-to-nearest weight pack) and the fp32 emulation of the wide kind
# ======================================================================================================================================
def bf16_rne(v):
    """float32 array -> the nearest bf16 value (ties to even), as float32"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def bf16_trunc(v):
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split_weight(w):
    """store_split3: three round-to-nearest terms"""
    w = np.asarray(w, dtype=np.float32)
    b0 = bf16_rne(w); r1 = (w - b0).astype(np.float32)
    b1 = bf16_rne(r1); r2 = (r1 - b1).astype(np.float32)
    return b0, b1, bf16_rne(r2)


def split_act(x):
    """split3_pair_rt: nearest, truncated, the exact rest"""
    x = np.asarray(x, dtype=np.float32)
    t0 = bf16_rne(x); r1 = (x - t0).astype(np.float32)
    t1 = bf16_trunc(r1)
    return t0, t1, (r1 - t1).astype(np.float32)


def n_terms(parts):
    return sum((p != 0).astype(np.int64) for p in parts)


def im2col(x, c):
    """rows [M, K] -> [M, taps, K] float32: the zero-padded neighbourhood of every output position, torch tap order"""
    K, T = x.shape[1], c["taps"]
    if T == 1:
        return x.view(-1, 1, K)
    dims = (c["nv"], c["d3"], c["h"], c["w"]) if T == 27 else (c["nv"] * c["d3"], 1, c["h"], c["w"])
    v = x.view(*dims, K)
    pz = 1 if T == 27 else 0
    vp = F.pad(v, (0, 0, 1, 1, 1, 1, pz, pz))
    out = [vp[:, dz:dz + dims[1], dy:dy + dims[2], dx:dx + dims[3]] for dz in range(2 * pz + 1) for dy in range(3) for dx in range(3)]
    return torch.stack(out, dim=4).reshape(-1, T, K)


def emulate(c, d):
    """the wide kind in fp32, one fixed order: mfma3 - both operands split, per (tap, k) the six kept products (exact: 16 bits) added
    to an fp32 accumulator small terms first; mfma0 / image / nin - the rounded product, then the rounded sum (or an fma); bias and
    residual in the epilogue.  nout: the fmaf chain and the butterfly."""
    f32 = np.float32
    cols_ = im2col(d["x"], c).numpy()                                      # [M, T, K]
    w = d["w"].permute(0, 2, 1).contiguous().numpy()                       # [N, T, K]
    M, T, K = cols_.shape
    N = w.shape[0]
    acc = np.zeros((M, N), dtype=f32)
    fam = c["fam"]
    if fam == "nout":
        Q = K // 4
        parts = []
        for q in range(Q):
            p = None
            for e in range(4):
                xv, wv = cols_[:, 0, 4 * q + e].astype(np.float64)[:, None], w[:, 0, 4 * q + e].astype(np.float64)[None, :]
                p = (xv * wv).astype(f32) if p is None else (xv * wv + p.astype(np.float64)).astype(f32)
            parts.append(p)
        off = 1
        while off < Q:
            parts = [(parts[q] + parts[q ^ off]).astype(f32) for q in range(Q)]
            off <<= 1
        acc = parts[0]
        if d["bias"] is not None:
            acc = (acc + d["bias"].numpy()[None, :]).astype(f32)
        return torch.from_numpy(acc)
    if fam in ("image", "nin") and d["bias"] is not None:
        acc = acc + d["bias"].numpy()[None, :]
    if fam == "mfma3":
        xs, ws = split_act(cols_), split_weight(w)
        order = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))          # (activation term, weight term); (1,2), (2,1), (2,2) dropped
    for t in range(T):
        for k in range(K):
            if fam == "mfma3":
                for i, j in order:
                    p = xs[i][:, t, k].astype(np.float64)[:, None] * ws[j][:, t, k].astype(np.float64)[None, :]
                    acc = (acc.astype(np.float64) + p).astype(f32)
            elif fam in ("image", "nin"):
                acc = (cols_[:, t, k].astype(np.float64)[:, None] * w[:, t, k].astype(np.float64)[None, :] + acc.astype(np.float64)).astype(f32)
            else:
                p = (cols_[:, t, k][:, None] * w[:, t, k][None, :]).astype(f32)
                acc = (acc + p).astype(f32)
    if fam not in ("image", "nin") and d["bias"] is not None:
        acc = (acc + d["bias"].numpy()[None, :]).astype(f32)
    if d["res"] is not None:
        acc = (acc + d["res"].numpy()).astype(f32)
    return torch.from_numpy(acc)


# ======================================================================================================================================
# the packed weight layouts (include/arco_hip.h, csrc/igemm.hip) restated in numpy
# ======================================================================================================================================
def ceil_to(v, m):
    return (v + m - 1) // m * m


def pack_logical(W, cout, cin, taps, mode):
    """[taps][N][K] float32 of the logical operand: mode & 1 = the data-gradient form (flipped taps, transposed)"""
    W = np.asarray(W, dtype=np.float32).reshape(cout, cin, taps)
    if mode & 1:
        return np.ascontiguousarray(W[:, :, ::-1].transpose(2, 1, 0))       # [tap][ci][co] = W[co][ci][T-1-tap]
    return np.ascontiguousarray(W.transpose(2, 0, 1))


def pack_gather_logical(src, n2, k2, g, gm, mode):
    """mode >> 3 = gm: the GEMM form W2 [n2][k2] of a k2 s2 (transposed) convolution gathered from the torch layout"""
    src = np.asarray(src, dtype=np.float32).reshape(-1)
    a, b = np.meshgrid(np.arange(n2), np.arange(k2), indexing="ij")
    if gm == 1:
        W2 = src[(a * g + b % g) * 8 + b // g]
    elif gm == 2:
        W2 = src[(b * g + a % g) * 8 + a // g]
    else:
        W2 = src[b % g]
    return np.ascontiguousarray(W2.T if mode & 1 else W2)[None]


def pack_expected(logical, mode, npad, kpad):
    """the packed buffer as integers: plain fp32 [T][npad][kpad] (int32 view), f16 (int16 view) or the split format (int16 view:
    element (tap, n, k) -> ((tap npad + n) kpad / 16 + k / 16) * 48 + plane * 16 + k % 16); pad entries zero"""
    T, N, K = logical.shape
    full = np.zeros((T, npad, kpad), dtype=np.float32)
    full[:, :N, :K] = logical
    if mode & 4:
        return full.astype(np.float16).view(np.int16)
    if mode & 2:
        parts = split_weight(full)
        out = np.zeros((T, npad, kpad // 16, 3, 16), dtype=np.int16)
        for p in range(3):
            out[:, :, :, p, :] = (parts[p].view(np.uint32) >> 16).astype(np.uint16).view(np.int16).reshape(T, npad, kpad // 16, 16)
        return out.reshape(T, npad, -1)
    return full.view(np.int32)
