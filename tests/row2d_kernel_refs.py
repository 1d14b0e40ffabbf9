"""Case tables, inputs, float64 references and bounds shared by tests/test_row2d_kernels_gpu.py (the 2-D row-sparse head kernels
arco_gather_upcat_rows(_h) / arco_lerp4_cat_rows(_h) and the small step utilities arco_zero_rows(_h), arco_cast_rows_f2h,
arco_fold_residual, arco_unfold_residual, arco_combine_terms(_bwd) of csrc/elementwise.hip, one entry point at a time) and
tests/test_row2d_kernels_cpu.py (the same bounds held against an fp32 emulation, the input conditions, planted errors).  A sibling of
tests/side_kernel_refs.py, whose align_corners restatement (ac_axis32 / ac_axis_exact / corners), forward bound (blend_tol) and
buffer helpers it uses.  Plain CPU torch / numpy only; every case is seeded, computed once (functools.lru_cache) and never modified.
u = 2^-24."""
import functools
import math

import numpy as np
import torch

import side_kernel_refs as R
from loss_kernel_refs import TINY, U, gen
from side_kernel_refs import NV, RATIOS_2D, corners, blend_tol, interp64, rand

F32 = np.float32


# ======================================================================================================================================
# (1) arco_gather_upcat_rows(_h), arco_lerp4_cat_rows(_h)
# ======================================================================================================================================
# X[j][:Clo] = the align_corners bilinear sample of lo at pixel pix[j] of the hi grid, X[j][Clo:] = hi[pix[j]].
#   * lo part, per element, against F.interpolate(mode="bilinear", align_corners=True) in float64: side_kernel_refs.blend_tol - the
#     coordinate term (two roundings of the source coordinate times the local slope) plus K_BLEND u max|corner| (derived there for
#     the three-level blend; the two-level blend hy (hx v00 + lx v01) + ly (hx v10 + lx v11) makes at most six roundings on the value's
#     way out - three products and a sum per level, or fewer where the compiler fuses - plus 1 - l twice: inside k = 8);
#   * bit for bit the rows of the dense arco_bilinear_fwd (same index arithmetic, same expression);
#   * arco_lerp4_cat_rows, given the four neighbour rows and (ly, lx) of arco_up_neighbors, bit for bit the gather;
#   * hi part exact: an fp32 copy, or an f16 value widened.
#                 ratio Clo  Chi n    pad off     pad: ld = C + pad on every operand; off: the operand starts `off` channels into its buffer
ROW2D_CASES = [(0, 4, 4, 132, 0, 0), (0, 260, 8, 133, 8, 4), (1, 12, 0, 135, 8, 4), (2, 12, 4, 134, 8, 0), (3, 4, 12, 132, 0, 0),
               (4, 4, 4, 135, 8, 4), (5, 12, 4, 132, 8, 4), (6, 4, 4, 133, 0, 0), (1, 0, 8, 134, 8, 0), (2, 260, 0, 135, 0, 0),
               (1, 12, 8, 1, 8, 4), (0, 4, 4, 2, 0, 0)]


def border_pixels(hi):
    H, W = hi
    return [y * W + x for y in range(H) for x in range(W) if y in (0, H - 1) or x in (0, W - 1)]


def sample_pix2d(seed, nv, hi, n):
    """n sampled pixel ids of an [nv, H, W] map: EVERY border pixel of every image, one pixel 64 times, the rest random (with
    replacement), shuffled; n = 1: the last pixel of the last image; n = 2: the first and the last pixel"""
    g = gen(91, seed)
    vol = hi[0] * hi[1]
    tot = nv * vol
    if n <= 2:
        return torch.tensor([tot - 1] if n == 1 else [0, tot - 1], dtype=torch.int64)
    fixed = [img * vol + p for img in range(nv) for p in border_pixels(hi)]
    fixed += [int(torch.randint(0, tot, (1,), generator=g))] * 64
    assert n >= len(fixed), (n, len(fixed))
    rest = torch.randint(0, tot, (n - len(fixed),), generator=g).tolist()
    pix = torch.tensor(fixed + rest, dtype=torch.int64)
    return pix[torch.randperm(n, generator=g)].contiguous()


@functools.lru_cache(maxsize=None)
def row2d_case(i):
    r, Clo, Chi, n, pad, off = ROW2D_CASES[i]
    lo, hi = RATIOS_2D[r]
    g = gen(30, i)
    LO = rand(g, (NV, *lo, max(Clo, 1)))[..., :Clo].contiguous()
    HI = rand(g, (NV, *hi, max(Chi, 1)))[..., :Chi].contiguous()
    HI16 = HI.half()
    pix = sample_pix2d(400 + i, NV, hi, n)
    cn = corners(pix, lo, hi)
    vhi, vlo = hi[0] * hi[1], lo[0] * lo[1]
    if Clo:
        ref_lo = interp64(LO, hi).view(NV * vhi, Clo)[pix]
        tol_lo = blend_tol(LO, lo, hi).view(NV * vhi, Clo)[pix]
    else:
        ref_lo, tol_lo = torch.zeros((n, 0), dtype=torch.float64), torch.zeros((n, 0), dtype=torch.float64)
    idx4 = torch.from_numpy(cn["idx"])                                                            # [n, 4]: 00, 01, 10, 11
    LO2 = LO.view(NV * vlo, Clo)
    lylx = torch.from_numpy(np.stack([cn["ax"][a][2] for a in range(2)], 1).reshape(-1).copy())
    return dict(lo=lo, hi=hi, Clo=Clo, Chi=Chi, n=n, pad=pad, off=off, LO=LO, HI=HI, HI16=HI16, pix=pix, cn=cn, ref_lo=ref_lo, tol_lo=tol_lo,
                hi_rows=HI.view(NV * vhi, Chi)[pix], hi16_rows=HI16.view(NV * vhi, Chi)[pix].float(), idx4=idx4.reshape(-1).contiguous(),
                V=LO2[idx4.reshape(-1)].contiguous(), LO2=LO2, HI2=HI.view(NV * vhi, Chi), HI162=HI16.view(NV * vhi, Chi), lylx=lylx)


def emu_rows2d(c, fused):
    """the kernels' expression hy (hx v00 + lx v01) + ly (hx v10 + lx v11) in fp32 with the restatement's weights; fused: every sum of
    a product contracted into an fma (what the compiler may do), else every operation rounded"""
    n, Clo, ax = c["n"], c["Clo"], c["cn"]["ax"]
    v = [c["V"].view(n, 4, Clo)[:, k] for k in range(4)]
    t = lambda a, k: torch.from_numpy(np.ascontiguousarray(ax[k][a])).view(n, 1)
    ly, hy, lx, hx = t(2, 0), t(3, 0), t(2, 1), t(3, 1)
    if fused:
        a, b = R._fma32(lx, v[1], hx * v[0]), R._fma32(lx, v[3], hx * v[2])
        return R._fma32(ly, b, hy * a)
    return hy * (hx * v[0] + lx * v[1]) + ly * (hx * v[2] + lx * v[3])


# ======================================================================================================================================
# (2) arco_zero_rows(_h), arco_cast_rows_f2h                                                         exact
# ======================================================================================================================================
#              M  C    pad n                    n = 0 / 1; duplicates; the last: n C / 4 = 4096 * 256 + 1 work items over 5 rows
UTIL_CASES = [(9, 4, 4, 0), (9, 12, 8, 1), (7, 260, 4, 11), (33, 12, 0, 40), (5, 4, 4, 4096 * 256 + 1)]
CAST_SCALES = (1.0, 1024.0, 65536.0)


@functools.lru_cache(maxsize=None)
def util_idx(i):
    """row indices with duplicates that leave at least one row unnamed; the big case cycles over four of its five rows"""
    M, C, pad, n = UTIL_CASES[i]
    g = gen(31, i)
    if n > 1000:
        return (torch.arange(n, dtype=torch.int64) % 4 + 1).contiguous()
    idx = torch.randint(0, M - 1, (n,), generator=g)
    if n >= 4:
        idx[1] = idx[0]
        idx[n - 1] = idx[0]
    return idx.contiguous()


@functools.lru_cache(maxsize=None)
def zero_case(i, half):
    M, C, pad, n = UTIL_CASES[i]
    X = rand(gen(32, i), (M, C)) + 3.0
    X = X.half() if half else X
    ref = X.clone()
    idx = util_idx(i)
    ref[idx] = 0
    return dict(M=M, C=C, ld=C + pad, n=n, X=X, idx=idx, ref=ref)


def cast_specials(scale):
    """inputs whose product with `scale` (a power of two: exact) is: an f16 subnormal, the tie 2^-25 between 0 and the smallest
    subnormal (to even: 0), 3 2^-25 (to even: 2^-23), below half the smallest subnormal, round-to-nearest-even ties of normals
    (1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9, 2049 -> 2048, 2051 -> 2052), exactly 65504, 65519.996 (still rounds to 65504 after the
    clamp), 65520, 1e6, +-inf, NaN, -0.0, a normal fp32 whose product overflows fp32 (3e38 at the larger scales)"""
    s = scale
    return torch.tensor([3e-6 / s, -5.9e-8 / s, 2.0 ** -25 / s, 3 * 2.0 ** -25 / s, -(2.0 ** -26) / s, (1 + 2.0 ** -11) / s,
                         (1 + 3 * 2.0 ** -11) / s, 2049.0 / s, -2051.0 / s, 65504.0 / s, -65504.0 / s, 65519.996 / s, 65520.0 / s, 1e6 / s,
                         -1e6 / s, math.inf, -math.inf, math.nan, -0.0, 3e38, -3e38, 6.1e-5 / s, 1.0 / s, 33.3337 / s], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def cast_case(i, scale):
    """(x * scale) clamped to +-65504, then rounded to f16 - the CPU's arithmetic; rows that no index names keep the sentinel"""
    M, C, pad, n = UTIL_CASES[i]
    spec = cast_specials(scale)
    X = rand(gen(33, i), (M, C)) * 40.0 / scale
    k = torch.arange(M * C).view(M, C)
    X = torch.where(k % 3 == 0, spec[(k // 3) % spec.numel()], X)
    idx = util_idx(i)
    named = torch.zeros(M, dtype=torch.bool)
    named[idx] = True
    val = (X * torch.tensor(scale, dtype=torch.float32)).clamp(-65504.0, 65504.0).half()
    ref = torch.where(named.view(M, 1), val, torch.tensor(R.SENTINEL, dtype=torch.float16))
    return dict(M=M, C=C, lds=C + pad, ldd=C + 8 - pad, n=n, X=X, idx=idx, ref=ref, named=named, scale=scale)


# ======================================================================================================================================
# (3) arco_fold_residual / arco_unfold_residual                                                      exact
# ======================================================================================================================================
#             n     c         1025 x 1025 = 4096 * 256 + 2049 elements: past the grid cap
FOLD_CASES = [(2, 1), (3, 1), (3, 2), (17, 1), (17, 16), (1025, 1), (1025, 1024)]


@functools.lru_cache(maxsize=None)
def fold_case(i):
    """W' = W + I (one fp32 addition on the diagonal, the CPU's) as its column blocks lo [n, c], hi [n, n - c]; the reverse takes
    gradient blocks back to [n, n], a null block reading as zeros"""
    n, c = FOLD_CASES[i]
    g = gen(34, i)
    W = rand(g, (n, n))
    Wp = W + torch.eye(n)
    dlo, dhi = rand(g, (n, c)), rand(g, (n, n - c))
    return dict(n=n, c=c, W=W, lo=Wp[:, :c].contiguous(), hi=Wp[:, c:].contiguous(), dlo=dlo, dhi=dhi,
                dW=torch.cat((dlo, dhi), 1), dW_nolo=torch.cat((torch.zeros_like(dlo), dhi), 1),
                dW_nohi=torch.cat((dlo, torch.zeros_like(dhi)), 1))


# ======================================================================================================================================
# (4) arco_combine_terms (+ _bwd)                                                                     bounded / exact
# ======================================================================================================================================
# out = sum_i w_i t_i accumulated in order from 0: n products and n sums (the first onto 0: exact), any of them fused or not - within
# (n + 1) u sum|w_i t_i| of the float64 sum of the same fp32 w_i and t_i.  Backward: grads[i] = w_i g, one IEEE multiplication.
COMBINE_N = (1, 2, 3, 4, 5, 6, 7, 8)


@functools.lru_cache(maxsize=None)
def combine_case(n):
    """mixed signs; from n = 2 on a cancelling pair (w_0 t_0 = -w_1 t_1 exactly)"""
    g = gen(35, n)
    t = rand(g, (n,))
    w = torch.tensor([1.0, 0.5, 0.1, 1.0, 0.3, 2.0, 0.01, 0.7][:n]) * torch.tensor([1, 1, -1, 1, -1, 1, 1, -1][:n])
    if n >= 2:
        t[1] = -2.0 * t[0]                                                                      # w_0 t_0 + w_1 t_1 = t_0 - t_0 = 0
    prod = w.double() * t.double()
    gr = rand(g, (1,))
    return dict(n=n, t=t, w=w, ref=prod.sum().view(1), tol=((n + 1) * U * prod.abs().sum() + TINY).view(1), g=gr, grads=w * gr,
                grads64=w.double() * gr.double())


def emu_combine(c, fused):
    s = torch.zeros(())
    for i in range(c["n"]):
        s = R._fma32(c["w"][i], c["t"][i], s) if fused else s + c["w"][i] * c["t"][i]
    return s.view(1)
