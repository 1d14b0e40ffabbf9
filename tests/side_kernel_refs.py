"""Case tables, inputs, float64 / int64 references and per-element bounds shared by tests/test_side_kernels_gpu.py (the 3-D side
kernels of csrc/elementwise.hip, the 2-D adjoints, the layout and optimiser kernels, all of csrc/det_scatter.hip and the two casts
of csrc/conv_h.hip, one entry point at a time) and tests/test_side_kernels_cpu.py (the same bounds held against an fp32 emulation,
the input conditions, planted errors, the host-side rejections).  Plain CPU torch / numpy only; the comparison helpers at the end
take the GPU file's device buffers and the CPU file's host buffers alike.

Every case is seeded, computed once (functools.lru_cache) and never modified.  Every reference is float64 / int64 computed from the
SAME fp32 (or f16) values the kernel reads.  u = 2^-24; gamma(k) = k u / (1 - k u).

The align_corners index arithmetic (interp.h ac_src) is restated in numpy float32 (ac_axis32: one IEEE division, one
multiplication, a truncation, a subtraction; contraction is off in ac_src) and, separately, in exact integer arithmetic
(ac_axis_exact): the two are compared where the kernels' indices and weights are outputs."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from loss_kernel_refs import ISENT, SENTINEL, TINY, U, exact, gamma, gen

F32 = np.float32


def rand(g, shape):
    return torch.randn(tuple(shape), generator=g)


# ======================================================================================================================================
# (0) align_corners index arithmetic
# ======================================================================================================================================
def ac_axis32(o, I, O):
    """ac_src in numpy float32 for the output indices o: i0, i1, l, 1 - l"""
    o = np.asarray(o, dtype=np.int64)
    s = F32(I - 1) / F32(O - 1) if O > 1 else F32(0)
    src = (s * o.astype(F32)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), I - 1)
    i1 = np.where(i0 < I - 1, i0 + 1, i0)
    l = (src - i0.astype(F32)).astype(F32)
    return i0, i1, l, (F32(1) - l).astype(F32)


def ac_axis_exact(o, I, O):
    """the exact rational coordinate o (I - 1) / (O - 1) (one float64 rounding), and its cell by integer division"""
    o = np.asarray(o, dtype=np.int64)
    num, den = (o * (I - 1), O - 1) if O > 1 else (o * 0, 1)
    i0 = np.minimum(num // den, I - 1)
    return num / den, i0, np.minimum(i0 + 1, I - 1)


# resize ratios, each used by trilinear_fwd / trilinear_bwd and as the (lo, hi) pair of the row kernels
#          (Di, Hi, Wi)   (Do, Ho, Wo)
RATIOS = [((3, 4, 5), (6, 8, 10)),        # exact x2
          ((3, 5, 2), (7, 9, 5)),         # non-integer upsampling
          ((9, 7, 6), (4, 3, 5)),         # downsampling (head.py calls arco_trilinear_bwd outside the x2 case)
          ((5, 4, 3), (5, 4, 3)),         # identity
          ((1, 4, 4), (4, 4, 4)),         # input side 1
          ((4, 4, 4), (1, 4, 4)),         # output side 1
          ((1, 1, 1), (1, 1, 1))]         # everything 1
RATIOS_2D = [((3, 4), (6, 8)), ((3, 5), (7, 9)), ((9, 7), (4, 3)), ((5, 4), (5, 4)), ((1, 4), (4, 4)), ((4, 4), (1, 4)), ((1, 1), (1, 1))]
NV = 2


def sample_pix(seed, nv, dims, n):
    """n sampled voxel ids of an [nv, *dims] map: the first and last voxel of the first and last image, two voxels on every face
    (where i0 clamps), one voxel 64 times, the rest random (with replacement)"""
    g = gen(90, seed)
    vol = int(np.prod(dims))
    tot = nv * vol
    fixed = [0, vol - 1, (nv - 1) * vol, tot - 1]
    for ax in range(len(dims)):
        for side in (0, dims[ax] - 1):
            c = [int(torch.randint(0, d, (1,), generator=g)) for d in dims]
            c[ax] = side
            img = int(torch.randint(0, nv, (1,), generator=g))
            fixed.append(img * vol + int(np.ravel_multi_index(c, dims)))
    rep = int(torch.randint(0, tot, (1,), generator=g))
    fixed += [rep] * 64
    assert n >= len(fixed)
    rest = torch.randint(0, tot, (n - len(fixed),), generator=g).tolist()
    pix = torch.tensor(fixed + rest, dtype=torch.int64)
    return pix[torch.randperm(n, generator=g)].contiguous()


def corners(pix, lo, hi):
    """Every sampled output voxel's corners, 2-D or 3-D, in the kernels' order (z, y, x with x fastest).
    idx [n, 2^d] rows of the channels-last low-resolution tensor, w [n, 2^d] fp32 weights ((wz * wy) * wx, single multiplies),
    ax: per axis (i0, i1, l, h) of the float32 restatement, exact: per axis (coordinate, i0, i1), img."""
    d = len(lo)
    pixn = pix.numpy()
    vol = int(np.prod(hi))
    img = pixn // vol
    co = np.unravel_index(pixn - img * vol, hi)
    ax = [ac_axis32(co[a], lo[a], hi[a]) for a in range(d)]
    ex = [ac_axis_exact(co[a], lo[a], hi[a]) for a in range(d)]
    n = pixn.shape[0]
    idx = np.zeros((n, 2 ** d), dtype=np.int64)
    w = np.zeros((n, 2 ** d), dtype=F32)
    for k in range(2 ** d):
        bits = [(k >> (d - 1 - a)) & 1 for a in range(d)]
        r = img.copy()
        wk = None
        for a in range(d):
            r = r * lo[a] + ax[a][bits[a]]
            wa = ax[a][2] if bits[a] else ax[a][3]
            wk = wa if wk is None else (wk * wa).astype(F32)
        idx[:, k], w[:, k] = r, wk
    return dict(idx=idx, w=w, ax=ax, exact=ex, img=img, d=d, lo=lo, hi=hi)


def corner_property(idx, w, cn):
    """The float64 check on indices and weights (as produced by a kernel): the worst ratios of
      * |sum_k w_k coordinate_k - o (I - 1) / (O - 1)| / (4 S u), per axis, S the largest side.  First-order worst case of the chain:
        2 u (I - 1) from the scale and the product, u / 2 (I - 1) from 1 - l, 3 u (I - 1) from the two weight products and the other
        axes' h + l - 5.5 u (I - 1); the roundings do not line up, and 4 S u is what is held;
      * |sum_k w_k - 1| / (4 u): three roundings of 1 - l (u / 2 each) and two products;
    and whether every index lies inside its image."""
    d, lo, hi = cn["d"], cn["lo"], cn["hi"]
    S = max(max(lo), max(hi))
    idx, w64 = np.asarray(idx, dtype=np.int64), np.asarray(w, dtype=np.float64)
    vol = int(np.prod(lo))
    inside = bool(((idx // vol) == cn["img"][:, None]).all()) and bool((idx >= 0).all())
    co = np.unravel_index(idx % vol, lo)
    r_coord = 0.0
    for a in range(d):
        got = (w64 * co[a]).sum(1)
        r_coord = max(r_coord, float(np.abs(got - cn["exact"][a][0]).max() / (4 * S * U)))
    r_sum = float(np.abs(w64.sum(1) - 1.0).max() / (4 * U))
    return r_coord, r_sum, inside


#                 ratio n     (n % 4 in {0, 1, 3})
CORNER_CASES = [(0, 76), (1, 77), (2, 79), (3, 76), (4, 77), (5, 79), (6, 76)]


@functools.lru_cache(maxsize=None)
def corner_case(i, d):
    r, n = CORNER_CASES[i]
    lo, hi = RATIOS[r] if d == 3 else RATIOS_2D[r]
    pix = sample_pix(100 * d + i, NV, hi, n)
    cn = corners(pix, lo, hi)
    return dict(pix=pix, n=n, lo=lo, hi=hi, cn=cn, idx=torch.from_numpy(cn["idx"].reshape(-1).copy()),
                w=torch.from_numpy(cn["w"].reshape(-1).copy()),
                lylx=torch.from_numpy(np.stack([cn["ax"][a][2] for a in range(d)], 1).reshape(-1).copy()))


# ======================================================================================================================================
# (1) space-to-depth / depth-to-space (+ add)                                                         exact
# ======================================================================================================================================
def pack(V, nv, x2, y2, z2, c):
    """P[q][tap * C + c] = V[(n, 2x + dx, 2y + dy, 2z + dz)][c], tap = dx * 4 + dy * 2 + dz"""
    return V.reshape(nv, x2, 2, y2, 2, z2, 2, c).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(nv * x2 * y2 * z2, 8 * c)


def unpack(P, nv, x2, y2, z2, c):
    return P.reshape(nv, x2, y2, z2, 2, 2, 2, c).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(nv * x2 * y2 * z2 * 8, c)


#            NV X2     Y2 Z2 C(words) padv padp kind     'h': an f16 tensor of 2 C channels moved as C words (ops._s2d3)
S2D_CASES = [(2, 3, 2, 5, 4, 0, 0, "w"), (1, 1, 3, 2, 12, 8, 8, "w"), (2, 2, 1, 3, 4, 8, 0, "w"), (1, 3, 2, 1, 8, 0, 8, "w"),
             (2, 2, 3, 2, 8, 0, 8, "h"), (1, 1, 1, 1, 4, 8, 8, "w"),
             (3, 43691, 1, 1, 4, 0, 0, "w")]       # 3 * 43691 * 8 = 4096 * 256 + 8 work items: the grid-stride loop's second trip


@functools.lru_cache(maxsize=None)
def s2d_case(i):
    """random 32-bit patterns (NaN payloads, -0.0 and infinities among them, four planted in front)"""
    nv, x2, y2, z2, c, padv, padp, kind = S2D_CASES[i]
    rows = nv * x2 * y2 * z2 * 8
    V = torch.randint(-2 ** 31, 2 ** 31, (rows, c), generator=gen(2, i), dtype=torch.int64).to(torch.int32)
    V[0, :4] = torch.tensor([0x7fc12345, -0x3fffff, -2 ** 31, 0x7f800000], dtype=torch.int64).to(torch.int32)
    P = pack(V, nv, x2, y2, z2, c).contiguous()
    return dict(nv=nv, x2=x2, y2=y2, z2=z2, c=c, ldv=c + padv, ldp=8 * c + padp, kind=kind, V=V, P=P, rows=rows)


#            NV X2 Y2 Z2 C  pad
D2S_CASES = [(2, 3, 2, 5, 4, 0), (1, 1, 3, 2, 12, 8), (2, 2, 1, 3, 4, 8), (1, 3, 2, 1, 260, 0), (1, 1, 1, 1, 4, 8), (3, 43691, 1, 1, 4, 0)]


@functools.lru_cache(maxsize=None)
def d2s_case(i, half):
    """fp32: the CPU's single fp32 add; f16: (a.float() + b.float()).half()"""
    nv, x2, y2, z2, c, pad = D2S_CASES[i]
    g = gen(3, i, half)
    q = nv * x2 * y2 * z2
    P, A = rand(g, (q, 8 * c)) * 3, rand(g, (q * 8, c))
    if half:
        P, A = P.half(), A.half()
        ref = (unpack(P, nv, x2, y2, z2, c).float() + A.float()).half()
    else:
        ref = unpack(P, nv, x2, y2, z2, c) + A
    return dict(nv=nv, x2=x2, y2=y2, z2=z2, c=c, pad=pad, P=P, A=A, ref=ref.contiguous(), rows=q * 8)


# ======================================================================================================================================
# (2) trilinear resize, dense                                                                          bounded
# ======================================================================================================================================
# Forward, per output element, against F.interpolate(mode="trilinear", align_corners=True) in float64:
#   * the source coordinate: s = fl((I - 1) / (O - 1)) and src = fl(s o) are two roundings, |src - exact| <= 2 u exact; the blend is
#     continuous and piecewise linear, its slope along an axis is at most the largest difference D_a between the two corners of a
#     pair along that axis: sum_a 2 u coord_a D_a (l = src - i0 is exact).  The issue's starting form bounds coord_a by the side S_a
#     and D_a by 2 max|corner| - 4 u (Sd + Sh + Sw) max|corner| - and sits a factor 20 and more above what any rounding does on random
#     data; the local form here is the same derivation without those two steps;
#   * tl_blend1: three levels of (product, fma) = six roundings on the value's way out, and 1 - l (u / 2, absolute, per level):
#     7.5 u max|corner| since the weights of each level sum to 1: k = 8.
# Corner maximum and corner differences are local: over the eight corners of the float32 cell AND of the exact cell (at an integer
# coordinate the two may differ by one, with a weight of a few u on the far corner).
K_BLEND = 8
COORD = 2.001 * U                                     # |src - exact| <= COORD * exact (two roundings, second order included)


def cell_terms(X, lo, hi):
    """X [nv, *lo, C] -> (cmax, slope), both [nv, *hi, C]: max |corner|, and sum_a COORD coord_a D_a, over the float32 cell and the
    exact cell of every output voxel"""
    d = len(lo)
    a = X.double()
    cmax, D = None, [None] * d
    for kind in (0, 1):
        axes = []
        for k in range(d):
            o = np.arange(hi[k])
            if kind == 0:
                i0, i1, _, _ = ac_axis32(o, lo[k], hi[k])
            else:
                _, i0, i1 = ac_axis_exact(o, lo[k], hi[k])
            axes.append((torch.from_numpy(i0), torch.from_numpy(i1)))
        V = []
        for c in range(2 ** d):
            t = a
            for k in range(d):
                t = t.index_select(1 + k, axes[k][(c >> k) & 1])
            V.append(t)
            cmax = t.abs() if cmax is None else torch.maximum(cmax, t.abs())
        for k in range(d):
            for c in range(2 ** d):
                if not (c >> k) & 1:
                    dl = (V[c | (1 << k)] - V[c]).abs()
                    D[k] = dl if D[k] is None else torch.maximum(D[k], dl)
    slope = torch.zeros_like(cmax)
    for k in range(d):
        shp = [1] * (d + 2)
        shp[1 + k] = hi[k]
        slope = slope + COORD * torch.from_numpy(ac_axis_exact(np.arange(hi[k]), lo[k], hi[k])[0]).view(shp) * D[k]
    return cmax, slope


def blend_tol(X, lo, hi):
    cmax, slope = cell_terms(X, lo, hi)
    return K_BLEND * U * cmax + slope + TINY


# The adjoint, per input voxel i: dX[i] = sum over the outputs o that reference i of w_o(i) dY[o], w the product of the three axis
# weights.  Against float64 autograd:
#   * each axis weight is 1 - l or l: off by the coordinate error COORD coord_a(o), plus u / 2 for the rounding of 1 - l; the other
#     two weights are at most 1: |dY[o]| sum_a (COORD coord_a(o) + u / 2), over every o whose float32 OR exact cell holds i;
#   * w = (wz * wy) * wx two roundings, w * dY one, and the running sum over the n_c contributing outputs n_c - 1:
#     gamma(n_c + 3) sum_o |w_o dY[o]|.
# Both sums are separable along the axes (einsum with per-axis [O, I] matrices).  (The issue's starting form, the forward bound with
# max|dY| times n_c, is a factor 100 above the roundings.)
def axis_mats(I, O):
    """per axis: W [O, I] exact weights, R [O, I] 1 where the float32 or the exact cell of o holds i, E [O] the weight's error"""
    o = np.arange(O)
    i0, i1, _, _ = ac_axis32(o, I, O)
    coord, e0, e1 = ac_axis_exact(o, I, O)
    W, Rm = np.zeros((O, I)), np.zeros((O, I))
    l = coord - e0
    np.add.at(W, (o, e0), 1.0 - l)
    np.add.at(W, (o, e1), l)
    for idx in (i0, i1, e0, e1):
        Rm[o, idx] = 1.0
    return torch.from_numpy(W), torch.from_numpy(Rm), torch.from_numpy(COORD * coord + U / 2)


def adjoint_tol(dY, lo, hi):
    g = dY.abs().double()
    m = [axis_mats(lo[k], hi[k]) for k in range(3)]
    T = lambda A, B, Cm: torch.einsum("nzyxc,zi,yj,xk->nijkc", g, A, B, Cm)
    W, Rm = [t[0].abs() for t in m], [t[1] for t in m]
    ER = [t[2].view(-1, 1) * t[1] for t in m]
    coord = T(ER[0], Rm[1], Rm[2]) + T(Rm[0], ER[1], Rm[2]) + T(Rm[0], Rm[1], ER[2])
    cnt = torch.einsum("i,j,k->ijk", Rm[0].sum(0), Rm[1].sum(0), Rm[2].sum(0))
    mag = T(W[0], W[1], W[2])
    return coord + (cnt + 3).view(1, *lo, 1) * U * 1.001 * mag + TINY, cnt


def interp64(X, hi):
    d = len(hi)
    x = X.double().movedim(-1, 1)
    y = F.interpolate(x, size=tuple(hi), mode="trilinear" if d == 3 else "bilinear", align_corners=True)
    return y.movedim(1, -1).contiguous()


#            ratio C  padx pady
TRI_CASES = [(r, C, px, py) for r in range(len(RATIOS)) for (C, px, py) in ((4, 0, 8), (12, 8, 0))]
TRI_BIG_FWD = ((2, 3, 1), (17, 61681, 1))          # 17 * 61681 = 4096 * 256 + 1 output voxels at C = 4, one image
TRI_BIG_BWD = ((17, 61681, 1), (2, 8, 1))          # ... input voxels of the adjoint (61680 / 7: weights that are not 0 or 1)


def _tri(lo, hi, C, nv, seed):
    g = gen(4, *seed)
    X = rand(g, (nv, *lo, C))
    dY = rand(g, (nv, *hi, C))
    ref = interp64(X, hi)
    tol = blend_tol(X, lo, hi)
    # the adjoint: float64 autograd
    x64 = X.double().requires_grad_(True)
    interp64_out = F.interpolate(x64.movedim(-1, 1), size=tuple(hi), mode="trilinear", align_corners=True).movedim(1, -1)
    (dX,) = torch.autograd.grad(interp64_out, x64, dY.double())
    tol_b, cnt = adjoint_tol(dY, lo, hi)
    return dict(lo=lo, hi=hi, C=C, nv=nv, X=X, dY=dY, ref=ref, tol=tol, dX=dX.detach(), tol_b=tol_b, cnt=cnt)


@functools.lru_cache(maxsize=None)
def tri_case(i):
    r, C, px, py = TRI_CASES[i]
    lo, hi = RATIOS[r]
    c = _tri(lo, hi, C, NV, (i,))
    c.update(px=px, py=py)
    return c


@functools.lru_cache(maxsize=None)
def tri_big(bwd):
    lo, hi = TRI_BIG_BWD if bwd else TRI_BIG_FWD
    c = _tri(lo, hi, 4, 1, (900 + int(bwd),))
    c.update(px=0, py=0)
    return c


def _fma32(a, b, c):
    """fl32(a b + c) for fp32 tensors (the product is exact in float64; the double rounding of the sum moves an ulp at most)"""
    return (a.double() * b.double() + c.double()).float()


def emu_blend(v, hx, lx, hy, ly, hz, lz):
    """tl_blend1 on fp32 tensors, v[k] in the corner order z, y, x"""
    a0, a1 = _fma32(lx, v[1], hx * v[0]), _fma32(lx, v[3], hx * v[2])
    a2, a3 = _fma32(lx, v[5], hx * v[4]), _fma32(lx, v[7], hx * v[6])
    b0, b1 = _fma32(ly, a1, hy * a0), _fma32(ly, a3, hy * a2)
    return _fma32(lz, b1, hz * b0)


def emu_tri_fwd(c):
    lo, hi, X = c["lo"], c["hi"], c["X"]
    ax = [ac_axis32(np.arange(hi[k]), lo[k], hi[k]) for k in range(3)]
    t = lambda a, k: torch.from_numpy(np.ascontiguousarray(ax[k][a]))
    shp = [(1, -1, 1, 1, 1), (1, 1, -1, 1, 1), (1, 1, 1, -1, 1)]
    v = []
    for k in range(8):
        bz, by, bx = (k >> 2) & 1, (k >> 1) & 1, k & 1
        v.append(X.index_select(1, t(bz, 0)).index_select(2, t(by, 1)).index_select(3, t(bx, 2)))
    l = [t(2, k).view(shp[k]) for k in range(3)]
    h = [t(3, k).view(shp[k]) for k in range(3)]
    return emu_blend(v, h[2], l[2], h[1], l[1], h[0], l[0])


def emu_tri_bwd(c):
    """trilinear_bwd_kernel in fp32: per axis ac_weight, w = (wz * wy) * wx, acc += w * g over the outputs in zo, yo, xo order"""
    lo, hi, dY = c["lo"], c["hi"], c["dY"]
    W = []
    for k in range(3):
        i0, i1, l, h = ac_axis32(np.arange(hi[k]), lo[k], hi[k])
        m = np.zeros((hi[k], lo[k]), dtype=F32)
        for o in range(hi[k]):
            m[o, i0[o]] += h[o]
            m[o, i1[o]] = F32(m[o, i1[o]] + l[o])
        W.append(torch.from_numpy(m))
    acc = torch.zeros((c["nv"], *lo, c["C"]))
    for zo in range(hi[0]):
        for yo in range(hi[1]):
            wzy = W[0][zo].view(-1, 1, 1) * W[1][yo].view(1, -1, 1)
            for xo in range(hi[2]):
                w = (wzy * W[2][xo].view(1, 1, -1)).view(1, *lo, 1)
                acc = acc + w * dY[:, zo, yo, xo].view(c["nv"], 1, 1, 1, c["C"])
    return acc


# ======================================================================================================================================
# (3) row kernels: gather_upcat_rows3d(_h), lerp8_cat_rows3d(_h), lerp8_rows3d_bwd, the fp32-atomic scatters
# ======================================================================================================================================
#              ratio Clo  Chi n    pad  off     pad: ld = C + pad on every operand; off: the operand starts `off` channels into the buffer
ROW_CASES = [(0, 4, 4, 76, 0, 0), (0, 260, 8, 77, 8, 4), (1, 12, 0, 79, 8, 4), (2, 12, 4, 77, 8, 0), (3, 4, 12, 76, 0, 0),
             (4, 4, 4, 79, 8, 4), (5, 12, 4, 76, 8, 4), (6, 4, 4, 77, 0, 0), (1, 0, 8, 76, 8, 0), (2, 260, 0, 79, 0, 0)]


@functools.lru_cache(maxsize=None)
def row_case(i):
    """lo [NV, *lo, Clo] fp32, hi [NV, *hi, Chi] fp32 and f16, pix; the rows of cat(trilinear(lo), hi)[pix] in float64 with the
    forward bound on the lo part (the hi part is exact: a copy, f16 widening is exact); V = the eight corner rows of every sampled
    voxel (rows 8 j + k), the input of lerp8_cat_rows3d."""
    r, Clo, Chi, n, pad, off = ROW_CASES[i]
    lo, hi = RATIOS[r]
    g = gen(5, i)
    LO = rand(g, (NV, *lo, max(Clo, 1)))[..., :Clo].contiguous()
    HI = rand(g, (NV, *hi, max(Chi, 1)))[..., :Chi].contiguous()
    HI16 = HI.half()
    pix = sample_pix(200 + i, NV, hi, n)
    cn = corners(pix, lo, hi)
    vhi = int(np.prod(hi))
    if Clo:
        ref_lo = interp64(LO, hi).view(NV * vhi, Clo)[pix]
        tol_lo = blend_tol(LO, lo, hi).view(NV * vhi, Clo)[pix]
    else:
        ref_lo, tol_lo = torch.zeros((n, 0), dtype=torch.float64), torch.zeros((n, 0), dtype=torch.float64)
    idx8 = torch.from_numpy(cn["idx"])
    V = LO.view(NV * int(np.prod(lo)), Clo)[idx8.reshape(-1)].contiguous()                        # [8 n, Clo]
    return dict(lo=lo, hi=hi, Clo=Clo, Chi=Chi, n=n, pad=pad, off=off, LO=LO, HI=HI, HI16=HI16, pix=pix, cn=cn, ref_lo=ref_lo,
                tol_lo=tol_lo, hi_rows=HI.view(NV * vhi, Chi)[pix], hi16_rows=HI16.view(NV * vhi, Chi)[pix].float(), V=V,
                LO2=LO.view(NV * int(np.prod(lo)), Clo), HI2=HI.view(NV * vhi, Chi), HI162=HI16.view(NV * vhi, Chi))


def emu_rows(c):
    """the blend of the eight corner rows in fp32 with the restatement's weights (both row kernels and the dense kernel)"""
    ax, n, Clo = c["cn"]["ax"], c["n"], c["Clo"]
    v = [c["V"].view(n, 8, Clo)[:, k] for k in range(8)]
    t = lambda a, k: torch.from_numpy(np.ascontiguousarray(ax[k][a])).view(n, 1)
    return emu_blend(v, t(3, 2), t(2, 2), t(3, 1), t(2, 1), t(3, 0), t(2, 0))


# lerp8_rows3d_bwd / the dV part of lerp4_cat_rows_bwd: dV[2^d j + k] = w[2^d j + k] * dX[j] - one IEEE multiplication per element of
# the fp32 weight it is GIVEN (lerp8) or forms from (ly, lx) by one multiplication after 1 - l (lerp4: w = h h, h l, l h, l l).  Held
# to u |ref| against the float64 product of the same fp32 weight (the weight's own error against the exact coordinate is what
# corner_property holds), and bit for bit against the fp32 product.
@functools.lru_cache(maxsize=None)
def lerp_bwd_case(i, d):
    r, Clo, Chi, n, pad, off = ROW_CASES[i]
    lo, hi = RATIOS[r] if d == 3 else RATIOS_2D[r]
    g = gen(6, i, d)
    pix = sample_pix(300 + 10 * d + i, NV, hi, n)
    cn = corners(pix, lo, hi)
    dX = rand(g, (n, Clo + Chi))
    w = torch.from_numpy(cn["w"])                                                                # [n, 2^d] fp32
    ref = (w.double().view(n, -1, 1) * dX[:, :Clo].double().view(n, 1, Clo)).reshape(n * 2 ** d, Clo)
    emu = (w.view(n, -1, 1) * dX[:, :Clo].view(n, 1, Clo)).reshape(n * 2 ** d, Clo)
    out = dict(lo=lo, hi=hi, Clo=Clo, Chi=Chi, n=n, pad=pad, off=off, pix=pix, cn=cn, dX=dX, w=w.reshape(-1).contiguous(), ref=ref,
               tol=U * ref.abs() + TINY, emu=emu,
               lylx=torch.from_numpy(np.stack([cn["ax"][a][2] for a in range(d)], 1).reshape(-1).copy()))
    out.update(scatter_hi(pix, dX[:, Clo:], NV * int(np.prod(hi))))
    return out


# The fp32-atomic scatters: dlo[corner k of pix[j]] += w_k(j) * dX[j][:Clo], dhi[pix[j]] += dX[j][Clo:].  The sum's order is the
# order of arrival: any order of n_r terms is within (n_r - 1) u sum|terms|; the term itself is ((wz * wy) * wx) * v, three
# roundings (2-D: two): (n_r + 3) u sum|terms| per element covers both against the float64 sum of the products of the same fp32
# 1 - l and l.  n_r counts every term that lands on the element (a clamped corner pair lands twice).
def scatter_ref(rows, terms, M):
    """rows [m] int64, terms [m, C] float64 -> sum, sum|.|, count per destination row"""
    C = terms.shape[1]
    s, a = torch.zeros((M, C), dtype=torch.float64), torch.zeros((M, C), dtype=torch.float64)
    s.index_add_(0, rows, terms)
    a.index_add_(0, rows, terms.abs())
    n_r = torch.zeros(M, dtype=torch.float64).index_add_(0, rows, torch.ones(rows.shape[0], dtype=torch.float64))
    return s, a, n_r


def scatter_hi(pix, g_hi, M):
    s, a, n_r = scatter_ref(pix, g_hi.double(), M)
    return dict(dhi=s, tol_hi=(n_r.view(-1, 1) + 3) * U * a + TINY, nr_hi=n_r)


@functools.lru_cache(maxsize=None)
def scatter_case(i, d):
    c = dict(lerp_bwd_case(i, d))
    n, Clo = c["n"], c["Clo"]
    rows = torch.from_numpy(c["cn"]["idx"]).reshape(-1)
    s, a, n_r = scatter_ref(rows, c["ref"], NV * int(np.prod(c["lo"])))
    c.update(dlo=s, tol_lo=(n_r.view(-1, 1) + 3) * U * a + TINY, nr_lo=n_r, rows=rows)
    return c


def emu_scatter(rows, terms32, M):
    """fp32 accumulation in the order of the list (one of the orders the atomics may take)"""
    out = torch.zeros((M, terms32.shape[1]))
    for r, t in zip(rows.tolist(), terms32):
        out[r] = out[r] + t
    return out


# ======================================================================================================================================
# (4) copy_rows, layout transposes, put_rows, row_nonzero, casts                                      exact
# ======================================================================================================================================
#             M        C   padx pady
COPY_CASES = [(1, 4, 0, 0), (7, 12, 8, 0), (5, 260, 0, 8), (33, 8, 8, 8), (4096 * 256 + 1, 4, 0, 0)]


@functools.lru_cache(maxsize=None)
def copy_case(i):
    M, C, px, py = COPY_CASES[i]
    g = gen(7, i)
    X, Y0 = rand(g, (M, C)), rand(g, (M, C))
    return dict(M=M, C=C, px=px, py=py, X=X, Y0=Y0, acc=X + Y0)


#              NB C   P   pad
TRANS_CASES = [(3, 5, 1, 0), (1, 33, 70, 3), (2, 31, 33, 0), (3, 64, 32, 8), (1, 1, 1, 1)]


@functools.lru_cache(maxsize=None)
def trans_case(i):
    NB, C, P, pad = TRANS_CASES[i]
    X = rand(gen(8, i), (NB, C, P))
    return dict(NB=NB, C=C, P=P, pad=pad, nchw=X, nhwc=X.permute(0, 2, 1).contiguous())


#            n   C    Mdst pads padd
PUT_CASES = [(5, 263, 9, 1, 5), (7, 4, 7, 0, 0), (6, 513, 11, 3, 3), (3, 3, 5, 1, 1)]


@functools.lru_cache(maxsize=None)
def put_case(i):
    n, C, M, ps, pd = PUT_CASES[i]
    g = gen(9, i)
    src = rand(g, (n, C))
    idx = torch.randperm(M, generator=g)[:n].contiguous()
    ref = torch.full((M, C), SENTINEL)
    ref[idx] = src
    return dict(n=n, C=C, M=M, lds=C + ps, ldd=C + pd, src=src, idx=idx, ref=ref)


def nonzero_case():
    """M = 11 rows (M % 4 != 0) of C = 263 channels (vector loop: 0 .. 255 and a second trip at 256 .. 259; tail 260 .. 262), ld = 264:
    the pad column holds the sentinel and must not be read."""
    C, M = 263, 11
    X = torch.zeros((M, C))
    X[1, ::2] = -0.0                                     # +0 / -0 only
    X[2, 17] = 1e-45                                     # a single subnormal
    X[3, 100] = math.nan
    X[4, 259] = -math.inf
    X[5, 262] = 1.0                                      # only in the last tail channel
    X[6, 256] = -2.0                                     # only in channel 256: the vector loop's second trip
    X[7] = rand(gen(10), (C,))
    X[9, 0] = 1.0
    X[10, 260] = 1e-30
    ref = torch.tensor([0, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    return dict(C=C, M=M, ld=264, X=X, ref=ref)


CAST_N = (1, 2, 3, 4, 5, 6, 7, 1027, 4 * (4096 * 256) + 5)     # n % 4 in {0 .. 3}, n < 4, and one vector past the grid cap
CAST_SCALE = 1024.0


@functools.lru_cache(maxsize=None)
def cast_case(n):
    """f2h: (x * scale) clamped to +-65504, then rounded to f16 - the CPU's arithmetic.  The kernel saturates: values above 65504
    after scaling, +-inf included, become +-65504; NaN stays NaN.  The specials (repeated through the buffer): products that round
    to f16 subnormals, to zero, exactly 65504, just above it (65504 (1 + 2^-23), 65520, 1e6), +-inf, NaN, -0.0.
    h2f: every f16 bit pattern class (subnormals, +-inf, NaN, -0.0) widened: exact."""
    g = gen(11, n)
    s = CAST_SCALE
    spec = torch.tensor([3e-6 / s, -5.9e-8 / s, 2e-8 / s, 65504.0 / s, -65504.0 / s, 65504.0 * (1 + 2.0 ** -23) / s, 65520.0 / s, 1e6 / s,
                         -1e6 / s, math.inf, -math.inf, math.nan, -0.0, 6.1e-5 / s, 1.0 / s, 33.3337 / s], dtype=torch.float32)
    x = rand(g, (n,)) * 40.0
    k = torch.arange(n)
    x = torch.where(k % 3 == 0, spec[(k // 3) % spec.numel()], x) if n < 64 else torch.where(k % 64 < 16, spec[k % 16], x)
    f2h = (x * s).clamp(-65504.0, 65504.0).half()
    hbits = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int64).to(torch.int16)
    hspec = torch.tensor([0x0001, -0x7fff, 0x7c00, -0x400, 0x7e01, -0x8000, 0x03ff, 0x7bff], dtype=torch.int64).to(torch.int16)
    hbits = torch.where(k % 5 == 0, hspec[(k // 5) % 8], hbits)
    h = hbits.view(torch.float16)
    return dict(n=n, x=x, f2h=f2h, h=h, h2f=h.float())


def same_or_nan(got, ref):
    """bit for bit, except that a NaN may be any NaN"""
    got, ref = got.detach().cpu(), ref
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    iv = {2: torch.int16, 4: torch.int32}[got.element_size()]
    nan = torch.isnan(ref)
    return bool((torch.isnan(got) == nan).all()) and bool((got.view(iv) == ref.view(iv))[~nan].all())


# ======================================================================================================================================
# (5) optimiser steps                                                                                  bounded
# ======================================================================================================================================
# sgd_nesterov_kernel: gv = g + wd p; b = first ? gv : mom buf + gv; p' = p - lr (nesterov ? gv + mom b : b); the compiler may
# contract any product into the following sum, so every step is bounded by roundings x sum|terms| (fewer roundings when fused):
#   Tg = |g| + |wd p| (2 roundings), Tb = first ? Tg : |mom buf| + Tg (2 more: 4), Ts = nesterov ? Tg + mom Tb : Tb (2 more: 6),
#   buf' within gamma(4) Tb;  p' = p - lr step: the product and the difference, gamma(2) (|p| + lr Ts), plus lr x the step's own
#   error gamma(6) lr Ts.
# Reference: the float64 formula of torch.optim.SGD on the same fp32 p, g, buf, lr, momentum, weight_decay.
#            n     lr    mom  wd    first
OPT_CASES = [(1, 0.01, 0.9, 1e-4, 0), (255, 0.01, 0.9, 0.0, 1), (1027, 0.1, 0.0, 1e-4, 0), (1027, 0.01, 0.9, 1e-4, 1),
             (4096 * 256 + 1, 0.003, 0.99, 5e-4, 0)]


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def opt_case(i, nesterov):
    n, lr, mom, wd, first = OPT_CASES[i]
    g_ = gen(12, i)
    p, g, buf = rand(g_, (n,)), rand(g_, (n,)) * 0.1, rand(g_, (n,)) * 0.3
    lr_, mom_, wd_ = f32(lr), f32(mom), f32(wd)
    p64, g64, b64 = p.double(), g.double(), buf.double()
    gv = g64 + wd_ * p64
    b = gv if first else mom_ * b64 + gv
    step = gv + mom_ * b if nesterov else b
    Tg = g64.abs() + (wd_ * p64).abs()
    Tb = Tg if first else (mom_ * b64).abs() + Tg
    Ts = Tg + mom_ * Tb if nesterov else Tb
    return dict(n=n, lr=lr, mom=mom, wd=wd, first=first, p=p, g=g, buf=buf, ref_p=p64 - lr_ * step, ref_b=b,
                tol_b=gamma(4) * Tb + TINY, tol_p=gamma(2) * (p64.abs() + lr_ * Ts) + gamma(6) * lr_ * Ts + TINY)


def emu_opt(c, nesterov):
    p, g, buf = c["p"], c["g"], c["buf"]
    lr, mom, wd = (torch.tensor(c[k], dtype=torch.float32) for k in ("lr", "mom", "wd"))
    gv = g + wd * p
    b = gv if c["first"] else mom * buf + gv
    return p - lr * ((gv + mom * b) if nesterov else b), b


# ema_kernel: om = fl(1 - m) (u / 2 absolute: relative u at worst on om <= 1 ... folded into the q term), k m + q om: two products
# and a sum, or a product, an fma: gamma(2) |k m| + gamma(3) |q (1 - m)|.  m = 1: om = 0 and k stays, bit for bit; m = 0: k = q.
#            n     m
EMA_CASES = [(1027, 0.0), (1027, 0.99), (255, 1.0), (4096 * 256 + 1, 0.999)]


@functools.lru_cache(maxsize=None)
def ema_case(i):
    n, m = EMA_CASES[i]
    g_ = gen(13, i)
    k, q = rand(g_, (n,)), rand(g_, (n,))
    m_ = f32(m)
    a, b = k.double() * m_, q.double() * (1.0 - m_)
    return dict(n=n, m=m, k=k, q=q, ref=a + b, tol=gamma(2) * a.abs() + gamma(3) * b.abs() + TINY,
                emu=k * torch.tensor(m, dtype=torch.float32) + q * (1.0 - torch.tensor(m, dtype=torch.float32)))


# ======================================================================================================================================
# (6) det_scatter.hip: absmax, and the fixed-point chain absmax -> scatter -> finish -> clear        exact (int64 restatement)
# ======================================================================================================================================
DET_BITS = 44


def absmax_bits(x):
    """bit pattern of the largest |x| (a NaN's is above an infinity's) of an fp32 tensor, as a python int"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0x7fffffff
    return int(b.max()) if b.numel() else 0


#               n        C   pad  special
ABSMAX_CASES = [(1, 1, 0, None), (7, 63, 8, None), (5, 130, 8, "nan"), (3, 64, 0, "inf"), (4, 4, 4, "zero"), (2, 65, 3, "negmax"),
                (1024 * 256 + 1, 1, 1, None)]          # one element past the grid's 1024 x 256 threads


@functools.lru_cache(maxsize=None)
def absmax_case(i):
    """|values| <= 4 < |sentinel| = 7.25: a pad column read by mistake becomes the maximum"""
    n, C, pad, sp = ABSMAX_CASES[i]
    x = rand(gen(14, i), (n, C)).clamp(-4.0, 4.0)
    if sp == "nan":
        x[n - 1, C - 1] = math.nan
    if sp == "inf":
        x[0, 0] = -math.inf
    if sp == "zero":
        x.zero_()
        x[1, 1] = -0.0
    if sp == "negmax":
        x[1, C - 1] = -4.5
    if n > 1000:
        x[n - 1, 0] = 4.25                          # the maximum sits in the second trip's only element
    return dict(n=n, C=C, ld=C + pad, x=x, bits=absmax_bits(x))


# The chain, restated (numpy; every step is the kernel's own, none is a tolerance):
#   mb = absmax bits; sh = 44 + 126 - (mb >> 23); q_e = rint(ldexp(fl32(w_e * src[e / div]), sh)) (round half even, as __float2ll_rn;
#   the product is ONE fp32 multiplication; ldexp is exact above 2^-126 and whatever lies below rounds to q = 0 on both sides);
#   acc[r(e)] += q_e in int64 (r(e) = list ? list[idx[e]] : idx[e]); dst[r] = fl32(alpha * ldexp(fl32(acc[r]), -sh)) on every row
#   named by the entries: one int64 -> fp32 conversion (round to nearest even), an exact scaling, one multiplication.
#   mb >= 0x7f800000 (an inf or a NaN anywhere): the named rows become the quiet NaN 0x7fc00000, nothing is accumulated;
#   mb == 0: nothing is accumulated and NOTHING IS WRITTEN (the destination keeps what it held - head.py zero-fills it).
# Condition (asserted on the CPU): contributions per destination element x |w| <= 1 stay below the 2^18 headroom; sources are zero
# or normal.
# Float64 bound, per element: n_r 2^-45 max|src| + u |sum| against sum_e float64(fl32(w_e src_e)), n_r the contributions to the row.
# Each contribution is rounded to the unit 2^-sh, off by half a unit = 2^(E - 171) at most, E = mb >> 23; max|src| < 2^(E - 126), so
# half a unit is 2^-45 max|src| when the maximum sits at the TOP of its binade and up to 2^-44 max|src| at the bottom; u |sum| is
# the conversion.  The cases with small-valued rows (where the first term is all there is) therefore put the launch maximum at the
# top of a binade, (2 - 2^-23) 2^k, and so does the finite alpha = -3 case; elsewhere u |sum| dominates by 2^20.  With B the bound
# above, y the value before the last multiplication (|y - sum| <= B) and dst = fl(alpha y): a power of two multiplies exactly,
# |dst - alpha sum| <= |alpha| B; any other alpha rounds once more, u |alpha y| <= u |alpha| (|sum| + B), which gives
# |alpha| B (1 + u) + u |alpha sum|.
#             name        C   pad M_dst n_e   div list  w      alpha  special
DET_CASES = [("plain", 1, 0, 3, 7, 1, False, False, 1.0, None),
             ("list_w", 63, 8, 9, 50, 3, True, True, 0.5, "top"),
             ("corners", 64, 0, 12, 64, 8, False, True, -3.0, "top"),
             ("collide", 65, 0, 6, 4096 + 50, 1, False, True, 1.0, "top"),
             ("small_rows", 130, 8, 10, 80, 8, True, True, 1.0, "top_small"),
             ("min_normal", 64, 0, 5, 21, 1, False, False, 1.0, "min"),
             ("two_120", 65, 8, 7, 30, 3, True, True, 0.5, "big"),
             ("zero", 63, 0, 4, 9, 1, False, True, 1.0, "zero"),
             ("inf", 64, 8, 4, 9, 1, True, False, 1.0, "inf"),
             ("nan", 1, 0, 4, 9, 3, False, True, -3.0, "nan")]
TOP = float(np.float32(2.0) - np.float32(2.0 ** -23))


@functools.lru_cache(maxsize=None)
def det_case(i):
    name, C, pad, M, n_e, div, use_list, use_w, alpha, sp = DET_CASES[i]
    g = gen(15, i)
    n_src = (n_e + div - 1) // div
    src = rand(g, (n_src, C)).clamp(-3.9, 3.9)
    w = (torch.rand((n_e,), generator=g) * 2 - 1) if use_w else None
    if name == "collide":
        idx = torch.cat((torch.full((4096,), 2, dtype=torch.int64), torch.randint(0, M, (n_e - 4096,), generator=g)))
    else:
        idx = torch.randint(0, M - 1, (n_e,), generator=g)                     # the last destination row is never named
    lst = None
    if use_list:                                                                # idx names entries of the int32 list
        lst = torch.randperm(M, generator=g)[:M - 1].to(torch.int32).contiguous()
    if sp in ("top", "top_small"):
        src[0, 0] = TOP * 2.0                                                   # 3.9999998: the top of [2, 4)
    if sp == "top_small":
        src[1] = src[1] * 2.0 ** -30                                            # a small-valued row: 2^-30 of the maximum
        src[2] = src[2].sign() * 2.0 ** -48                                     # all below 2^-45 of the maximum: comes out zero
        idx[8:16] = 0                                                           # rows 1 and 2 (div = 8) go to destinations 0 and 1,
        idx[16:24] = 1                                                          # and nothing else does
        idx[:8] = 2
        idx[24:] = torch.randint(2, M - 1, (n_e - 24,), generator=g)
    if sp == "min":
        src = torch.where(torch.rand((n_src, C), generator=g) < 0.5, 0.0, 1.0) * src.sign() * 2.0 ** -126
        src[0, 0] = 2.0 ** -126
    if sp == "big":
        src = src * 2.0 ** 110
        src[0, 0] = -(2.0 ** 120)
    if sp == "zero":
        src.zero_()
    if sp == "inf":
        src[1, 3] = math.inf
    if sp == "nan":
        src[2, 0] = math.nan
    c = dict(name=name, C=C, ld_acc=C + pad, M=M, n_e=n_e, div=div, lst=lst, w=w, alpha=alpha, sp=sp, src=src, idx=idx, n_src=n_src)
    c.update(det_chain(src, div, lst, idx, w, alpha, M))
    return c


def det_chain(src, div, lst, idx, w, alpha, M, drop=None):
    """the restatement; drop = an entry left out (a planted error)"""
    s = src.numpy()
    n_e, C = idx.shape[0], s.shape[1]
    mb = absmax_bits(src)
    r = idx.numpy() if lst is None else lst.numpy().astype(np.int64)[idx.numpy()]
    touched = np.zeros(M, dtype=bool)
    touched[r] = True
    acc = np.zeros((M, C), dtype=np.int64)
    out = dict(mb=mb, rows=torch.from_numpy(r.copy()), touched=torch.from_numpy(touched))
    if mb >= 0x7f800000:
        out.update(acc=torch.from_numpy(acc), dst=None, kind="nan")
        return out
    if mb == 0:
        out.update(acc=torch.from_numpy(acc), dst=None, kind="zero")
        return out
    sh = DET_BITS + 126 - (mb >> 23)
    e = np.arange(n_e)
    wv = np.ones(n_e, dtype=F32) if w is None else w.numpy()
    prod = (wv[:, None] * s[e // div]).astype(F32)
    q = np.rint(np.ldexp(prod.astype(np.float64), sh)).astype(np.int64)
    keep = np.ones(n_e, dtype=bool)
    if drop is not None:
        keep[drop] = False
    np.add.at(acc, r[keep], q[keep])
    dst = (F32(alpha) * np.ldexp(acc.astype(F32), -sh).astype(F32)).astype(F32)
    # float64
    p64 = torch.from_numpy(prod.astype(np.float64))
    ssum, _, n_r = scatter_ref(out["rows"], p64, M)
    amax = float(torch.tensor([mb], dtype=torch.int32).view(torch.float32))
    pow2_alpha = math.frexp(abs(alpha))[0] == 0.5
    tol = abs(alpha) * (n_r.view(-1, 1) * 2.0 ** -45 * amax + U * ssum.abs())
    if not pow2_alpha:                                                          # the final multiplication rounds
        tol = tol * (1.0 + U) + U * (alpha * ssum).abs()
    tol = tol + TINY
    per_elem = np.zeros((M, C), dtype=np.int64)
    np.add.at(per_elem, r, (np.abs(wv)[:, None] * np.ones((1, C)) > 0).astype(np.int64))
    out.update(acc=torch.from_numpy(acc), dst=torch.from_numpy(dst), kind="ok", sh=sh, ref64=alpha * ssum, tol64=tol, n_r=n_r,
               max_contrib=int(per_elem.max()), pow2_alpha=pow2_alpha)
    return out


# ======================================================================================================================================
# (7) comparison helpers of the GPU file (each is shown to reject a planted error in the CPU file)
# ======================================================================================================================================
GUARD = 8                                             # sentinel elements kept behind every output buffer


def sent(dtype):
    return SENTINEL if dtype.is_floating_point else ISENT


def body(buf, n, shape=None):
    """the first n elements of a guarded buffer on the CPU, after checking that the guard still holds the sentinel"""
    if buf.is_cuda:
        torch.cuda.synchronize()
    assert bool((buf[n:n + GUARD] == sent(buf.dtype)).all()), "the guard behind the buffer was written"
    out = buf[:n].cpu()
    return out if shape is None else out.view(shape)


def cols(buf, rows, ld, off, C):
    """(the [rows, C] operand, True when every other column and the guard still hold the sentinel)"""
    got = body(buf, rows * ld, (rows, ld))
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + C] = False
    return got[:, off:off + C], bool((got[:, keep] == sent(buf.dtype)).all())


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_corners(name, c, idx, w):
    """the float64 property first (the binding check), then indices and weight bits against the numpy float32 restatement"""
    k = 2 ** c["cn"]["d"]
    r_coord, r_sum, inside = corner_property(idx.view(-1, k).numpy(), w.view(-1, k).numpy(), c["cn"])
    print(f"{name}: coordinate err / (4 S u) {r_coord:.3f}, weight-sum err / (4 u) {r_sum:.3f}")
    assert inside and r_coord <= 1.0 and r_sum <= 1.0, name + ": the float64 property fails"
    assert exact(idx, c["idx"]) and bits_equal(w, c["w"]), name + ": the float64 property holds but the float32 restatement differs"
