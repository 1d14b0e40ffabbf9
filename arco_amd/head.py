"""Row-sparse student head (trainer-internal fast path; results identical to the dense modules).

In the reference step the student representation
    rep = q_representation(FeatureExtractor(feature_map))          (train_arco_2d.py:317-330)
is a dense [B,496,256,256] tensor, but the loss only ever reads <= num_queries rows of it per
class (loss_helper_3d.py:455-457) and d loss / d rep is non-zero only on those rows.  Every op
between the 128x128 level of the FeatureExtractor and `rep` is per-pixel (1x1 convs) or a
4-neighbour bilinear lerp, so the sampled rows can be computed exactly from
    x3p = fea3(x)+x   [B,480,128,128]   (dense, cheap)      and    f4 [B,16,256,256]:
    X4[j] = cat(bilinear(x3p)[pix_j], f4[pix_j]);   A[j] = W2 . W1 . W4 . X4[j]
Row values are bit-identical to the dense path (same fp32 lerp order, same K-order MFMA
accumulation); the backward scatters dX4 rows back into x3p / f4 and the weight gradients are
GEMMs over the anchor rows only.  This removes ~3.3 TFLOP/step of dense fp32 GEMM work at
BASELINE config 2 without changing any result.
"""
import math
import os

import torch

from . import _lib as L
from . import ops
from ._contrast import _ceil, rows_view


def _gemm(x, w):
    """x [n, K] @ w[N, K]^T on the MFMA conv kernel (1x1)."""
    n, k = int(x.shape[0]), int(x.shape[1])
    y, _ = ops.conv_raw(x, x.stride(0), k, ops.pack_weight(w, 1, 0), int(w.shape[0]), 1, 1, n, 1)
    return y.permute(0, 2, 3, 1).reshape(n, int(w.shape[0]))


def _gemm_t(dy, w):
    """dy [n, N] @ w[N, K]  (data gradient of _gemm)."""
    n, nn_ = int(dy.shape[0]), int(dy.shape[1])
    y, _ = ops.conv_raw(dy, dy.stride(0), nn_, ops.pack_weight(w, 1, 1), int(w.shape[1]), 1, 1, n, 1)
    return y.permute(0, 2, 3, 1).reshape(n, int(w.shape[1]))


def _wgrad(dy, x, like):
    n = int(dy.shape[0])
    return ops.conv_wgrad(dy, dy.stride(0), int(dy.shape[1]), x, x.stride(0), int(x.shape[1]), 1, 1, 1, n, like)


def _fm_grad_buffer(half, ptr, shape, dev):
    """(fp32 scatter target [nb, *spatial, c], done(idx, n) -> the gradient to hand back) of a feature map read as rows: the f16
    form of the producer's gradient carrying ops.LOSS_SCALE for a map stored as f16 (_row_grad_buffer_h), else the target itself
    (_row_grad_buffer)."""
    if half:
        return _row_grad_buffer_h(ptr, shape, dev)
    buf, fin = _row_grad_buffer(ptr, shape, dev)

    def done(idx, n):
        fin(idx, n)
        return buf
    return buf, done


def _fea_rows(X, w, mode):
    """fea_i(X) + X on rows (mode 0) / its data gradient W^T dY + dY (mode 1): the 1x1 conv with the residual in the GEMM epilogue."""
    k = int(X.shape[1])
    y, _ = ops.conv_raw(X, k, k, ops.pack_weight(w, 1, mode), k, 1, 1, int(X.shape[0]), 1, residual=X, ld_res=k)
    return y.permute(0, 2, 3, 1).reshape(int(X.shape[0]), k)


def _row_grad_buffer(ptr, shape, dev):
    """Zero channels-last buffer [nb, *spatial, c] for a sparse row-scatter gradient of the feature map [nb, c, *spatial] at
    `ptr`, and a finaliser fin(idx, n).  When the map is an output of a graph-replayed pass the buffer IS that pass's
    gradient-input buffer (ops.grad_sink: zero by invariant) - no dense fill, no copy into the graph - and fin registers
    the re-zeroing of the n touched rows idx after the backward graph has replayed; otherwise a fresh zeros tensor and
    a no-op."""
    nb, c, spatial = int(shape[0]), int(shape[1]), tuple(int(v) for v in shape[2:])
    gt, k = ops.grad_sink(ptr, (nb, c) + spatial)
    if gt is not None:
        buf = gt.static_grads[k].movedim(1, -1)
        if buf.is_contiguous() and c % 4 == 0:
            def fin(idx, n):
                gt.cleanup.append(lambda: L.call("arco_zero_rows", L.ptr(buf), c, c, L.ptr(idx), n))
            return buf, fin
        gt.sink_busy[k] = False
    return torch.zeros((nb,) + spatial + (c,), dtype=torch.float32, device=dev), (lambda idx, n: None)


def _row_grad_buffer_h(ptr, shape, dev):
    """_row_grad_buffer for a feature map stored as f16 (ops.fm_rows_half): (fp32 scatter target [nb, *spatial, c], done(idx, n) ->
    the f16 gradient [nb, *spatial, c] carrying ops.LOSS_SCALE).  Graph-replayed producer: the scatter target is a persistent fp32
    scratch (zero by invariant), done() casts the n touched rows into the producer's f16 gradient-input buffer (ops.grad_sink),
    re-zeroes them in the scratch and registers their re-zeroing in the f16 buffer for after the backward graph - the rows are summed
    in fp32 and rounded once, exactly as the dense cast of the dense fp32 gradient did.  Otherwise: a fresh fp32 tensor and a dense cast."""
    nb, c, spatial = int(shape[0]), int(shape[1]), tuple(int(v) for v in shape[2:])
    gt, k = ops.grad_sink(ptr, (nb, c) + spatial)
    if gt is not None:
        buf = gt.static_grads[k].movedim(1, -1)
        if buf.is_contiguous() and c % 4 == 0 and buf.dtype == torch.float16:
            scratch = gt.__dict__.setdefault("_row_scratch", {}).get(k)
            if scratch is None:
                scratch = gt._row_scratch[k] = torch.zeros(buf.shape, dtype=torch.float32, device=dev)

            def done(idx, n):
                L.call("arco_cast_rows_f2h", L.ptr(scratch), c, c, L.ptr(idx), n, float(ops.LOSS_SCALE), L.ptr(buf), c)
                L.call("arco_zero_rows", L.ptr(scratch), c, c, L.ptr(idx), n)
                gt.cleanup.append(lambda: L.call("arco_zero_rows_h", L.ptr(buf), c, c, L.ptr(idx), n))
                return buf
            return scratch, done
        gt.sink_busy[k] = False
    dense = torch.zeros((nb,) + spatial + (c,), dtype=torch.float32, device=dev)

    def done_dense(idx, n):
        out = torch.empty(dense.shape, dtype=torch.float16, device=dev)
        L.call("arco_cast_f2h", L.ptr(dense), dense.numel(), float(ops.LOSS_SCALE), L.ptr(out))
        return out
    return dense, done_dense


# Order-independent row scatter (csrc/det_scatter.hip): fixed-point int64 accumulation instead of fp32 atomics - the gradient of the
# row-sparse 3-D head is bit-reproducible, which f16 activation storage needs to be reproducible at all (the ulp of an fp32 atomic's
# arrival order decides f16 roundings downstream; profiles/r05_notes.md section 7).  ARCO_DET_SCATTER = 0: fp32 atomics everywhere;
# 1 (default): the 3-D head order-independent; 2: the 2-D heads too (17 more small launches on the 2-D step's critical path).
DET_SCATTER = int(os.environ.get("ARCO_DET_SCATTER", "1"))
# The fixed-point accumulators of the order-independent scatter: one int64 buffer of the destination's size per (device, rows, channels),
# kept between steps (zero between uses: every call clears exactly the rows it touched) - 315 MB for the LiTS-shaped full-resolution map,
# 80 MB for its half-resolution one (a trainer uses two).  Nothing evicts them behind the caller's back - captured HIP graphs hold their
# addresses; release_det_buffers() frees them once no graph that used them will be replayed.  A buffer first created inside a capture
# lives in that graph's pool, which is why the trainers run their first steps eagerly.  Resolution: values are scaled to the launch-wide largest magnitude, so a contribution below 2^-45 of that
# maximum is dropped - far below one fp32 ulp of any sum the maximum takes part in, not of a row that only holds tiny values.
_ACC64 = {}


def _det_acc(dev, rows, C):
    key = (dev.index, rows, C)
    acc = _ACC64.get(key)
    if acc is None:
        acc = _ACC64[key] = torch.zeros((rows, C), dtype=torch.int64, device=dev)
    return acc


def release_det_buffers():
    """Free the int64 accumulators of the order-independent scatter (they are re-created, zeroed, on the next use)."""
    _ACC64.clear()


def _det_scatter_rows(src, ld_src, C, div, idx, w, n_e, dst, ld_dst):
    """dst[idx[e]] = sum over e of w[e] * src[e // div] (C channels), dst rows zero before; src: [n_e // div, >= C] fp32 view."""
    dev = src.device
    rows = dst.numel() // ld_dst
    acc = _det_acc(dev, rows, C)
    mb = torch.empty(1, dtype=torch.int32, device=dev)
    try:
        L.call("arco_det_absmax", L.ptr(src), ld_src, C, n_e // div, L.ptr(mb))
        L.call("arco_det_scatter_rows", L.ptr(src), ld_src, C, div, None, L.ptr(idx), None if w is None else L.ptr(w), n_e,
               L.ptr(acc), C, L.ptr(mb))
        L.call("arco_det_finish_rows", None, L.ptr(idx), n_e, L.ptr(acc), C, C, L.ptr(mb), 1.0, L.ptr(dst), ld_dst)
        L.call("arco_det_clear_rows", None, L.ptr(idx), n_e, L.ptr(acc), C, C)
    except Exception:
        _ACC64.pop((dev.index, rows, C), None)      # "zero between uses" may no longer hold: the next call starts from a fresh buffer
        raise


def _scatter_upcat2d(dX, ldx, pix, n, dlo, clo, hi_h, hi_w, dhi, chi, ho, wo):
    """adjoint of arco_gather_upcat_rows: dlo += bilinear corners of dX[:, :clo], dhi[pix] += dX[:, clo:]"""
    if DET_SCATTER >= 2:
        dev = dX.device
        idx4 = torch.empty(4 * n, dtype=torch.int64, device=dev)
        w4 = torch.empty(4 * n, dtype=torch.float32, device=dev)
        L.call("arco_corner_rows2d", L.ptr(pix), n, hi_h, hi_w, ho, wo, L.ptr(idx4), L.ptr(w4))
        _det_scatter_rows(dX, ldx, clo, 4, idx4, w4, 4 * n, dlo, clo)
        _det_scatter_rows(dX[:, clo:], ldx, chi, 1, pix, None, n, dhi, chi)
    else:
        L.call("arco_scatter_upcat_rows", L.ptr(dX), ldx, L.ptr(pix), n, L.ptr(dlo), clo, clo, hi_h, hi_w, L.ptr(dhi), chi, chi, ho, wo)


def _lerp4_cat_rows_bwd(dX, ldx, clo, lylx, pix, n, dV, dhi, chi):
    """adjoint of arco_lerp4_cat_rows: the four weighted copies of dX[:, :clo] (plain stores) and dhi[pix] += dX[:, clo:]"""
    if DET_SCATTER >= 2:
        L.call("arco_lerp4_cat_rows_bwd", L.ptr(dX), ldx, clo, L.ptr(lylx), L.ptr(pix), n, L.ptr(dV), clo, L.ptr(dhi), chi, 0)
        _det_scatter_rows(dX[:, clo:], ldx, chi, 1, pix, None, n, dhi, chi)
    else:
        L.call("arco_lerp4_cat_rows_bwd", L.ptr(dX), ldx, clo, L.ptr(lylx), L.ptr(pix), n, L.ptr(dV), clo, L.ptr(dhi), chi, chi)


def _q_tail(X, w4, w1, w2):
    """fea4, q_representation[0] and [1] on rows: (h0, h1, a)."""
    h0 = _gemm(X, w4)
    h1 = _gemm(h0, w1)
    return h0, h1, _gemm(h1, w2)


def _q_tail_bwd(da, X, h0, h1, w4, w1, w2):
    """adjoint of _q_tail: (dX, dw4, dw1, dw2) - the weight gradients are GEMMs over the anchor rows only."""
    da = da.contiguous()
    dw2 = _wgrad(da, h1, w2)
    dh1 = _gemm_t(da, w2)
    dw1 = _wgrad(dh1, h0, w1)
    dh0 = _gemm_t(dh1, w1)
    dw4 = _wgrad(dh0, X, w4)
    return _gemm_t(dh0, w4), dw4, dw1, dw2


def _rows2d(lo, maps, feas, pix):
    """The 2-D row path through L = len(maps) levels (maps and feas coarse to fine).  idx[L-1] = pix and idx[i-1] = the 4 neighbours at
    maps[i-1]'s resolution of every row of idx[i] (4^(L-1-i) n rows at level i); Xs[0] = cat(bilinear(lo), maps[0]) on idx[0];
    Xs[i] = cat(4-way lerp of fea_i(Xs[i-1])+Xs[i-1], maps[i][idx[i]]).  Returns (Xs, idx, lylx) as lists by level, lylx[i] being the
    lerp coefficients into level i (lylx[0] is None); Xs[-1] is the input rows of fea4."""
    dev = lo.device
    nl = len(maps)
    lo_r, ldlo = rows_view(lo)
    rv = [rows_view(m) for m in maps]
    idx, lylx = [None] * (nl - 1) + [pix], [None] * nl
    for i in range(nl - 1, 0, -1):
        m = int(idx[i].shape[0])
        idx[i - 1] = torch.empty(4 * m, dtype=torch.int64, device=dev)
        lylx[i] = torch.empty(2 * m, dtype=torch.float32, device=dev)
        L.call("arco_up_neighbors", L.ptr(idx[i]), m, *maps[i - 1].shape[2:], *maps[i].shape[2:], L.ptr(idx[i - 1]), L.ptr(lylx[i]))
    (r, ld), m = rv[0], int(idx[0].shape[0])
    k = int(lo.shape[1]) + int(maps[0].shape[1])
    X = torch.empty((m, k), dtype=torch.float32, device=dev)
    L.call(L.h("arco_gather_upcat_rows", r), L.ptr(lo_r), ldlo, *lo.shape[1:], L.ptr(r), ld, *maps[0].shape[1:], L.ptr(idx[0]), m,
           L.ptr(X), k)
    Xs = [X]
    for i in range(1, nl):
        (r, ld), m, c = rv[i], int(idx[i].shape[0]), int(maps[i].shape[1])
        Xp = _fea_rows(X, feas[i - 1], 0)                     # fea_i(x)+x rows
        X = torch.empty((m, k + c), dtype=torch.float32, device=dev)
        L.call(L.h("arco_lerp4_cat_rows", r), L.ptr(Xp), k, k, L.ptr(lylx[i]), L.ptr(r), ld, c, L.ptr(idx[i]), m, L.ptr(X), k + c)
        Xs.append(X)
        k += c
    return Xs, idx, lylx


class LazyHead2dFn(torch.autograd.Function):
    """Row-sparse 2-D head over L = 1, 2 or 3 levels: fea_(5-L) .. fea3 and fea4 are evaluated only where the anchors need them - the 4
    neighbours at the next coarser map of every anchor, the 4 neighbours one map further down of each of those, ...  Inputs (reached
    through lazy_head2d): lo = the dense fea_(4-L)(x)+x and the L finest maps, e.g. L = 3: x1p = fea1(x)+x [B,384,32,32], f2 [B,64,64,64],
    f3 [B,32,128,128], f4 [B,16,256,256] - 16 n rows of 448 channels instead of the 65 536 rows of the dense 64 x 64 map (~1000 anchors
    per step): the dense fea2 GEMM (65 536 x 448 x 64 + the upsampled 117 MB residual), its data and weight gradients and the 64 x 64
    bilinear backward leave the student path.  Rows are bit-identical to the dense modules (same lerp order, same K-order MFMA
    accumulation); d loss / d lo becomes dense again from lo's level down."""

    @staticmethod
    def forward(ctx, lo, w1, w2, pix, *maps_feas):
        nl = len(maps_feas) // 2
        maps, feas = maps_feas[:nl], maps_feas[nl:]
        Xs, idx, lylx = _rows2d(lo, maps, feas, pix)
        h0, h1, a = _q_tail(Xs[-1], feas[-1], w1, w2)
        ctx.save_for_backward(h0, h1, w1, w2, *Xs, *feas, *idx, *lylx)
        ctx.shapes = (tuple(lo.shape),) + tuple(tuple(m.shape) for m in maps)
        ctx.fptrs = tuple(m.data_ptr() for m in maps)
        ctx.fhalf = tuple(m.dtype == torch.float16 for m in maps)      # ops.fm_rows_half: maps consumed as stored
        return a

    @staticmethod
    def backward(ctx, da):
        nl = len(ctx.fptrs)
        h0, h1, w1, w2 = ctx.saved_tensors[:4]
        Xs, feas, idx, lylx = (ctx.saved_tensors[4 + j * nl:4 + (j + 1) * nl] for j in range(4))
        (nb, clo, hlo, wlo), ms = ctx.shapes[0], ctx.shapes[1:]
        dev = da.device
        dX, dw4, dw1, dw2 = _q_tail_bwd(da, Xs[-1], h0, h1, feas[-1], w1, w2)
        dmaps, dws = [None] * nl, [None] * (nl - 1) + [dw4]
        for i in range(nl - 1, 0, -1):
            m, k, c = int(idx[i].shape[0]), int(Xs[i - 1].shape[1]), ms[i][1]
            dXp = torch.empty((4 * m, k), dtype=torch.float32, device=dev)
            buf, done = _fm_grad_buffer(ctx.fhalf[i], ctx.fptrs[i], ms[i], dev)
            _lerp4_cat_rows_bwd(dX, k + c, k, lylx[i], idx[i], m, dXp, buf, c)
            dmaps[i] = done(idx[i], m)
            dws[i - 1] = _wgrad(dXp, Xs[i - 1], feas[i - 1])
            dX = _fea_rows(dXp, feas[i - 1], 1)     # d(fea_i(x)+x)/dx: W^T dy + dy  (residual fused in the dgrad GEMM epilogue)
        m, (c, h, w) = int(idx[0].shape[0]), ms[0][1:]
        dlo = torch.zeros((nb, hlo, wlo, clo), dtype=torch.float32, device=dev)
        buf, done = _fm_grad_buffer(ctx.fhalf[0], ctx.fptrs[0], ms[0], dev)
        _scatter_upcat2d(dX, clo + c, idx[0], m, dlo, clo, hlo, wlo, buf, c, h, w)
        dmaps[0] = done(idx[0], m)
        return (dlo.permute(0, 3, 1, 2), dw1, dw2, None, *(d.permute(0, 3, 1, 2) for d in dmaps), *dws)


def lazy_head2d(lo, maps, fea_weights, q1_weight, q2_weight, pix):
    """Anchor rows of q_representation(FeatureExtractor(...)) at high-res pixel ids `pix`: lo = the dense low-resolution input
    fea_(4-L)(x)+x, maps = the L = 1, 2 or 3 finest feature maps coarse to fine, fea_weights = the L fea weights above lo (the last
    being fea4) - FeatureExtractor.forward_lowres / forward_lowres2 / forward_lowres1 return (lo, *maps)."""
    return LazyHead2dFn.apply(lo, q1_weight, q2_weight, pix, *maps, *fea_weights)


# ---------------------------------------------------------------------------------------------------------------------------
# The 3-D heads.  The 3-D pyramid is not the 2-D one: the two finest maps f3, f4 share a resolution, so everything above the
# 56x56x40 level is per-voxel (fea3, the identity resize, fea4, q_rep) and the join with f4 is a plain row gather.  Two levels
# (maps = f3, f4): one trilinear gather from the dense x2p = fea2(x)+x suffices.  Three levels (maps = f2, f3, f4; round 6), the
# 56x56x40 level lazy too: a sampled voxel needs exactly its EIGHT trilinear corners of x2p = fea2(cat(up(x1p), f2)) + cat(...):
# 8 n rows of 224 channels instead of the dense 501 760-row map (450 MB at the LA size: the step's longest GEMM launch writes it,
# its prototype sums, its resize adjoint, its data and weight gradients read it - for ~1 % of its rows).
# x1p = fea1(...)+... [B,192,28,28,20] stays dense.
# ---------------------------------------------------------------------------------------------------------------------------
def _rows3d(lo, maps, feas, pix):
    """The 3-D row path.  Two levels: X3 = cat(trilinear(lo)[pix], f3[pix]).  Three levels: the corner rows idx8 (at f2's resolution,
    weights w8) of every sampled voxel, X2 = cat(trilinear(lo), f2) on them, X3 = cat(trilinear blend of the eight rows of
    fea2(X2)+X2, f3[pix]).  Both: X4 = cat(fea3(X3)+X3, f4[pix]).  Returns ([X2,] X3, X4), idx8, w8 (None with two levels)."""
    dev = pix.device
    n = int(pix.shape[0])
    three = len(maps) == 3
    lo_r, ldlo = rows_view(lo)
    rv = [rows_view(m) for m in maps]
    at, idx8, w8 = pix, None, None
    if three:
        at = idx8 = torch.empty(8 * n, dtype=torch.int64, device=dev)
        w8 = torch.empty(8 * n, dtype=torch.float32, device=dev)
        L.call("arco_corner_rows3d", L.ptr(pix), n, *maps[0].shape[2:], *maps[1].shape[2:], L.ptr(idx8), L.ptr(w8))
    (r, ld), m = rv[0], int(at.shape[0])
    k = int(lo.shape[1]) + int(maps[0].shape[1])
    X = torch.empty((m, k), dtype=torch.float32, device=dev)
    L.call(L.h("arco_gather_upcat_rows3d", r), L.ptr(lo_r), ldlo, *lo.shape[1:], L.ptr(r), ld, *maps[0].shape[1:], L.ptr(at), m,
           L.ptr(X), k)
    Xs = [X]
    if three:
        (r, ld), c = rv[1], int(maps[1].shape[1])
        Xp = _fea_rows(X, feas[0], 0)
        X = torch.empty((n, k + c), dtype=torch.float32, device=dev)
        L.call(L.h("arco_lerp8_cat_rows3d", r), L.ptr(Xp), k, k, *maps[0].shape[2:], L.ptr(r), ld, *maps[1].shape[1:], L.ptr(pix), n,
               L.ptr(X), k + c)
        Xs.append(X)
        k += c
    (r, ld), c = rv[-1], int(maps[-1].shape[1])
    X4 = torch.empty((n, k + c), dtype=torch.float32, device=dev)
    X4[:, :k] = _fea_rows(X, feas[-2], 0)
    L.call(L.h("arco_gather_rows", r), L.ptr(r), ld, c, None, L.ptr(pix), None, 0, n, L.ptr(X4[:, k:]), k + c)
    return Xs + [X4], idx8, w8


def _scatter_map_rows(src, ld_src, C, idx, n_e, half, ptr, shape, dev):
    """The gradient of a 3-D feature map read as plain rows, dmap[idx[e]] += src[e] in the map's row-gradient buffer (order-independent
    by default, DET_SCATTER); returns the gradient to hand back, channels-last."""
    buf, done = _fm_grad_buffer(half, ptr, shape, dev)
    if DET_SCATTER:
        _det_scatter_rows(src, ld_src, C, 1, idx, None, n_e, buf, C)
    else:
        L.call("arco_scatter_add_rows", L.ptr(src), ld_src, C, None, L.ptr(idx), n_e, None, 1.0, L.ptr(buf), C)
    return done(idx, n_e)


def _det_scatter_corners3d(dX, ldx, clo, at, m, sp_lo, sp_hi, dlo):
    """order-independent adjoint of the trilinear part of arco_gather_upcat_rows3d: dlo += the eight weighted corners of dX[:, :clo]"""
    idx = torch.empty(8 * m, dtype=torch.int64, device=dX.device)
    w = torch.empty(8 * m, dtype=torch.float32, device=dX.device)
    L.call("arco_corner_rows3d", L.ptr(at), m, *sp_lo, *sp_hi, L.ptr(idx), L.ptr(w))
    _det_scatter_rows(dX, ldx, clo, 8, idx, w, 8 * m, dlo, clo)


class LazyHead3dFn(torch.autograd.Function):
    """Row-sparse student head of the 3-D step: q_representation(FeatureExtractor_3d(...)) rows at the sampled voxels only
    (model_3D.py:46-58, train_arco_3d.py:289-296).  Two levels: lo = x2p = fea2(x)+x (dense), maps f3, f4.  Three levels, fea2
    evaluated on rows too: lo = x1p = fea1(.)+. [B,192,28,28,20] (dense), maps f2 [B,32,56,56,40], f3, f4 [B,16,112,112,80]; the
    gradient becomes dense again from the 28x28x20 level down (48 MB).  The maps' gradients are row scatters (order-independent by
    default, DET_SCATTER)."""

    @staticmethod
    def forward(ctx, lo, w1, w2, pix, *maps_feas):
        nl = len(maps_feas) // 2
        maps, feas = maps_feas[:nl], maps_feas[nl:]
        Xs, idx8, w8 = _rows3d(lo, maps, feas, pix)
        h0, h1, a = _q_tail(Xs[-1], feas[-1], w1, w2)
        ctx.save_for_backward(h0, h1, w1, w2, pix, idx8, w8, *Xs, *feas)
        ctx.shapes = (tuple(lo.shape),) + tuple(tuple(m.shape) for m in maps)
        ctx.fptrs = tuple(m.data_ptr() for m in maps)
        ctx.fhalf = tuple(m.dtype == torch.float16 for m in maps)      # ops.fm_rows_half: maps consumed as stored
        return a

    @staticmethod
    def backward(ctx, da):
        nl = len(ctx.fptrs)
        h0, h1, w1, w2, pix, idx8, w8 = ctx.saved_tensors[:7]
        Xs, feas = ctx.saved_tensors[7:7 + nl], ctx.saved_tensors[7 + nl:]
        sl, ms = ctx.shapes[0], ctx.shapes[1:]
        dev = da.device
        n, clo = int(pix.shape[0]), sl[1]
        k3, c3, c4 = int(Xs[-2].shape[1]), ms[-2][1], ms[-1][1]

        def dmap(i, src, ld_src, idx, n_e):
            return _scatter_map_rows(src, ld_src, ms[i][1], idx, n_e, ctx.fhalf[i], ctx.fptrs[i], ms[i], dev)
        dX4, dw4, dw1, dw2 = _q_tail_bwd(da, Xs[-1], h0, h1, feas[-1], w1, w2)
        dX3p = dX4[:, :k3].contiguous()
        df4 = dmap(nl - 1, dX4[:, k3:], k3 + c4, pix, n)
        dw3 = _wgrad(dX3p, Xs[-2], feas[-2])
        dX3 = _fea_rows(dX3p, feas[-2], 1)
        dlo = torch.zeros((sl[0], *sl[2:], clo), dtype=torch.float32, device=dev)
        if nl == 2:
            df3, done = _fm_grad_buffer(ctx.fhalf[0], ctx.fptrs[0], ms[0], dev)
            if DET_SCATTER:
                _det_scatter_corners3d(dX3, k3, clo, pix, n, sl[2:], ms[0][2:], dlo)
                _det_scatter_rows(dX3[:, clo:], k3, c3, 1, pix, None, n, df3, c3)
            else:
                L.call("arco_scatter_upcat_rows3d", L.ptr(dX3), k3, L.ptr(pix), n, L.ptr(dlo), clo, clo, *sl[2:],
                       L.ptr(df3), c3, c3, *ms[0][2:])
            df3 = done(pix, n)
            return (dlo.movedim(-1, 1), dw1, dw2, None, df3.movedim(-1, 1), df4.movedim(-1, 1), dw3, dw4)
        k2, c2 = int(Xs[0].shape[1]), ms[0][1]
        df3 = dmap(1, dX3[:, k2:], k3, pix, n)
        dX2p = torch.empty((8 * n, k2), dtype=torch.float32, device=dev)
        L.call("arco_lerp8_rows3d_bwd", L.ptr(dX3), k3, k2, L.ptr(w8), n, L.ptr(dX2p), k2)
        dw2f = _wgrad(dX2p, Xs[0], feas[0])
        dX2 = _fea_rows(dX2p, feas[0], 1)
        df2 = dmap(0, dX2[:, clo:], k2, idx8, 8 * n)
        if DET_SCATTER:
            _det_scatter_corners3d(dX2, k2, clo, idx8, 8 * n, sl[2:], ms[0][2:], dlo)
        else:       # (the fp32-atomic adjoint of the gather: lo part only - dhi = a scratch row sink of the right shape)
            sink = torch.zeros((ms[0][0], *ms[0][2:], c2), dtype=torch.float32, device=dev)
            L.call("arco_scatter_upcat_rows3d", L.ptr(dX2), k2, L.ptr(idx8), 8 * n, L.ptr(dlo), clo, clo, *sl[2:],
                   L.ptr(sink), c2, c2, *ms[0][2:])
        return (dlo.movedim(-1, 1), dw1, dw2, None, df2.movedim(-1, 1), df3.movedim(-1, 1), df4.movedim(-1, 1), dw2f, dw3, dw4)


def lazy_head3d(lo, maps, fea_weights, q1_weight, q2_weight, pix):
    """Rows of q_representation(FeatureExtractor_3d(...)) at the sampled voxels `pix`: (lo, maps) = what forward_lowres2 (x2p, f3, f4)
    or forward_lowres1 (x1p, f2, f3, f4) returns, fea_weights = the fea weights above lo (the last being fea4)."""
    return LazyHead3dFn.apply(lo, q1_weight, q2_weight, pix, *maps, *fea_weights)


def _class_weights(pl):
    """low-valid bits of every pixel as float rows [n_pix, Cp] (Cp = C padded to 4)."""
    Cp = _ceil(pl.C, 4)
    wm = torch.empty((pl.n_pix, Cp), dtype=torch.float32, device=pl.dev)
    L.call("arco_lv_weights", L.ptr(pl.codes), pl.n_pix, pl.C, Cp, L.ptr(wm))
    return wm, Cp


def _wsum(rows, ld, wt, ldw, n_rows, C, D, totals, out, ldo):
    ws = torch.empty(L.query("arco_proto_ws_floats", n_rows, C, D), dtype=torch.float32, device=rows.device)
    fn = L.h("arco_weighted_row_sum", rows)      # (f16 activation storage)
    L.call(fn, L.ptr(rows), ld, L.ptr(wt), ldw, n_rows, C, D, L.ptr(totals), L.ptr(ws), L.ptr(out), ldo)


class LazyTeacher:
    """Teacher side of the 2-D and 3-D steps without the dense 496-channel tensor, for (lo, maps, fea weights) as the student heads of
    either rank take them (model_2D.py:51-53, model_3D.py:46-58).  Every map is linear in the feature maps, so
        prototype_c = W4 . cat((W3+I) . cat((W2+I) . cat(S(lo; w''), S(f2; w')), S(f3; w)), S(f4; w))         (three levels)
    with S(t; w) = the class-weighted row sums (class means) of t and the class mask w pushed through the resize adjoint once per change
    of resolution below the finest map (2-D, three levels: 256^2 -> 128^2 -> 64^2 -> 32^2, the weighted row sums reading 66 MB
    instead of the dense 117 MB fea2 output, which is not built at all; 3-D: f3 shares f4's resolution and its mask).  Key rows are
    evaluated at the key pixels only, through the student's row path."""

    def __init__(self, lo, maps, fea_weights):
        self.lo, self.maps, self.feas = lo, list(maps), list(fea_weights)

    @torch.no_grad()
    def prototypes(self, pl):
        ts = [self.lo, *self.maps]
        rv = [rows_view(t) for t in ts]
        nb, C = int(self.lo.shape[0]), pl.C
        wm, Cp = _class_weights(pl)
        wts = [(wm, pl.n_pix)]              # (class-weight rows, row count) of every tensor, walking from the finest map down
        for t, fine in zip(ts[-2::-1], ts[:0:-1]):
            sp, sp_fine = tuple(t.shape[2:]), tuple(fine.shape[2:])
            if sp == sp_fine:
                wts.append(wts[-1])
                continue
            w = torch.empty((nb * math.prod(sp), Cp), dtype=torch.float32, device=pl.dev)
            if len(sp) == 2:
                L.call("arco_bilinear_bwd", L.ptr(wts[-1][0]), Cp, nb, *sp, Cp, *sp_fine, L.ptr(w), Cp, 0)
            else:
                L.call("arco_trilinear_bwd", L.ptr(wts[-1][0]), Cp, nb, *sp, Cp, *sp_fine, L.ptr(w), Cp)
            wts.append((w, int(w.shape[0])))
        wts.reverse()
        R = _ceil(C, 16)
        cs = [int(t.shape[1]) for t in ts]

        def wsum(i, out, ldo):
            (r, ld), (w, n_t) = rv[i], wts[i]
            _wsum(r, ld, w, Cp, n_t, C, cs[i], pl.totals, out, ldo)
        k = cs[0] + cs[1]
        S = torch.zeros((R, k), dtype=torch.float32, device=pl.dev)            # lo and the coarsest map share the first block
        wsum(0, S, k)
        wsum(1, S[:, cs[0]:], k)
        for i in range(2, len(ts)):                                            # every finer map joins fea_i(S)+S
            Sn = torch.zeros((R, k + cs[i]), dtype=torch.float32, device=pl.dev)
            Sn[:, :k] = _fea_rows(S, self.feas[i - 2], 0)
            wsum(i, Sn[:, k:], k + cs[i])
            S, k = Sn, k + cs[i]
        return _gemm(S, self.feas[-1])[:C].contiguous()

    @torch.no_grad()
    def rows(self, pix):
        rows = _rows2d if self.lo.dim() == 4 else _rows3d
        return _gemm(rows(self.lo, self.maps, self.feas, pix)[0][-1], self.feas[-1])
