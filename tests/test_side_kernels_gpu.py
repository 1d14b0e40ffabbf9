"""The 3-D side kernels of csrc/elementwise.hip, the 2-D adjoints, the layout and optimiser kernels, all of csrc/det_scatter.hip and
the two casts of csrc/conv_h.hip called DIRECTLY (arco_amd._lib), one entry point per test, against a plain float64 / int64 reference
on the CPU computed from the same input values (tests/side_kernel_refs.py) - not through ops.py / head.py, a golden file or another
HIP route.  Every output buffer is prefilled with a sentinel: the pad columns of a padded stride, the columns around a channel-slice
operand and GUARD elements behind the buffer must keep it.  Every toleranced test prints its worst err / bound and asserts <= 1.

  exact (torch.equal; on integer views where NaN bit patterns matter): arco_s2d3 (both directions, words and f16 pairs),
  arco_d2s3_add(_h), arco_copy_rows, the two layout transposes, arco_put_rows, arco_row_nonzero, arco_cast_h2f / arco_cast_f2h
  (arco_cast_f2h saturates: +-inf and everything above 65504 after scaling become +-65504, NaN stays NaN), arco_det_absmax,
  the indices AND weight bits of arco_corner_rows3d / arco_corner_rows2d / arco_up_neighbors against a numpy float32 restatement,
  the hi part of the gathers, the rows of arco_gather_upcat_rows3d against the dense arco_trilinear_fwd, arco_lerp8_cat_rows3d
  against the gather, arco_lerp8_rows3d_bwd and the dV of arco_lerp4_cat_rows_bwd against the fp32 product, and the fixed-point
  chain arco_det_absmax -> arco_det_scatter_rows -> arco_det_finish_rows -> arco_det_clear_rows against its int64 restatement.

  per-element bounds (u = 2^-24; derivations in tests/side_kernel_refs.py; worst err / bound: CPU emulation | GPU)
  * arco_trilinear_fwd        0.34 | 0.34   arco_gather_upcat_rows3d(_h) 0.24 | 0.24   arco_lerp8_cat_rows3d(_h) 0.24 | 0.24
  * arco_trilinear_bwd        0.22 | 0.22   arco_lerp8_rows3d_bwd        1.00 | 1.00   arco_lerp4_cat_rows_bwd   dV 1.00 | 1.00  dhi 0.20 | 0.20
  * arco_scatter_upcat_rows3d dlo 0.33 | 0.33  dhi 0.18 | 0.18           arco_scatter_upcat_rows   dlo 0.31 | 0.31  dhi 0.20 | 0.20
  * arco_sgd_nesterov / arco_sgd_momentum   buf 0.48 | 0.47   p 0.50 | 0.50           arco_ema 1.00 | 1.00
  * the fixed-point chain against float64 (n_r 2^-45 max|src| + u |sum|, times |alpha|)   1.00 | 1.00 (0.995, small_rows);
    alpha = -3, with the rounding of its last multiplication added   0.86 | 0.86
  * corner weights against the exact coordinate: coordinate / (4 S u) 0.07 | 0.07, weight sum / (4 u) 0.19 | 0.19
The emulation's figures are the largest printed by tests/test_side_kernels_cpu.py, the GPU's the largest printed by this file on
an MI355X.  A ratio of 1.00 is a single rounding against u |ref| (the two weight products: one multiplication, bit for bit the
fp32 product) or the half unit of the fixed-point scale against 2^-45 max|src| (the small-valued rows of the chain).  arco_ema's
bound, gamma(2) |k m| + gamma(3) |q (1 - m)|, covers two or three roundings; its 1.00 (m = 0.999, one element among 4096 x 256 + 1,
k = 1.00107) is the rounding of the product k m at 0.9997 u |k m| and the rounding of the sum at 0.993 u |sum|, both at their worst
and in the same direction, beside a q (1 - m) term 6e-5 of k m: the bound is rigorous and attained.
arco_ema reads 1.00 | 1.00 to two places (0.997).  The coordinate check of the corner kernels sits at 0.07 of the issue's 4 S u: S is the largest side, the error grows with the coordinate itself, and the roundings do
not line up; what binds there is the bit comparison with the float32 restatement, which every case passes on the GPU (indices and
weight bits of all three kernels), so that no cause had to be sought for a difference."""
import numpy as np
import pytest
import torch

import side_kernel_refs as R
from loss_kernel_refs import SENTINEL, exact, worst
from side_kernel_refs import GUARD, bits_equal, body, check_corners, cols, sent

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAG_SENT = 249


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def filled(n, dtype=torch.float32, value=None):
    """n elements + GUARD, all holding the sentinel"""
    return torch.full((int(n) + GUARD,), sent(dtype) if value is None else value, dtype=dtype, device=DEV)


def put(t, ld=None, off=0, zero=False):
    """[rows, C] CPU tensor -> (device buffer of rows x ld + GUARD sentinels with t at columns off .. off + C, the operand's
    pointer-carrying view).  None for an operand of no columns and no stride."""
    rows, C = t.shape
    ld = C if ld is None else ld
    assert off + C <= ld or rows == 0
    if ld == 0:
        return None, None
    buf = torch.full((rows * ld + GUARD,), sent(t.dtype), dtype=t.dtype)
    buf[:rows * ld].view(rows, ld)[:, off:off + C] = 0 if zero else t
    buf = buf.to(DEV)
    return buf, buf[off:]


def report(name, ratio):
    print(f"{name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def held(name, got, ref, tol):
    report(name, worst(got, ref, tol))


def ids(cases):
    return lambda i: "-".join(str(v) for v in cases[i]).replace(" ", "")


# ---- (1) space-to-depth / depth-to-space ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", (0, 1))
@pytest.mark.parametrize("i", range(len(R.S2D_CASES)), ids=ids(R.S2D_CASES))
def test_s2d3(L, i, direction):
    """a permutation of 4-byte words: random bit patterns (NaN payloads, -0.0) arrive unchanged; kind 'h' is the form ops._s2d3 uses
    for f16 tensors (half the channel count and half the stride)"""
    c = R.s2d_case(i)
    q, rows, C, ldv, ldp = c["rows"] // 8, c["rows"], c["c"], c["ldv"], c["ldp"]
    if direction == 0:
        vb, v = put(c["V"], ldv)
        pb = filled(q * ldp, torch.int32)
        p = pb
    else:
        pb, p = put(c["P"], ldp)
        vb = filled(rows * ldv, torch.int32)
        v = vb
    L.call("arco_s2d3", L.ptr(v), ldv, c["nv"], c["x2"], c["y2"], c["z2"], C, L.ptr(p), ldp, direction)
    got, ok = cols(pb, q, ldp, 0, 8 * C) if direction == 0 else cols(vb, rows, ldv, 0, C)
    assert ok and exact(got, c["P"] if direction == 0 else c["V"])
    print(f"s2d3 case {i} dir {direction}: exact")


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.D2S_CASES)), ids=ids(R.D2S_CASES))
def test_d2s3_add(L, i, half):
    c = R.d2s_case(i, half)
    C, pad, rows = c["c"], c["pad"], c["rows"]
    _, p = put(c["P"], 8 * C + pad)
    _, a = put(c["A"], C + pad)
    vb = filled(rows * (C + pad), c["P"].dtype)
    L.call("arco_d2s3_add_h" if half else "arco_d2s3_add", L.ptr(p), 8 * C + pad, c["nv"], c["x2"], c["y2"], c["z2"], C, L.ptr(a), C + pad,
           L.ptr(vb), C + pad)
    got, ok = cols(vb, rows, C + pad, 0, C)
    assert ok and exact(got, c["ref"])
    print(f"d2s3_add case {i} half {half}: exact")


# ---- (2) trilinear resize, dense -----------------------------------------------------------------------------------------------------------
def run_tri_fwd(L, c):
    C, lo, hi = c["C"], c["lo"], c["hi"]
    rows = c["nv"] * int(np.prod(hi))
    _, x = put(c["X"].view(-1, C), C + c["px"])
    yb = filled(rows * (C + c["py"]))
    L.call("arco_trilinear_fwd", L.ptr(x), C + c["px"], c["nv"], *lo, C, *hi, L.ptr(yb), C + c["py"])
    got, ok = cols(yb, rows, C + c["py"], 0, C)
    assert ok
    return got


def run_tri_bwd(L, c):
    C, lo, hi = c["C"], c["lo"], c["hi"]
    rows = c["nv"] * int(np.prod(lo))
    _, dy = put(c["dY"].view(-1, C), C + c["py"])
    xb = filled(rows * (C + c["px"]))
    L.call("arco_trilinear_bwd", L.ptr(dy), C + c["py"], c["nv"], *lo, C, *hi, L.ptr(xb), C + c["px"])
    got, ok = cols(xb, rows, C + c["px"], 0, C)
    assert ok
    return got


@pytest.mark.parametrize("i", range(len(R.TRI_CASES)), ids=ids(R.TRI_CASES))
def test_trilinear_fwd(L, i):
    c = R.tri_case(i)
    got = run_tri_fwd(L, c)
    held(f"trilinear fwd case {i}", got.view(c["ref"].shape), c["ref"], c["tol"])
    if c["lo"] == c["hi"]:
        assert exact(got.view(c["X"].shape), c["X"])                                              # the identity, bit for bit


def test_trilinear_fwd_second_grid_trip(L):
    c = R.tri_big(False)
    held("trilinear fwd 4096 x 256 + 1 voxels", run_tri_fwd(L, c).view(c["ref"].shape), c["ref"], c["tol"])


@pytest.mark.parametrize("i", range(len(R.TRI_CASES)), ids=ids(R.TRI_CASES))
def test_trilinear_bwd(L, i):
    c = R.tri_case(i)
    got = run_tri_bwd(L, c).view(c["dX"].shape)
    held(f"trilinear bwd case {i}", got, c["dX"], c["tol_b"])
    assert bool((got[(c["cnt"] == 0).view(1, *c["lo"], 1).expand_as(got)] == 0).all())            # unreferenced voxels: zero


def test_trilinear_bwd_second_grid_trip(L):
    c = R.tri_big(True)
    held("trilinear bwd 4096 x 256 + 1 voxels", run_tri_bwd(L, c).view(c["dX"].shape), c["dX"], c["tol_b"])


# ---- (3) row kernels -----------------------------------------------------------------------------------------------------------------------
def run_rows(L, c, name, half, first):
    """arco_gather_upcat_rows3d / arco_lerp8_cat_rows3d (first = the lo map or the corner rows V)"""
    Clo, Chi, n, pad, off = c["Clo"], c["Chi"], c["n"], c["pad"], c["off"]
    lda, ldh, ldx = (Clo + pad if Clo else 0), (Chi + pad if Chi else 0), Clo + Chi + pad
    _, a = put(first, lda, off if Clo else 0)
    hi = c["HI162"] if half else c["HI2"]
    _, h = put(hi, ldh, off if Chi else 0)
    xb = filled(n * ldx)
    pix = dev(c["pix"])
    L.call(name + ("_h" if half else ""), L.ptr(a), lda, Clo, *c["lo"], L.ptr(h), ldh, Chi, *c["hi"], L.ptr(pix), n, L.ptr(xb), ldx)
    got, ok = cols(xb, n, ldx, 0, Clo + Chi)
    assert ok
    return got


def check_rows(name, c, got, half):
    Clo = c["Clo"]
    assert exact(got[:, Clo:], c["hi16_rows"] if half else c["hi_rows"])                          # a copy / an exact widening
    if Clo:
        held(name, got[:, :Clo], c["ref_lo"], c["tol_lo"])


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.ROW_CASES)), ids=ids(R.ROW_CASES))
def test_gather_upcat_rows3d(L, i, half):
    c = R.row_case(i)
    got = run_rows(L, c, "arco_gather_upcat_rows3d", half, c["LO2"])
    check_rows(f"gather_upcat_rows3d case {i} half {half}", c, got, half)
    if c["Clo"] and not half:                                                                     # the rows of the dense resize, bit for bit
        d = dict(C=c["Clo"], lo=c["lo"], hi=c["hi"], nv=R.NV, X=c["LO"], px=0, py=0)
        assert bits_equal(got[:, :c["Clo"]], run_tri_fwd(L, d)[c["pix"]])


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.ROW_CASES)), ids=ids(R.ROW_CASES))
def test_lerp8_cat_rows3d(L, i, half):
    c = R.row_case(i)
    got = run_rows(L, c, "arco_lerp8_cat_rows3d", half, c["V"])
    check_rows(f"lerp8_cat_rows3d case {i} half {half}", c, got, half)
    if c["Clo"] and not half:                                                                     # the gather's blend of the same corner rows
        assert bits_equal(got, run_rows(L, c, "arco_gather_upcat_rows3d", half, c["LO2"]))


@pytest.mark.parametrize("i", range(len(R.ROW_CASES)), ids=ids(R.ROW_CASES))
def test_lerp8_rows3d_bwd(L, i):
    c = R.lerp_bwd_case(i, 3)
    Clo, n, pad = c["Clo"], c["n"], c["pad"]
    ldx, ldv = Clo + c["Chi"] + pad, Clo + pad
    _, dx = put(c["dX"], ldx)
    w8 = dev(c["w"])
    vb = filled(8 * n * ldv)
    L.call("arco_lerp8_rows3d_bwd", L.ptr(dx), ldx, Clo, L.ptr(w8), n, L.ptr(vb), ldv)
    got, ok = cols(vb, 8 * n, ldv, 0, Clo) if ldv else (torch.zeros((8 * n, 0)), True)
    assert ok
    held(f"lerp8_rows3d_bwd case {i}", got, c["ref"], c["tol"])
    assert bits_equal(got, c["emu"])                                                              # one IEEE multiplication


def run_scatter(L, c, which):
    """arco_scatter_upcat_rows3d / arco_scatter_upcat_rows / arco_lerp4_cat_rows_bwd on zeroed destinations inside sentinel pads"""
    Clo, Chi, n, pad, off = c["Clo"], c["Chi"], c["n"], c["pad"], c["off"]
    Mlo, Mhi = R.NV * int(np.prod(c["lo"])), R.NV * int(np.prod(c["hi"]))
    ldx, ldl, ldh = Clo + Chi + pad, (Clo + pad if Clo else 0), (Chi + pad if Chi else 0)
    _, dx = put(c["dX"], ldx)
    pix = dev(c["pix"])
    hb, h = put(torch.zeros((Mhi, Chi)), ldh, off if Chi else 0, zero=True)
    out = {}
    if which == "lerp4":
        ldv = Clo + pad
        vb = filled(4 * n * ldv)
        lylx = dev(c["lylx"])
        L.call("arco_lerp4_cat_rows_bwd", L.ptr(dx), ldx, Clo, L.ptr(lylx), L.ptr(pix), n, L.ptr(vb), ldv, L.ptr(h), ldh, Chi)
        out["dV"], ok = cols(vb, 4 * n, ldv, 0, Clo) if ldv else (torch.zeros((4 * n, 0)), True)
        assert ok
    else:
        lb, l = put(torch.zeros((Mlo, Clo)), ldl, off if Clo else 0, zero=True)
        L.call(which, L.ptr(dx), ldx, L.ptr(pix), n, L.ptr(l), ldl, Clo, *c["lo"], L.ptr(h), ldh, Chi, *c["hi"])
        if Clo:
            out["dlo"], ok = cols(lb, Mlo, ldl, off, Clo)
            assert ok
    if Chi:
        out["dhi"], ok = cols(hb, Mhi, ldh, off, Chi)
        assert ok
    return out


def check_scatter(name, c, out):
    if "dlo" in out:
        held(name + " dlo", out["dlo"], c["dlo"], c["tol_lo"])
    if "dhi" in out:
        held(name + " dhi", out["dhi"], c["dhi"], c["tol_hi"])


@pytest.mark.parametrize("i", range(len(R.ROW_CASES)), ids=ids(R.ROW_CASES))
def test_scatter_upcat_rows3d(L, i):
    c = R.scatter_case(i, 3)
    check_scatter(f"scatter_upcat_rows3d case {i}", c, run_scatter(L, c, "arco_scatter_upcat_rows3d"))


@pytest.mark.parametrize("i", range(len(R.ROW_CASES)), ids=ids(R.ROW_CASES))
def test_scatter_upcat_rows(L, i):
    c = R.scatter_case(i, 2)
    check_scatter(f"scatter_upcat_rows case {i}", c, run_scatter(L, c, "arco_scatter_upcat_rows"))


@pytest.mark.parametrize("i", range(len(R.ROW_CASES)), ids=ids(R.ROW_CASES))
def test_lerp4_cat_rows_bwd(L, i):
    c = R.scatter_case(i, 2)
    out = run_scatter(L, c, "lerp4")
    held(f"lerp4_cat_rows_bwd case {i} dV", out["dV"], c["ref"], c["tol"])
    assert bits_equal(out["dV"], c["emu"])
    check_scatter(f"lerp4_cat_rows_bwd case {i}", c, out)


# ---- (4) corner indices and weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CORNER_CASES)), ids=ids(R.CORNER_CASES))
def test_corner_rows3d(L, i):
    c = R.corner_case(i, 3)
    n = c["n"]
    pix, ib, wb = dev(c["pix"]), filled(8 * n, torch.int64), filled(8 * n)
    L.call("arco_corner_rows3d", L.ptr(pix), n, *c["lo"], *c["hi"], L.ptr(ib), L.ptr(wb))
    check_corners(f"corner_rows3d case {i}", c, body(ib, 8 * n), body(wb, 8 * n))


@pytest.mark.parametrize("i", range(len(R.CORNER_CASES)), ids=ids(R.CORNER_CASES))
def test_corner_rows2d(L, i):
    c = R.corner_case(i, 2)
    n = c["n"]
    pix, ib, wb = dev(c["pix"]), filled(4 * n, torch.int64), filled(4 * n)
    L.call("arco_corner_rows2d", L.ptr(pix), n, *c["lo"], *c["hi"], L.ptr(ib), L.ptr(wb))
    check_corners(f"corner_rows2d case {i}", c, body(ib, 4 * n), body(wb, 4 * n))


@pytest.mark.parametrize("i", range(len(R.CORNER_CASES)), ids=ids(R.CORNER_CASES))
def test_up_neighbors(L, i):
    c = R.corner_case(i, 2)
    n = c["n"]
    pix, ib, lb = dev(c["pix"]), filled(4 * n, torch.int64), filled(2 * n)
    L.call("arco_up_neighbors", L.ptr(pix), n, *c["lo"], *c["hi"], L.ptr(ib), L.ptr(lb))
    nb4, lylx = body(ib, 4 * n), body(lb, 2 * n)
    l = lylx.view(n, 2).numpy()
    h = (np.float32(1) - l).astype(np.float32)
    w = np.stack([h[:, 0] * h[:, 1], h[:, 0] * l[:, 1], l[:, 0] * h[:, 1], l[:, 0] * l[:, 1]], 1).astype(np.float32)
    r_coord, r_sum, inside = R.corner_property(nb4.view(n, 4).numpy(), w, c["cn"])
    print(f"up_neighbors case {i}: coordinate err / (4 S u) {r_coord:.3f}, weight-sum err / (4 u) {r_sum:.3f}")
    assert inside and r_coord <= 1.0 and r_sum <= 1.0
    assert exact(nb4, c["idx"]) and bits_equal(lylx, c["lylx"])


# ---- (5) copies, transposes, put_rows, row_nonzero, casts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("i", range(len(R.COPY_CASES)), ids=ids(R.COPY_CASES))
def test_copy_rows(L, i, accumulate):
    c = R.copy_case(i)
    M, C, ldx, ldy = c["M"], c["C"], c["C"] + c["px"], c["C"] + c["py"]
    _, x = put(c["X"], ldx)
    yb, y = put(c["Y0"], ldy)
    L.call("arco_copy_rows", L.ptr(x), ldx, M, C, L.ptr(y), ldy, accumulate)
    got, ok = cols(yb, M, ldy, 0, C)
    assert ok and exact(got, c["acc"] if accumulate else c["X"])                                  # accumulate: one fp32 add
    print(f"copy_rows case {i} accumulate {accumulate}: exact")


@pytest.mark.parametrize("i", range(len(R.TRANS_CASES)), ids=ids(R.TRANS_CASES))
def test_nchw_to_nhwc(L, i):
    c = R.trans_case(i)
    NB, C, Pn, ld = c["NB"], c["C"], c["P"], c["C"] + c["pad"]
    x, yb = dev(c["nchw"]), filled(NB * Pn * ld)
    L.call("arco_nchw_to_nhwc", L.ptr(x), NB, C, Pn, L.ptr(yb), ld)
    got, ok = cols(yb, NB * Pn, ld, 0, C)
    assert ok and exact(got, c["nhwc"].view(NB * Pn, C))


@pytest.mark.parametrize("i", range(len(R.TRANS_CASES)), ids=ids(R.TRANS_CASES))
def test_nhwc_to_nchw(L, i):
    c = R.trans_case(i)
    NB, C, Pn, ld = c["NB"], c["C"], c["P"], c["C"] + c["pad"]
    _, x = put(c["nhwc"].view(NB * Pn, C), ld)
    yb = filled(NB * C * Pn)
    L.call("arco_nhwc_to_nchw", L.ptr(x), ld, NB, C, Pn, L.ptr(yb))
    assert exact(body(yb, NB * C * Pn, (NB, C, Pn)), c["nchw"])


@pytest.mark.parametrize("i", range(len(R.PUT_CASES)), ids=ids(R.PUT_CASES))
def test_put_rows(L, i):
    c = R.put_case(i)
    n, C, M = c["n"], c["C"], c["M"]
    _, s = put(c["src"], c["lds"])
    idx, db = dev(c["idx"]), filled(M * c["ldd"])
    L.call("arco_put_rows", L.ptr(s), c["lds"], C, L.ptr(idx), n, L.ptr(db), c["ldd"])
    got, ok = cols(db, M, c["ldd"], 0, C)
    assert ok and exact(got, c["ref"])                                                            # unnamed rows keep the sentinel


def test_row_nonzero(L):
    c = R.nonzero_case()
    _, x = put(c["X"], c["ld"])
    fb = torch.full((c["M"] + GUARD,), FLAG_SENT, dtype=torch.uint8, device=DEV)
    L.call("arco_row_nonzero", L.ptr(x), c["ld"], c["C"], c["M"], L.ptr(fb))
    torch.cuda.synchronize()
    got = fb.cpu()
    assert bool((got[c["M"]:] == FLAG_SENT).all()) and exact(got[:c["M"]], c["ref"])


@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_h2f(L, n):
    c = R.cast_case(n)
    x, yb = dev(c["h"]), filled(n)
    L.call("arco_cast_h2f", L.ptr(x), n, L.ptr(yb))
    assert R.same_or_nan(body(yb, n), c["h2f"])


@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_f2h(L, n):
    """(x * scale) saturated at +-65504 and rounded to f16 as the CPU rounds it: what the kernel does today with values above 65504
    after scaling and with +-inf is +-65504 (a clipped gradient, not an inf); NaN stays NaN."""
    c = R.cast_case(n)
    x, yb = dev(c["x"]), filled(n, torch.float16)
    L.call("arco_cast_f2h", L.ptr(x), n, R.CAST_SCALE, L.ptr(yb))
    assert R.same_or_nan(body(yb, n), c["f2h"])


# ---- (6) optimiser steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nesterov", (True, False), ids=("nesterov", "momentum"))
@pytest.mark.parametrize("i", range(len(R.OPT_CASES)), ids=ids(R.OPT_CASES))
def test_sgd(L, i, nesterov):
    c = R.opt_case(i, nesterov)
    n = c["n"]
    pb, bb = filled(n), filled(n)
    pb[:n], bb[:n] = dev(c["p"]), dev(c["buf"])
    g = dev(c["g"])
    L.call("arco_sgd_nesterov" if nesterov else "arco_sgd_momentum", L.ptr(pb), L.ptr(g), L.ptr(bb), n, c["lr"], c["mom"], c["wd"], c["first"])
    held(f"sgd nesterov {nesterov} case {i} buf", body(bb, n), c["ref_b"], c["tol_b"])
    held(f"sgd nesterov {nesterov} case {i} p", body(pb, n), c["ref_p"], c["tol_p"])


@pytest.mark.parametrize("i", range(len(R.EMA_CASES)), ids=ids(R.EMA_CASES))
def test_ema(L, i):
    c = R.ema_case(i)
    n = c["n"]
    kb = filled(n)
    kb[:n] = dev(c["k"])
    q = dev(c["q"])
    L.call("arco_ema", L.ptr(kb), L.ptr(q), n, c["m"])
    got = body(kb, n)
    held(f"ema case {i}", got, c["ref"], c["tol"])
    if c["m"] == 1.0:
        assert exact(got, c["k"])
    if c["m"] == 0.0:
        assert exact(got, c["q"])


# ---- (7) det_scatter.hip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.ABSMAX_CASES)), ids=ids(R.ABSMAX_CASES))
def test_det_absmax(L, i):
    c = R.absmax_case(i)
    _, x = put(c["x"], c["ld"])
    mb = filled(1, torch.int32)
    L.call("arco_det_absmax", L.ptr(x), c["ld"], c["C"], c["n"], L.ptr(mb))
    assert int(body(mb, 1)[0]) & 0xffffffff == c["bits"]


@pytest.mark.parametrize("i", range(len(R.DET_CASES)), ids=lambda i: R.DET_CASES[i][0])
def test_det_chain(L, i):
    """absmax -> scatter -> finish -> clear against the int64 restatement: the accumulator after the scatter, the destination after
    finish (bit for bit; rows that no entry names keep the sentinel, and so do all rows of an all-zero source), the accumulator
    after clear (zero).  On top, every finite case is held to float64: |alpha| (n_r 2^-45 max|src| + u |sum|), plus the rounding of
    the last multiplication where alpha is no power of two (alpha = -3)."""
    c = R.det_case(i)
    C, M, n_e, lda = c["C"], c["M"], c["n_e"], c["ld_acc"]
    ldd = C + 4
    _, src = put(c["src"], C + 4)
    ab, acc = put(torch.zeros((M, C), dtype=torch.int64), lda, zero=True)
    idx, lst, w = dev(c["idx"]), dev(c["lst"]), dev(c["w"])
    mb, db = filled(1, torch.int32), filled(M * ldd)
    L.call("arco_det_absmax", L.ptr(src), C + 4, C, c["n_src"], L.ptr(mb))
    assert int(body(mb, 1)[0]) & 0xffffffff == c["mb"]
    L.call("arco_det_scatter_rows", L.ptr(src), C + 4, C, c["div"], L.ptr(lst), L.ptr(idx), L.ptr(w), n_e, L.ptr(acc), lda, L.ptr(mb))
    got, ok = cols(ab, M, lda, 0, C)
    assert ok and exact(got, c["acc"])
    L.call("arco_det_finish_rows", L.ptr(lst), L.ptr(idx), n_e, L.ptr(acc), lda, C, L.ptr(mb), c["alpha"], L.ptr(db), ldd)
    dst, ok = cols(db, M, ldd, 0, C)
    t = c["touched"]
    assert ok and bool((dst[~t] == SENTINEL).all())
    if c["kind"] == "nan":
        assert bool((dst[t].view(torch.int32) == 0x7fc00000).all())
    elif c["kind"] == "zero":
        assert bool((dst[t] == SENTINEL).all())
    else:
        assert bits_equal(dst[t], c["dst"][t])
        held(f"det chain {c['name']}", dst[t], c["ref64"][t], c["tol64"][t])
    L.call("arco_det_clear_rows", L.ptr(lst), L.ptr(idx), n_e, L.ptr(acc), lda, C)
    got, ok = cols(ab, M, lda, 0, C)
    assert ok and bool((got == 0).all())


@pytest.mark.parametrize("i", (1, 2, 4), ids=lambda i: R.DET_CASES[i][0])
def test_det_finish_and_clear_alone(L, i):
    """arco_det_finish_rows and arco_det_clear_rows on the REFERENCE's accumulator and maximum: each held without the scatter in
    front of it.  Rows that no entry names keep their accumulator (here a marker) through clear."""
    c = R.det_case(i)
    C, M, n_e, lda, ldd = c["C"], c["M"], c["n_e"], c["ld_acc"], c["C"] + 4
    t = c["touched"]
    a0 = c["acc"].clone()
    a0[~t] = 12345
    ab, acc = put(a0, lda)
    idx, lst = dev(c["idx"]), dev(c["lst"])
    mb = dev(torch.tensor([c["mb"]], dtype=torch.int64).to(torch.int32))
    db = filled(M * ldd)
    L.call("arco_det_finish_rows", L.ptr(lst), L.ptr(idx), n_e, L.ptr(acc), lda, C, L.ptr(mb), c["alpha"], L.ptr(db), ldd)
    dst, ok = cols(db, M, ldd, 0, C)
    assert ok and bool((dst[~t] == SENTINEL).all()) and bits_equal(dst[t], c["dst"][t])
    L.call("arco_det_clear_rows", L.ptr(lst), L.ptr(idx), n_e, L.ptr(acc), lda, C)
    got, ok = cols(ab, M, lda, 0, C)
    assert ok and bool((got[t] == 0).all()) and bool((got[~t] == 12345).all())
