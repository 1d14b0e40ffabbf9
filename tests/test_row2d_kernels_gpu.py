"""The 2-D row-sparse head kernels and the small step utilities of csrc/elementwise.hip called DIRECTLY (arco_amd._lib), one entry point
per test, against a plain float64 reference on the CPU computed from the same input values (tests/row2d_kernel_refs.py) - not
through head.py / ops.py or another HIP route.  Every output buffer is prefilled with a sentinel: the pad columns of a padded
stride, the columns around a channel-slice operand, rows that no index names and GUARD elements behind the buffer must keep it.

  exact: the hi part of arco_gather_upcat_rows(_h) / arco_lerp4_cat_rows(_h) (an fp32 copy, an f16 value widened); the rows of
  arco_gather_upcat_rows against the dense arco_bilinear_fwd, bit for bit; arco_lerp4_cat_rows against the gather, bit for bit, given
  the neighbour rows and (ly, lx) that arco_up_neighbors produced on the GPU; arco_zero_rows(_h); arco_cast_rows_f2h ((x * scale)
  saturated at +-65504 - +-inf included - then rounded to nearest even; NaN stays NaN, -0.0 stays -0.0); arco_fold_residual /
  arco_unfold_residual (either gradient block null); arco_combine_terms_bwd against the fp32 product.

  per-element bounds (u = 2^-24; derivations in tests/row2d_kernel_refs.py; worst err / bound: CPU emulation | GPU)
  * arco_gather_upcat_rows(_h)  lo part against float64 bilinear, side_kernel_refs.blend_tol   0.21 | 0.21
  * arco_lerp4_cat_rows(_h)     the same                                                       0.21 | 0.21
  * arco_combine_terms          (n + 1) u sum|w_i t_i| against the float64 sum                 0.05 | 0.05
The emulation's figures are the largest printed by tests/test_row2d_kernels_cpu.py (over both of its forms, every operation rounded
and every product-sum fused), the GPU's the largest printed by this file on an MI355X.

The bit comparisons found one disagreement, fixed in the kernels: written as the plain expression hy (hx v00 + lx v01) + ly (hx v10 +
lx v11), the dense resize, the gather and the 4-way lerp compiled to three different chains of multiplies and fused multiply-adds -
the gather's rows differed from the dense resize's in the last bit on 0.5 % of the elements, the lerp's from the gather's on 14 % -
although each was far inside the float64 bound.  All three now evaluate bl_blend1 (csrc/interp.h), one explicit chain."""
import ctypes

import pytest
import torch

import row2d_kernel_refs as R2
import side_kernel_refs as R
from loss_kernel_refs import exact, worst
from side_kernel_refs import GUARD, bits_equal, body, cols, sent

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def filled(n, dtype=torch.float32):
    """n elements + GUARD, all holding the sentinel"""
    return torch.full((int(n) + GUARD,), sent(dtype), dtype=dtype, device=DEV)


def put(t, ld=None, off=0):
    """[rows, C] CPU tensor -> (device buffer of rows x ld + GUARD sentinels with t at columns off .. off + C, the operand's
    pointer-carrying view).  None for an operand of no columns and no stride."""
    rows, C = t.shape
    ld = C if ld is None else ld
    assert off + C <= ld or rows == 0
    if ld == 0:
        return None, None
    buf = torch.full((rows * ld + GUARD,), sent(t.dtype), dtype=t.dtype)
    buf[:rows * ld].view(rows, ld)[:, off:off + C] = t
    buf = buf.to(DEV)
    return buf, buf[off:]


def report(name, ratio):
    print(f"{name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def ids(cases):
    return lambda i: "-".join(str(v) for v in cases[i]).replace(" ", "")


# ---- (1) arco_gather_upcat_rows(_h), arco_lerp4_cat_rows(_h) ---------------------------------------------------------------------------------
def run_rows(L, c, lerp4, half, lylx=None, V=None):
    """the gather (first operand: the lo map) or the 4-way lerp (first operand: the corner rows V, with lylx); every operand with
    ld = C + pad and starting `off` channels into its buffer, X too"""
    Clo, Chi, n, pad, off = c["Clo"], c["Chi"], c["n"], c["pad"], c["off"]
    lda, ldh, ldx = (Clo + pad if Clo else 0), (Chi + pad if Chi else 0), Clo + Chi + pad
    first = (c["V"] if V is None else V) if lerp4 else c["LO2"]
    _, a = put(first, lda, off if Clo else 0)
    _, h = put(c["HI162"] if half else c["HI2"], ldh, off if Chi else 0)
    xb = filled(n * ldx)
    x = xb[off:]
    pix = dev(c["pix"])
    sfx = "_h" if half else ""
    if lerp4:
        ll = dev(c["lylx"]) if lylx is None else lylx
        L.call("arco_lerp4_cat_rows" + sfx, L.ptr(a), lda, Clo, L.ptr(ll), L.ptr(h), ldh, Chi, L.ptr(pix), n, L.ptr(x), ldx)
    else:
        L.call("arco_gather_upcat_rows" + sfx, L.ptr(a), lda, Clo, *c["lo"], L.ptr(h), ldh, Chi, *c["hi"], L.ptr(pix), n, L.ptr(x), ldx)
    got, ok = cols(xb, n, ldx, off, Clo + Chi)
    assert ok
    return got


def check_rows(name, c, got, half):
    Clo = c["Clo"]
    assert exact(got[:, Clo:], c["hi16_rows"] if half else c["hi_rows"])                          # a copy / an exact widening
    if Clo:
        report(name, worst(got[:, :Clo], c["ref_lo"], c["tol_lo"]))


def dense_bilinear(L, c):
    Clo, lo, hi = c["Clo"], c["lo"], c["hi"]
    rows = R.NV * hi[0] * hi[1]
    x = dev(c["LO2"])
    yb = filled(rows * Clo)
    L.call("arco_bilinear_fwd", L.ptr(x), Clo, R.NV, *lo, Clo, *hi, L.ptr(yb), Clo)
    return body(yb, rows * Clo, (rows, Clo))


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R2.ROW2D_CASES)), ids=ids(R2.ROW2D_CASES))
def test_gather_upcat_rows(L, i, half):
    c = R2.row2d_case(i)
    got = run_rows(L, c, False, half)
    check_rows(f"gather_upcat_rows case {i} half {half}", c, got, half)
    if c["Clo"]:                                                                                  # the rows of the dense resize, bit for bit
        assert bits_equal(got[:, :c["Clo"]], dense_bilinear(L, c)[c["pix"]])
        if c["lo"] == c["hi"]:
            assert bits_equal(got[:, :c["Clo"]], c["LO2"][c["pix"]])                              # the identity


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R2.ROW2D_CASES)), ids=ids(R2.ROW2D_CASES))
def test_lerp4_cat_rows(L, i, half):
    """on the reference's corner rows and (ly, lx); then on what arco_up_neighbors gives on the GPU: bit for bit the gather"""
    c = R2.row2d_case(i)
    got = run_rows(L, c, True, half)
    check_rows(f"lerp4_cat_rows case {i} half {half}", c, got, half)
    n = c["n"]
    pix, ib, lb = dev(c["pix"]), filled(4 * n, torch.int64), filled(2 * n)
    L.call("arco_up_neighbors", L.ptr(pix), n, *c["lo"], *c["hi"], L.ptr(ib), L.ptr(lb))
    nb4 = body(ib, 4 * n)
    body(lb, 2 * n)
    assert int(nb4.min()) >= 0 and int(nb4.max()) < c["LO2"].shape[0]
    got_nb = run_rows(L, c, True, half, lylx=lb, V=c["LO2"][nb4].contiguous())
    assert bits_equal(got_nb, run_rows(L, c, False, half))


# ---- (2) arco_zero_rows(_h), arco_cast_rows_f2h ------------------------------------------------------------------------------------------------
def dev_idx(idx):
    """an empty index list still needs a pointer (the entry points reject a null idx before they look at n)"""
    return dev(idx) if idx.numel() else torch.zeros(1, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R2.UTIL_CASES)), ids=ids(R2.UTIL_CASES))
def test_zero_rows(L, i, half):
    c = R2.zero_case(i, half)
    xb, x = put(c["X"], c["ld"])
    idx = dev_idx(c["idx"])
    L.call("arco_zero_rows_h" if half else "arco_zero_rows", L.ptr(x), c["ld"], c["C"], L.ptr(idx), c["n"])
    got, ok = cols(xb, c["M"], c["ld"], 0, c["C"])
    assert ok and bits_equal_any(got, c["ref"])                                                   # +0.0 in the named rows, the rest untouched


def bits_equal_any(a, b):
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


@pytest.mark.parametrize("scale", R2.CAST_SCALES)
@pytest.mark.parametrize("i", range(len(R2.UTIL_CASES)), ids=ids(R2.UTIL_CASES))
def test_cast_rows_f2h(L, i, scale):
    c = R2.cast_case(i, scale)
    M, C = c["M"], c["C"]
    sb, s = put(c["X"], c["lds"])
    db = filled(M * c["ldd"], torch.float16)
    idx = dev_idx(c["idx"])
    L.call("arco_cast_rows_f2h", L.ptr(s), c["lds"], C, L.ptr(idx), c["n"], scale, L.ptr(db), c["ldd"])
    got, ok = cols(db, M, c["ldd"], 0, C)
    assert ok and R.same_or_nan(got, c["ref"])                                                    # unnamed rows keep the sentinel
    src, ok = cols(sb, M, c["lds"], 0, C)
    assert ok and R.same_or_nan(src, c["X"])                                                      # the source is read only


# ---- (3) arco_fold_residual / arco_unfold_residual -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R2.FOLD_CASES)), ids=ids(R2.FOLD_CASES))
def test_fold_residual(L, i):
    c = R2.fold_case(i)
    n, k = c["n"], c["c"]
    lb, hb = filled(n * k), filled(n * (n - k))
    L.call("arco_fold_residual", L.ptr(dev(c["W"])), n, k, L.ptr(lb), L.ptr(hb))
    assert bits_equal(body(lb, n * k, (n, k)), c["lo"]) and bits_equal(body(hb, n * (n - k), (n, n - k)), c["hi"])


@pytest.mark.parametrize("null", ("none", "lo", "hi"))
@pytest.mark.parametrize("i", range(len(R2.FOLD_CASES)), ids=ids(R2.FOLD_CASES))
def test_unfold_residual(L, i, null):
    c = R2.fold_case(i)
    n, k = c["n"], c["c"]
    wb = filled(n * n)
    dlo, dhi = (None if null == "lo" else dev(c["dlo"])), (None if null == "hi" else dev(c["dhi"]))
    L.call("arco_unfold_residual", L.ptr(dlo), L.ptr(dhi), n, k, L.ptr(wb))
    assert bits_equal(body(wb, n * n, (n, n)), {"none": c["dW"], "lo": c["dW_nolo"], "hi": c["dW_nohi"]}[null])


# ---- (4) arco_combine_terms (+ _bwd) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R2.COMBINE_N)
def test_combine_terms(L, n):
    c = R2.combine_case(n)
    ts = [c["t"][i].clone().to(DEV) for i in range(n)]                                            # n separate 0-d device floats
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    ws = (ctypes.c_float * n)(*[float(w) for w in c["w"]])
    ob = filled(1)
    L.call("arco_combine_terms", ptrs, ws, n, L.ptr(ob))
    report(f"combine_terms n {n}", worst(body(ob, 1), c["ref"], c["tol"]))
    gb = filled(n)
    L.call("arco_combine_terms_bwd", ws, n, L.ptr(dev(c["g"])), L.ptr(gb))
    assert bits_equal(body(gb, n), c["grads"])                                                    # one IEEE multiplication
