"""CPU companion of tests/test_side_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * every toleranced comparison: the kernel's formula emulated in fp32 (numpy float32 index arithmetic, torch fp32 values, the fma of
    tl_blend1 through float64) stays inside the SAME per-element bound against the SAME float64 reference of
    tests/side_kernel_refs.py; the worst ratios are printed, and the largest per kernel is recorded in the GPU file's docstring;
  * the input conditions the GPU file relies on hold for its inputs;
  * every comparison helper rejects a planted error: corner order x / y swapped, l and 1 - l swapped, the index clamp off by one, one
    tap dropped from the adjoint, one fixed-point contribution dropped, one row of a permutation shifted;
  * the argument checks of the entry points reject on the host (ARCO_ERR_ARG before anything is launched: no GPU needed)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import side_kernel_refs as R
from loss_kernel_refs import SENTINEL, exact, pad_ok, worst


def report(name, ratio):
    print(f"emulated {name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


# ---- emulations inside the bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.TRI_CASES)))
def test_trilinear_bounds_hold_for_the_emulation(i):
    c = R.tri_case(i)
    report(f"trilinear fwd case {i}", worst(R.emu_tri_fwd(c), c["ref"], c["tol"]))
    report(f"trilinear bwd case {i}", worst(R.emu_tri_bwd(c), c["dX"], c["tol_b"]))
    if c["lo"] == c["hi"]:
        assert exact(R.emu_tri_fwd(c), c["X"])
    # float64 autograd IS the transposed float64 resize: <dY, resize(X)> == <dX, X>
    a, b = float((c["dY"].double() * c["ref"]).sum()), float((c["dX"] * c["X"].double()).sum())
    assert abs(a - b) <= 1e-9 * (abs(a) + 1.0)


def test_trilinear_big_cases_pass_the_grid_cap_by_one():
    for bwd in (False, True):
        lo, hi = R.TRI_BIG_BWD if bwd else R.TRI_BIG_FWD
        assert int(np.prod(lo if bwd else hi)) == 4096 * 256 + 1
    c = R.tri_big(False)
    report("trilinear fwd big", worst(R.emu_tri_fwd(c), c["ref"], c["tol"]))


@pytest.mark.parametrize("i", range(len(R.ROW_CASES)))
def test_row_bounds_hold_for_the_emulation(i):
    c = R.row_case(i)
    if c["Clo"]:
        report(f"row blend case {i}", worst(R.emu_rows(c), c["ref_lo"], c["tol_lo"]))
    assert exact(c["hi16_rows"], c["HI16"].view(R.NV * int(np.prod(c["hi"])), c["Chi"])[c["pix"]].float())
    for d in (2, 3):
        s = R.scatter_case(i, d)
        report(f"lerp bwd d {d} case {i}", worst(s["emu"], s["ref"], s["tol"]))
        M = R.NV * int(np.prod(s["lo"]))
        report(f"scatter lo d {d} case {i}", worst(R.emu_scatter(s["rows"], s["emu"], M), s["dlo"], s["tol_lo"]))
        Mh = R.NV * int(np.prod(s["hi"]))
        report(f"scatter hi d {d} case {i}", worst(R.emu_scatter(s["pix"], s["dX"][:, s["Clo"]:], Mh), s["dhi"], s["tol_hi"]))
        # reversed arrival order: another of the orders the atomics may take
        report(f"scatter lo reversed d {d} case {i}", worst(R.emu_scatter(s["rows"].flip(0), s["emu"].flip(0), M), s["dlo"], s["tol_lo"]))


@pytest.mark.parametrize("d", (2, 3))
@pytest.mark.parametrize("i", range(len(R.CORNER_CASES)))
def test_corner_restatement_holds_the_float64_property(i, d):
    c = R.corner_case(i, d)
    r_coord, r_sum, inside = R.corner_property(c["cn"]["idx"], c["cn"]["w"], c["cn"])
    print(f"emulated corners d {d} case {i}: coordinate err / (4 S u) {r_coord:.3f}, weight-sum err / (4 u) {r_sum:.3f}")
    assert inside and r_coord <= 1.0 and r_sum <= 1.0
    # the float32 cell is the exact cell, or its neighbour with a weight of a few u on the far corner
    for a in range(d):
        i0, _, l, _ = c["cn"]["ax"][a]
        e0 = c["cn"]["exact"][a][1]
        assert bool(((i0 == e0) | ((np.abs(i0 - e0) == 1) & ((l < 1e-5) | (l > 1 - 1e-5)))).all())


@pytest.mark.parametrize("nesterov", (True, False))
@pytest.mark.parametrize("i", range(len(R.OPT_CASES)))
def test_optimiser_bounds_hold_for_the_emulation(i, nesterov):
    c = R.opt_case(i, nesterov)
    p, b = R.emu_opt(c, nesterov)
    report(f"sgd nesterov {nesterov} case {i} buf", worst(b, c["ref_b"], c["tol_b"]))
    report(f"sgd nesterov {nesterov} case {i} p", worst(p, c["ref_p"], c["tol_p"]))
    if i == 3:                                                                # the float64 formula is torch.optim.SGD's
        pp = torch.nn.Parameter(c["p"].double().clone())
        pp.grad = c["g"].double().clone()
        opt = torch.optim.SGD([pp], lr=R.f32(c["lr"]), momentum=R.f32(c["mom"]), weight_decay=R.f32(c["wd"]), nesterov=nesterov)
        opt.step()                                                            # first step: buf = g
        assert worst(pp.detach(), c["ref_p"], 1e-12 * c["ref_p"].abs() + 1e-15) <= 1.0


@pytest.mark.parametrize("i", range(len(R.EMA_CASES)))
def test_ema_bound_holds_for_the_emulation(i):
    c = R.ema_case(i)
    report(f"ema case {i}", worst(c["emu"], c["ref"], c["tol"]))


@pytest.mark.parametrize("i", range(len(R.DET_CASES)))
def test_det_restatement_holds_the_float64_bound_and_its_conditions(i):
    c = R.det_case(i)
    s = c["src"]
    finite = s[torch.isfinite(s)]
    assert bool(((finite == 0) | (finite.abs() >= 2.0 ** -126)).all())                            # zero or normal
    if c["w"] is not None:
        assert float(c["w"].abs().max()) <= 1.0
    if c["kind"] != "ok":
        assert bool((c["acc"] == 0).all())
        return
    assert c["max_contrib"] < 2 ** 18 and int(c["acc"].abs().max()) < 2 ** 62
    t = c["touched"]                                                                              # every finite case, alpha = -3 too
    report(f"det chain {c['name']}", worst(c["dst"][t], c["ref64"][t], c["tol64"][t]))
    if c["sp"] == "top_small":
        rows = c["rows"]
        small, tiny = int(rows[8]), int(rows[16])
        assert bool((c["dst"][tiny] == 0).all()) and bool((c["dst"][small] != 0).any())            # below 2^-45 of the maximum: zero
        assert float(c["dst"][small].abs().max()) < 2.0 ** -25 * 4.0
    if c["name"] == "collide":
        assert int(c["n_r"].max()) >= 4096


def test_case_tables_cover_the_listed_edges():
    assert {c[1] for c in R.DET_CASES} == {1, 63, 64, 65, 130} and {c[5] for c in R.DET_CASES} == {1, 3, 8}
    assert {c[8] for c in R.DET_CASES} == {1.0, 0.5, -3.0} and {c[6] for c in R.DET_CASES} == {True, False}
    assert {c[7] for c in R.DET_CASES} == {True, False} and any(c[2] > 0 for c in R.DET_CASES)
    assert {c[9] for c in R.DET_CASES} >= {"min", "big", "zero", "inf", "nan", "top_small"}
    assert R.det_case(5)["mb"] == 0x00800000 and R.det_case(6)["mb"] == (120 + 127) << 23
    assert {c[1] for c in R.ROW_CASES} >= {4, 12, 260, 0} and {c[2] for c in R.ROW_CASES} >= {0, 4}
    assert {c[0] for c in R.ROW_CASES} == set(range(len(R.RATIOS))) == {c[0] for c in R.TRI_CASES}
    assert {c[3] % 4 for c in R.ROW_CASES} == {0, 1, 3} == {c[1] % 4 for c in R.CORNER_CASES}
    assert any(c[4] and c[5] for c in R.ROW_CASES) and any(not c[4] for c in R.ROW_CASES)
    for cases, work in ((R.S2D_CASES, lambda c: c[0] * c[1] * c[2] * c[3] * 8 * (c[4] // 4)),
                        (R.D2S_CASES, lambda c: c[0] * c[1] * c[2] * c[3] * 8 * (c[4] // 4)), (R.COPY_CASES, lambda c: c[0] * (c[1] // 4)),
                        (R.OPT_CASES, lambda c: c[0]), (R.EMA_CASES, lambda c: c[0])):
        assert any(4096 * 256 < work(c) <= 4096 * 256 + 8 for c in cases), cases
    assert any(c[0] * c[1] == 1024 * 256 + 1 for c in R.ABSMAX_CASES)
    assert any(n // 4 == 4096 * 256 + 1 for n in R.CAST_N) and {n % 4 for n in R.CAST_N} == {0, 1, 2, 3} and min(R.CAST_N) < 4
    assert {c[3] for c in R.OPT_CASES} >= {0.0} and {c[2] for c in R.OPT_CASES} >= {0.0} and {c[4] for c in R.OPT_CASES} == {0, 1}
    assert {c[1] for c in R.EMA_CASES} >= {0.0, 0.99, 1.0}
    s = R.S2D_CASES
    assert any(c[1] == 1 for c in s) and any(c[2] == 1 for c in s) and any(c[3] == 1 for c in s) and any(c[1] % 2 and c[1] > 1 for c in s)
    assert any(c[5] for c in s) and any(c[6] for c in s) and any(c[7] == "h" for c in s)
    t = R.TRANS_CASES
    assert any(c[1] < 32 for c in t) and any(c[1] % 32 and c[1] > 32 for c in t) and any(c[2] == 1 for c in t) and any(c[0] == 3 for c in t)
    assert any(c[1] % 4 and c[1] > 256 for c in R.PUT_CASES)


@pytest.mark.parametrize("i", range(len(R.ROW_CASES)))
def test_sampled_voxels_hold_the_listed_conditions(i):
    c = R.row_case(i)
    pix, hi = c["pix"], c["hi"]
    vol = int(np.prod(hi))
    assert {0, vol - 1, (R.NV - 1) * vol, R.NV * vol - 1} <= set(pix.tolist())
    assert int(torch.bincount(pix).max()) >= 64
    co = np.unravel_index(pix.numpy() % vol, hi)
    for a in range(3):
        assert (co[a] == 0).any() and (co[a] == hi[a] - 1).any()
    assert int(pix.min()) >= 0 and int(pix.max()) < R.NV * vol


def test_exact_inputs_hold_their_conditions():
    for i, cs in enumerate(R.S2D_CASES):
        c = R.s2d_case(i)
        if cs[7] == "h":                                                     # moved as words == the f16 tensor's own permutation
            V16 = c["V"].view(torch.int16)
            assert torch.equal(R.pack(V16, c["nv"], c["x2"], c["y2"], c["z2"], 2 * c["c"]).contiguous().view(torch.int32), c["P"])
        f = c["V"].view(torch.float32)
        assert bool(torch.isnan(f).any()) and bool((c["V"] == -2 ** 31).any())
        assert torch.equal(R.unpack(c["P"], c["nv"], c["x2"], c["y2"], c["z2"], c["c"]), c["V"])
    c = R.nonzero_case()
    assert torch.equal(c["ref"].bool(), ((c["X"] != 0) | torch.isnan(c["X"])).any(1)) and c["M"] % 4 != 0
    for i in range(len(R.PUT_CASES)):
        c = R.put_case(i)
        assert c["idx"].unique().numel() == c["n"] and c["lds"] % 4 == 0 and c["ldd"] % 4 == 0
    for i in range(len(R.ABSMAX_CASES)):
        c = R.absmax_case(i)
        fin = c["x"][torch.isfinite(c["x"])]
        assert float(fin.abs().max()) < abs(SENTINEL)
    c = R.cast_case(1027)
    y = c["f2h"].float()
    assert float(y[torch.isfinite(y)].abs().max()) == 65504.0 and bool(torch.isnan(y).any()) and not bool(torch.isinf(y).any())
    sub = (y != 0) & (y.abs() < 2.0 ** -14)
    assert bool(sub.any()) and bool(torch.isinf(c["x"]).any())
    assert R.same_or_nan(c["h"].float(), c["h2f"]) and bool(torch.isnan(c["h2f"]).any()) and bool(torch.isinf(c["h2f"]).any())


# ---- planted errors --------------------------------------------------------------------------------------------------------------------------
def test_helpers_reject_planted_errors():
    c = R.row_case(2)                                                         # non-integer upsampling, 12 channels
    n, Clo = c["n"], c["Clo"]
    ax = c["cn"]["ax"]
    v = [c["V"].view(n, 8, Clo)[:, k] for k in range(8)]
    t = lambda a, k: torch.from_numpy(np.ascontiguousarray(ax[k][a])).view(n, 1)
    good = R.emu_blend(v, t(3, 2), t(2, 2), t(3, 1), t(2, 1), t(3, 0), t(2, 0))
    assert worst(good, c["ref_lo"], c["tol_lo"]) <= 1.0
    swapped_xy = R.emu_blend([v[k] for k in (0, 2, 1, 3, 4, 6, 5, 7)], t(3, 2), t(2, 2), t(3, 1), t(2, 1), t(3, 0), t(2, 0))
    assert worst(swapped_xy, c["ref_lo"], c["tol_lo"]) > 1e3                   # corner order x / y swapped
    swapped_l = R.emu_blend(v, t(2, 2), t(3, 2), t(3, 1), t(2, 1), t(3, 0), t(2, 0))
    assert worst(swapped_l, c["ref_lo"], c["tol_lo"]) > 1e3                    # l and 1 - l swapped
    one = good.clone()
    one[n // 2, Clo - 1] += 1e-4
    assert worst(one, c["ref_lo"], c["tol_lo"]) > 1.0
    # the index clamp off by one: the voxels on the far x face take their corner from one column short
    cc = R.corner_case(1, 3)
    cn = cc["cn"]
    idx = cn["idx"].copy()
    far = cn["ax"][2][0] == cc["lo"][2] - 1
    assert far.any()
    idx[far] -= 1
    r_coord, _, _ = R.corner_property(idx, cn["w"], cn)
    assert r_coord > 1e3 and not exact(torch.from_numpy(idx.reshape(-1)), cc["idx"])
    R.check_corners("the restatement itself", cc, cc["idx"].clone(), cc["w"].clone())
    with pytest.raises(AssertionError, match="float64 property fails"):
        R.check_corners("clamp off by one", cc, torch.from_numpy(idx.reshape(-1)), cc["w"])
    w = cn["w"].copy()
    w[3, 5] = np.nextafter(w[3, 5], np.float32(2))                            # one weight one ulp off: the bit comparison's to reject
    w = torch.from_numpy(w.reshape(-1))
    assert R.bits_equal(cc["w"].clone(), cc["w"]) and not R.bits_equal(w, cc["w"])
    with pytest.raises(AssertionError, match="float32 restatement differs"):
        R.check_corners("one ulp", cc, cc["idx"], w)
    nz = torch.tensor([0.0, 1.0])                                             # -0.0 == 0.0, but not bit for bit
    assert not R.bits_equal(-nz, nz) and not R.bits_equal(nz[:1], nz)
    # one tap dropped from the adjoint
    tc = dict(R.tri_case(2))
    assert worst(R.emu_tri_bwd(tc), tc["dX"], tc["tol_b"]) <= 1.0
    dY = tc["dY"].clone()
    dY[1, 2, 3, 1] = 0
    tc["dY"] = dY
    assert worst(R.emu_tri_bwd(tc), tc["dX"], tc["tol_b"]) > 1e3
    s = R.scatter_case(3, 3)
    M = R.NV * int(np.prod(s["lo"]))
    assert worst(R.emu_scatter(s["rows"][1:], s["emu"][1:], M), s["dlo"], s["tol_lo"]) > 1e3
    # one fixed-point contribution dropped, in the small-valued row: 2^-30 of the tensor maximum, far inside the 4e-7 of the maximum
    # that tests/test_det_scatter_gpu.py allows
    d = R.det_case(4)
    drop = 8 + int(d["w"][8:16].abs().argmax())
    bad = R.det_chain(d["src"], d["div"], d["lst"], d["idx"], d["w"], d["alpha"], d["M"], drop=drop)
    t = d["touched"]
    assert not R.bits_equal(bad["dst"][t], d["dst"][t]) and not exact(bad["acc"], d["acc"])
    assert worst(bad["dst"][t], d["ref64"][t], d["tol64"][t]) > 100.0
    assert float((bad["dst"] - d["dst"]).abs().max()) < 4e-7 * float(d["src"].abs().max())
    # one row of a permutation shifted
    sc = R.s2d_case(0)
    Pm = sc["P"].clone()
    Pm[3] = sc["P"][4]
    assert exact(sc["P"].clone(), sc["P"]) and not exact(Pm, sc["P"])
    pc = R.put_case(0)
    ref = torch.full_like(pc["ref"], SENTINEL)
    ref[(pc["idx"] + 1) % pc["M"]] = pc["src"]
    assert not exact(ref, pc["ref"])
    # the buffer checks of the GPU file (R.body / R.cols): a touched guard, pad column or column in front of a channel slice
    rows, ld, off, C = 4, 12, 4, 4
    for dtype in (torch.float32, torch.int64):
        buf = torch.full((rows * ld + R.GUARD,), R.sent(dtype), dtype=dtype)
        buf[:rows * ld].view(rows, ld)[:, off:off + C] = 3
        got, ok = R.cols(buf, rows, ld, off, C)
        assert ok and bool((got == 3).all()) and got.shape == (rows, C)
        for at in (2 * ld + off + C, 2 * ld + off - 1, 3 * ld + ld - 1, 0):  # behind the slice, in front of it, the last pad, the first
            bad_buf = buf.clone()
            bad_buf[at] = 0
            assert not R.cols(bad_buf, rows, ld, off, C)[1], at
        for at in (rows * ld, rows * ld + R.GUARD - 1):                       # the guard's first and last element
            bad_buf = buf.clone()
            bad_buf[at] = 0
            with pytest.raises(AssertionError, match="guard"):
                R.cols(bad_buf, rows, ld, off, C)
            with pytest.raises(AssertionError, match="guard"):
                R.body(bad_buf, rows * ld)
    buf = torch.full((4, 12), SENTINEL)
    assert pad_ok(buf, 8)
    buf[2, 9] = 0.0
    assert not pad_ok(buf, 8)
    # a NaN where none belongs
    nanny = good.clone()
    nanny[0, 0] = math.nan
    assert worst(nanny, c["ref_lo"], c["tol_lo"]) == math.inf
    cs = R.cast_case(1027)
    wrong = cs["f2h"].clone()
    wrong[torch.isinf(cs["x"]).nonzero()[0]] = math.inf                       # an inf let through instead of +-65504
    assert R.same_or_nan(cs["f2h"].clone(), cs["f2h"]) and not R.same_or_nan(wrong, cs["f2h"])


# ---- argument checks (host side) -------------------------------------------------------------------------------------------------------------
def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced.  Every list below is a VALID call with one argument spoilt at a time; the valid call itself is never
    made."""
    import arco_amd._lib as L
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    assert buf.data_ptr() % 16 == 0
    p = ctypes.c_void_p(buf.data_ptr())
    odd4 = ctypes.c_void_p(buf.data_ptr() + 4)            # 4-byte aligned only
    odd8 = ctypes.c_void_p(buf.data_ptr() + 8)            # 8-byte aligned only
    bad = -1

    def spoil(name, ok, cases):
        for pos, val in cases:
            args = list(ok)
            args[pos] = val
            assert L.query(name, *args, None) == bad, (name, pos, val)

    nulls = lambda *pos: [(k, None) for k in pos]
    zeros = lambda *pos: [(k, 0) for k in pos]
    odd = lambda v, *pos: [(k, v) for k in pos]
    # s2d3: V, ldv, NV, X2, Y2, Z2, C, P, ldp, dir
    spoil("arco_s2d3", [p, 4, 1, 1, 1, 1, 4, p, 32, 0], nulls(0, 7) + zeros(2, 3, 4, 5, 6) + odd(odd8, 0, 7) + [(6, 6), (1, 6), (8, 34), (9, 2)])
    # d2s3_add(_h): P, ldp, NV, X2, Y2, Z2, C, ADD, lda, V, ldv
    ok = [p, 32, 1, 1, 1, 1, 4, p, 4, p, 4]
    spoil("arco_d2s3_add", ok, nulls(0, 7, 9) + zeros(2, 3, 4, 5, 6) + odd(odd8, 0, 7, 9) + [(6, 6), (1, 34), (8, 6), (10, 6)])
    spoil("arco_d2s3_add_h", ok, nulls(0, 7, 9) + zeros(2, 3, 4, 5, 6) + odd(odd4, 0, 7, 9) + [(6, 6)])
    # trilinear_fwd / _bwd: X, ldx, NV, Di, Hi, Wi, C, Do, Ho, Wo, Y, ldy
    ok = [p, 4, 1, 2, 2, 2, 4, 3, 3, 3, p, 4]
    for name in ("arco_trilinear_fwd", "arco_trilinear_bwd"):
        spoil(name, ok, nulls(0, 10) + zeros(2, 3, 4, 5, 6, 7, 8, 9) + odd(odd8, 0, 10) + [(6, 6), (1, 6), (11, 6), (2, -1)])
    # gather_upcat_rows3d(_h) / lerp8_cat_rows3d(_h): lo, ldlo, Clo, Di, Hi, Wi, hi, ldhi, Chi, Do, Ho, Wo, pix, n, X, ldx
    ok = [p, 4, 4, 2, 2, 2, p, 4, 4, 3, 3, 3, p, 1, p, 8]
    for name in ("arco_gather_upcat_rows3d", "arco_lerp8_cat_rows3d"):
        spoil(name, ok, nulls(0, 6, 12, 14) + zeros(3, 4, 5, 9, 10, 11) + odd(odd8, 0, 6, 14) + [(13, -1), (2, 6), (8, 6), (1, 6), (7, 6), (15, 6), (2, -4)])
        spoil(name + "_h", ok, nulls(0, 6, 12, 14) + zeros(3, 4, 5, 9, 10, 11) + odd(odd8, 0, 14) + odd(odd4, 6) + [(13, -1), (8, 6)])
        assert L.query(name, *[None if k in (0, 6, 12, 14) else v for k, v in enumerate(ok[:13])], 0, None, 8, None) == 0      # n == 0: nothing to do
    # lerp8_rows3d_bwd: dX, ldx, Clo, w8, n, dV, ldv
    spoil("arco_lerp8_rows3d_bwd", [p, 8, 4, p, 1, p, 4], nulls(0, 3, 5) + odd(odd8, 0, 5) + [(4, -1), (2, 6), (1, 6), (6, 6), (2, -4)])
    # scatter_upcat_rows3d: dX, ldx, pix, n, dlo, ldlo, Clo, Di, Hi, Wi, dhi, ldhi, Chi, Do, Ho, Wo
    spoil("arco_scatter_upcat_rows3d", [p, 8, p, 1, p, 4, 4, 2, 2, 2, p, 4, 4, 3, 3, 3],
          nulls(0, 2, 4, 10) + zeros(7, 8, 9, 13, 14, 15) + [(3, -1), (6, -1), (12, -1)])
    # scatter_upcat_rows: dX, ldx, pix, n, dlo, ldlo, Clo, Hi, Wi, dhi, ldhi, Chi, Ho, Wo
    spoil("arco_scatter_upcat_rows", [p, 8, p, 1, p, 4, 4, 2, 2, p, 4, 4, 3, 3], nulls(0, 2, 4, 9) + zeros(7, 8, 12, 13) + [(3, -1), (6, -1), (11, -1)])
    # up_neighbors: pix, n, Hi, Wi, Ho, Wo, nb4, lylx
    spoil("arco_up_neighbors", [p, 1, 2, 2, 3, 3, p, p], nulls(0, 6, 7) + zeros(2, 3, 4, 5) + [(1, -1)])
    # gather_upcat_rows(_h): lo, ldlo, Clo, Hi, Wi, hi, ldhi, Chi, Ho, Wo, pix, n, X, ldx
    ok = [p, 4, 4, 2, 2, p, 4, 4, 3, 3, p, 1, p, 8]
    common = nulls(0, 5, 10, 12) + zeros(3, 4, 8, 9) + [(11, -1), (2, 6), (7, 6), (1, 6), (6, 6), (13, 6), (2, -4), (7, -4)]
    spoil("arco_gather_upcat_rows", ok, common + odd(odd8, 0, 5, 12))
    spoil("arco_gather_upcat_rows_h", ok, common + odd(odd8, 0, 12) + odd(odd4, 5))
    for name in ("arco_gather_upcat_rows", "arco_gather_upcat_rows_h"):
        assert L.query(name, *[None if k in (0, 5, 10, 12) else v for k, v in enumerate(ok[:11])], 0, None, 8, None) == 0      # n == 0: nothing to do
        assert L.query(name, None, 0, 0, 2, 2, odd4, 4, 4, 3, 3, p, 1, p, 8, None) == bad                                       # an empty lo part: hi is still checked
    # lerp4_cat_rows(_h): V, ldv, Clo, lylx, hi, ldhi, Chi, pix, n, X, ldx
    ok = [p, 4, 4, p, p, 4, 4, p, 1, p, 8]
    common = nulls(0, 3, 4, 7, 9) + [(8, -1), (2, 6), (6, 6), (1, 6), (5, 6), (10, 6), (2, -4), (6, -4)]
    spoil("arco_lerp4_cat_rows", ok, common + odd(odd8, 0, 4, 9))
    spoil("arco_lerp4_cat_rows_h", ok, common + odd(odd8, 0, 9) + odd(odd4, 4))
    for name in ("arco_lerp4_cat_rows", "arco_lerp4_cat_rows_h"):
        assert L.query(name, None, 4, 4, None, None, 4, 4, None, 0, None, 8, None) == 0                                         # n == 0: nothing to do
    # zero_rows(_h): dst, ld, C, idx, n;  cast_rows_f2h: src, ld_src, C, idx, n, scale, dst, ld_dst
    spoil("arco_zero_rows", [p, 4, 4, p, 1], nulls(0, 3) + odd(odd8, 0) + [(2, 6), (2, 0), (2, -4), (1, 6), (4, -1)])
    spoil("arco_zero_rows_h", [p, 4, 4, p, 1], nulls(0, 3) + odd(odd4, 0) + [(2, 6), (2, 0), (2, -4), (1, 6), (4, -1)])
    spoil("arco_cast_rows_f2h", [p, 4, 4, p, 1, 1.0, p, 4], nulls(0, 3, 6) + odd(odd8, 0) + odd(odd4, 6) + [(2, 6), (2, 0), (1, 6), (7, 6), (4, -1)])
    # fold_residual: W, n, c, lo, hi;  unfold_residual: dlo, dhi, n, c, dW (either block may be null);  combine_terms: terms, weights,
    # n, out;  combine_terms_bwd: weights, n, g, grads
    spoil("arco_fold_residual", [p, 3, 1, p, p], nulls(0, 3, 4) + [(1, 0), (2, 0), (2, 3), (1, -3), (2, -1)])
    spoil("arco_unfold_residual", [p, p, 3, 1, p], nulls(4) + [(2, 0), (3, 0), (3, 3), (3, -1)])
    spoil("arco_combine_terms", [p, p, 2, p], nulls(0, 1, 3) + [(2, 0), (2, 9), (2, -1)])
    spoil("arco_combine_terms_bwd", [p, 2, p, p], nulls(0, 2, 3) + [(1, 0), (1, 9), (1, -1)])
    # lerp4_cat_rows_bwd: dX, ldx, Clo, lylx, pix, n, dV, ldv, dhi, ldhi, Chi
    spoil("arco_lerp4_cat_rows_bwd", [p, 8, 4, p, p, 1, p, 4, p, 4, 4], nulls(0, 3, 4, 6, 8) + odd(odd8, 0, 6) + [(5, -1), (2, 6), (1, 6), (7, 6), (10, -1)])
    # copy_rows: X, ldx, M, C, Y, ldy, accumulate
    spoil("arco_copy_rows", [p, 4, 1, 4, p, 4, 0], nulls(0, 4) + odd(odd8, 0, 4) + [(2, -1), (3, 0), (3, 6), (1, 6), (5, 6)])
    # nchw_to_nhwc: X, NB, C, P, Y, ldy;  nhwc_to_nchw: X, ldx, NB, C, P, Y
    spoil("arco_nchw_to_nhwc", [p, 1, 4, 4, p, 4], nulls(0, 4) + zeros(1, 2, 3) + [(1, 65536), (3, -1)])
    spoil("arco_nhwc_to_nchw", [p, 4, 1, 4, 4, p], nulls(0, 5) + zeros(2, 3, 4) + [(2, 65536), (4, -1)])
    # sgd: p, g, buf, n, lr, momentum, weight_decay, first;  ema: k, q, n, m
    for name in ("arco_sgd_nesterov", "arco_sgd_momentum"):
        spoil(name, [p, p, p, 4, 0.1, 0.9, 0.0, 0], nulls(0, 1, 2) + [(3, -1)])
        assert L.query(name, None, None, None, 0, 0.1, 0.9, 0.0, 0, None) == 0
    spoil("arco_ema", [p, p, 4, 0.5], nulls(0, 1) + [(2, -1)])
    # det_scatter.hip
    spoil("arco_det_absmax", [p, 4, 4, 1, p], nulls(0, 4) + [(2, 0), (3, -1)])
    spoil("arco_det_scatter_rows", [p, 4, 4, 1, None, p, None, 1, p, 4, p], nulls(0, 5, 8, 10) + [(2, 0), (3, 0), (7, -1), (8, odd4)])
    spoil("arco_det_finish_rows", [None, p, 1, p, 4, 4, p, 1.0, p, 4], nulls(1, 3, 6, 8) + [(5, 0), (2, -1)])
    spoil("arco_det_clear_rows", [None, p, 1, p, 4, 4], nulls(1, 3) + [(5, 0), (2, -1)])
    spoil("arco_corner_rows3d", [p, 1, 2, 2, 2, 3, 3, 3, p, p], nulls(0, 8, 9) + zeros(2, 3, 4, 5, 6, 7) + [(1, -1)])
    spoil("arco_corner_rows2d", [p, 1, 2, 2, 3, 3, p, p], nulls(0, 6, 7) + zeros(2, 3, 4, 5) + [(1, -1)])
    spoil("arco_row_nonzero", [p, 4, 4, 1, p], nulls(0, 4) + odd(odd8, 0) + [(2, 0), (1, 6), (3, -1)])
    spoil("arco_put_rows", [p, 4, 4, p, 1, p, 4], nulls(0, 3, 5) + odd(odd8, 0, 5) + [(2, 0), (1, 6), (6, 6), (4, -1)])
    spoil("arco_cast_h2f", [p, 4, p], nulls(0, 2) + [(1, 0), (0, odd4), (2, odd8)])
    spoil("arco_cast_f2h", [p, 4, 1.0, p], nulls(0, 3) + [(1, 0), (0, odd8), (3, odd4)])
