"""CPU companion of tests/test_glue_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * every toleranced comparison: the kernel's formula emulated in torch fp32, op by op (torch's own expf / logf and summation
    order), stays inside the SAME per-element bound against the SAME float64 reference of tests/glue_kernel_refs.py; the worst ratios
    are printed, and the largest per kernel is recorded in the GPU file's docstring;
  * the input conditions the GPU file relies on hold for its inputs: at most 0.1 % of the rows of a softmax case are left out of the
    arg-max comparison, every valid row of an unsupervised-CE case is a decided positive (float64 CE >= 1e-3) or a constructed zero,
    the emulation's selection equals the reference's, the cases cross every grid cap and reach every class-count instantiation, the
    percentile inputs hold the listed edges and their two float64 evaluation orders round to one fp32 threshold;
  * every comparison helper rejects a planted error: one wrong element, one touched pad column, a label off by one;
  * the argument checks of the entry points reject on the host (ARCO_ERR_ARG before anything is launched: no GPU needed)."""
import ctypes
import math

import pytest
import torch

import glue_kernel_refs as R
from loss_kernel_refs import SENTINEL, exact, pad_ok, worst


def report(name, ratio):
    print(f"emulated {name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def held(name, emu, c, keys):
    for k in keys:
        report(f"{name} {k}", worst(emu[k], c["ref"][k], c["tol"][k]))


# ---- softmax -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SOFTMAX_CASES)))
def test_softmax_bounds_hold_for_the_emulation_and_argmax_is_decided(i):
    c = R.softmax_case(i)
    e = R.emu_softmax(c)
    held(f"softmax case {i}", e, c, ("prob", "maxp", "ent"))
    left_out = 1.0 - float(c["decided"].double().mean())
    print(f"softmax case {i}: arg-max left out {left_out:.5f}, saturated rows {int(c['sat'].sum())}, bit-equal rows {int(c['equal'].sum())}")
    assert left_out <= 1e-3
    dec = c["decided"]
    assert torch.equal(e["amax"][dec], c["amax"][dec])
    if c["M"] >= 7:
        assert bool(c["equal"].any()) and bool((c["amax"][c["equal"]] == 0).all())
    sat = c["sat"]
    if bool(sat.any()):                                                  # p == 1 and entropy == -0.0 in fp32
        assert bool((e["maxp"][sat] == 1.0).all()) and bool((e["ent"][sat] == 0).all()) and bool(torch.signbit(e["ent"][sat]).all())


def test_softmax_cases_cover_the_listed_edges():
    cs = R.SOFTMAX_CASES
    assert {c[0] for c in cs} == {1, 2, 4, 5, 19, 32}
    assert {c[1] for c in cs} == {1, 255, 256, 257, 524288 + 300}
    assert any(c[3] > 0 and c[1] // c[2] == 3 for c in cs) and any(c[3] > 0 and c[1] == c[2] for c in cs)
    assert any(c[4] == 40.0 for c in cs) and any(c[1] > 2048 * 256 for c in cs)           # one row past gl_grid's cap and more
    assert sum(int(R.softmax_case(i)["sat"].sum()) for i in range(len(cs)) if cs[i][0] > 1) > 10


# ---- supervised CE + Dice, Dice on probabilities --------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SUP_CASES)))
def test_sup_loss_bounds_hold_for_the_emulation(i):
    c = R.sup_case(i)
    held(f"sup loss case {i}", R.emu_sup(c), c, ("out", "sums", "dx"))
    # the float64 formula the tolerance is derived from IS the gradient (autograd of CE and Dice)
    assert worst(c["dx_formula"], c["ref"]["dx"], 1e-12 + 1e-8 * c["ref"]["dx"].abs()) <= 1.0
    if c["kind"] == "absent" and c["C"] > 1:
        assert float(c["Y"][c["C"] - 1]) == 0.0
    if c["kind"] == "owner":
        assert float(c["Y"][c["C"] // 2]) == c["M"]


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("i", range(len(R.SUP_CASES)))
def test_dice_probs_bounds_hold_for_the_emulation(i, weighted):
    c = R.dice_case(i, weighted)
    held(f"dice probs case {i} {'weighted' if weighted else 'null weights'}", R.emu_dice(c), c, ("out", "sums", "dp"))
    if weighted and c["C"] > 2:
        assert len(set(c["w32"].tolist())) > 1


def test_sup_cases_cover_the_listed_edges():
    cs = R.SUP_CASES
    assert {c[0] for c in cs} == set(R.SUP_C) == {1, 2, 3, 4, 5, 8, 9, 19, 21, 32}
    assert {c[1] for c in cs} == {1, 255, 257, 262144 + 257}
    for lo, hi in ((1, 4), (5, 8), (9, 32)):                                      # every instantiation with C below and at CM
        inst = {c[0] for c in cs if lo <= c[0] <= hi}
        assert hi in inst and min(inst) < hi
    assert any(c[2] > 0 for c in cs) and any(c[3] > 0 for c in cs) and any(c[4] == 40.0 for c in cs)
    assert {c[5] for c in cs} == {"rand", "absent", "owner"}
    assert R.G_CE != 1.0 and R.G_DICE != 1.0


# ---- unsupervised CE -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.UNSUP_CASES)))
def test_unsup_loss_rows_are_decided_and_bounds_hold_for_the_emulation(i):
    c = R.unsup_case(i)
    valid, pos, zero = c["valid"], c["positive"], c["constructed"]
    assert not bool((valid & ~pos & ~zero).any())                         # no undecided row
    assert not bool((pos & zero).any())
    assert bool((c["ce"][pos] >= 1e-3).all())
    if c["M"] > 300 and c["special"] != "all_invalid":
        assert bool(zero.any()) and bool(pos.any()) and bool((~valid).any())
    e = R.emu_unsup(c)
    assert torch.equal(e["sel"], c["sel"])                                # fp32 CE > 0 selects exactly the decided positives
    held(f"unsup loss case {i}", e, c, ("loss", "dx"))
    assert bool((c["conf"] == R.UNSUP_THR).any())
    if c["special"] == "one_invalid":
        b = c["B"] // 2
        assert not bool(valid[b * c["P"]:(b + 1) * c["P"]].any()) and not bool(c["has"][b]) and int(c["has"].sum()) == c["B"] - 1
        assert math.isfinite(float(c["ref"]["loss"])) and bool((c["ref"]["dx"][b * c["P"]:(b + 1) * c["P"]] == 0).all())
    if c["special"] == "all_invalid":
        assert math.isnan(float(c["ref"]["loss"]))


def test_unsup_and_eqv_cases_cover_every_slab_count():
    for cs in (R.UNSUP_CASES, R.EQV_CASES):
        assert {c[0] for c in cs} == {1, 2, 3, 4, 7, 8, 9}
        assert {c[1] for c in cs} == {1, 255, 257, 131072 + 300}
        assert any(c[0] == 1 and c[1] > 512 * 256 for c in cs)
    assert {c[2] for c in R.UNSUP_CASES} == {2, 4, 19} and {c[2] for c in R.EQV_CASES} == {1, 4, 19}
    assert any(c[3] > 0 for c in R.UNSUP_CASES) and any(c[4] > 0 for c in R.UNSUP_CASES)
    assert any(c[3] > 0 and c[4] > 0 and c[3] != c[4] for c in R.EQV_CASES)
    assert {c[6] for c in R.UNSUP_CASES} == {None, "one_invalid", "all_invalid"}
    assert {c[6] for c in R.EQV_CASES} == {None, "same", "zero_mask"}


# ---- equivariance KL -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.EQV_CASES)))
def test_eqv_loss_bounds_hold_for_the_emulation(i):
    c = R.eqv_case(i)
    e = R.emu_eqv(c)
    held(f"eqv loss case {i}", e, c, ("loss", "den", "dp"))
    if c["special"] == "same":
        assert float(c["ref"]["loss"].abs()) < 1e-12 and float(e["loss"]) == 0.0 and bool((e["dp"] == 0).all())
    if c["special"] == "zero_mask":
        b, P = c["B"] // 2, c["P"]
        assert float(c["ref"]["den"][b]) == 1e-7 and bool((c["ref"]["dp"][b * P:(b + 1) * P] == 0).all())
    if c["M"] > 11 and c["special"] != "same" and c["C"] > 1:
        t32 = torch.softmax(c["q"], 1)
        assert bool((t32[c["sat"]][:, 1:] == 0).all())                    # t == 0 exactly: the t > 0 guard is reached
    if c["M"] > 11:
        assert bool(((c["m"] > 0) & (c["m"] < 1)).any())                  # a fractional mask


# ---- percentile masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.ENT_CASES)))
def test_entropy_mask_inputs_hold_their_edges(i):
    c = R.ent_case(i)
    name, ent, ok = c["name"], c["ent"], c["lab_u"] >= 0
    assert not bool(torch.isnan(ent).any())
    # a + (b - a) t evaluated with two roundings and with one fused rounding gives the same fp32 threshold
    assert torch.equal(c["thr32"].view(torch.int32), c["alt32"].view(torch.int32))
    assert bool((c["low"][:c["n_l"]] == (c["lab_l"] >= 0).float()).all())
    if name.startswith("n"):
        assert c["n_valid"] == int(name[1])
    if name == "n0":
        assert float(c["low"][c["n_l"]:].sum()) == 0 and float(c["high"][c["n_l"]:].sum()) == 0
    if name == "equal":
        assert float(c["low"].sum()) == 257 and float(c["high"].sum()) == 257
    if name == "half_at_thr":
        at = (ent == c["thr32"][0]) & ok
        assert int(at.sum()) == 128 and bool((c["low"][c["n_l"]:][at] == 1).all()) and bool((c["high"][c["n_l"]:][at] == 1).all())
    if name == "zeros":
        z = ent == 0
        assert bool(torch.signbit(ent[z]).any()) and bool((~torch.signbit(ent[z])).any())
        if c["q"][0] == 30.0:                                             # the threshold is a zero: both signs fall on the same side
            assert float(c["thr32"][0]) == 0.0 and bool((c["low"][c["n_l"]:][z] == 1).all())
    if name == "special":
        v = ent[ok]
        assert bool(torch.isinf(v).any()) and bool((v < 0).any()) and bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())
    if name == "bytes":
        keys = ent[ok].view(torch.int32).long() & 0xFFFFFFFF
        for byte in range(4):
            others = keys & ~(0xFF << (8 * byte))
            same = others.unique(return_counts=True)[1]
            assert int(same.max()) > 1, byte                              # values whose keys differ only in this byte
    if name == "big":
        assert c["n_u"] == 65536 + 300


def test_entropy_mask_cases_cover_the_listed_edges():
    cs = [R.ent_case(i) for i in range(len(R.ENT_CASES))]
    assert {c["n_valid"] for c in cs} >= {0, 1, 2, 3}
    qs = {q for c in cs for q in c["q"]}
    assert {0.0, 50.0, 100.0} <= qs
    fr = [f for c in cs if c["n_valid"] > 1 for f in c["frac"]]
    assert any(0 < f < 0.5 for f in fr) and any(f >= 0.5 for f in fr)
    assert any(c["n_u"] > 65536 and c["n_l"] == 0 for c in cs) and any(c["n_u"] > 65536 and c["n_l"] > 0 for c in cs)


# ---- exact kernels: the references hold their edges -------------------------------------------------------------------------------------
def test_exact_cases_cover_the_listed_edges():
    assert {(c[0], c[1]) for c in R.MIX_CASES} == {(m, b) for m in (0, 1, 2) for b in (1, 2, 33)}
    assert {c[2] for c in R.MIX_CASES} == {1, 3} and {c[3] for c in R.MIX_CASES} == {1, 3}
    for i, (mode, B, Z, Cimg) in enumerate(R.MIX_CASES):
        c = R.mix_case(i)
        if B == 1 and mode != 1:                                          # the partner is the image itself
            assert torch.equal(c["odata"], c["data"]) and torch.equal(c["otarget"], c["target"])
        if B == 33 and mode != 2:
            k = c["keep"].sum(1)
            assert int(k[0]) == c["keep"].shape[1] and int(k[1]) == 0 and int(k[2]) == c["keep"].shape[1] - 1
            assert not bool(c["keep"][2, -1])                             # the one-pixel box sits on the last row, column and slice
        if B == 33 and mode == 2:
            t, k = c["target"], c["keep"]
            for b, lab in ((0, 0), (1, 31), (2, 32), (3, 63)):
                assert bool((k[b] == (t[b] == lab)).all()) and bool((t[b] == lab).any())
            assert not bool(k[(t < 0) | (t >= 64)].any()) and bool((t == 1000).any()) and bool((t == 64).any())
            assert int(c["desc"][3, 7]) < 0                               # bit 63 arrives as a negative int
            assert bool((c["otarget"][31][~k[31]] == t[32][~k[31]]).all())        # the partner across the 32-image launch split
            assert bool((c["otarget"][32][~k[32]] == t[0][~k[32]]).all())         # ... and the wrap of the last image
    for hw in R.PRESENCE_HW:
        c = R.presence_case(hw)
        assert int(c["ref"][1]) == 0 and int(c["ref"][2]) == -(1 << 63)
    assert {c[0] for c in R.OVERLAP_CASES} == {1, 257, 262144 + 300} and {c[1] for c in R.OVERLAP_CASES} == {1, 2, 19, 32}
    c = R.window_case(5, 1)
    ww, hh, dd = R.WINDOW_VOL
    (px, py, pz), starts = c["patch"], c["starts"]
    assert pz == 1 and (starts[-1][0] + px, starts[-1][1] + py, starts[-1][2] + pz) == (ww, hh, dd)
    assert float((c["acc_cnt"] - c["cnt0"]).max()) >= 2                   # overlapping windows
    assert bool((c["score"][0] == c["score"][4]).any()) and bool((c["label"][c["score"][0] == c["score"].max(0).values] == 0).all())


# ---- TPS grid, grid_sample, AdvMorph fields -----------------------------------------------------------------------------------------------
def test_tps_grid_bound_holds_for_the_emulation():
    w = 0.0
    for nr in R.TPS_NR:
        for b in R.TPS_B:
            for hw in R.TPS_HW:
                c = R.tps_case(nr, b, hw)
                w = max(w, worst(R.emu_tps(c), c["ref"], c["tol"]))
    report("tps grid", w)


@pytest.mark.parametrize("border", (0, 1))
@pytest.mark.parametrize("i", range(len(R.GS_CASES)))
def test_grid_sample_bound_holds_for_the_emulation(i, border):
    c = R.gs_case(i, border)
    report(f"grid sample case {i} border {border}", worst(R.emu_grid_sample(c), c["ref"], c["tol"]))
    g = c["grid"]
    assert bool((g == -1).any()) and bool((g == 1).any()) and bool((g.abs() == 3).any() or g.shape[0] < 16) and float(g.abs().max()) <= 3
    assert bool(((g.abs() > 1) & (g.abs() < 1.0001)).any())              # just outside


def test_grid_sample_cases_cover_the_listed_edges():
    cs = R.GS_CASES
    assert {c[3] for c in cs} == {1, 3} and {c[4] for c in cs} == {1, 5}
    assert any(c[1] == 1 for c in cs) and any(c[2] == 1 for c in cs) and any(c[5] > 0 for c in cs) and any(c[6] > 0 for c in cs)
    assert any((c[7], c[8]) != (c[1], c[2]) for c in cs)
    # zeros mode: a tap outside contributes 0 - at grid = +-3 every tap is outside
    c = R.gs_case(0, 0)
    far = (c["grid"].abs() == 3).any(1)
    rows = far.view(-1, 1).expand(-1, c["D3"]).reshape(-1)
    assert bool(far.any()) and bool((c["ref"][rows] == 0).all())


def test_field_axpb_bound_holds_for_the_emulation():
    w = 0.0
    for i in range(len(R.AXPB_SHAPES)):
        for a in (False, True):
            for b in (False, True):
                for cl in (False, True):
                    c = R.axpb_case(i, a, b, cl)
                    w = max(w, worst(R.emu_axpb(c), c["ref"], c["tol"]))
    report("field axpb", w)
    assert float(R.emu_linspace(1)[0]) == -1.0 and {s[2] % 2 for s in R.AXPB_SHAPES if s[2] > 1} == {0, 1}
    assert any(s[1] == 1 for s in R.AXPB_SHAPES) and any(s[2] == 1 for s in R.AXPB_SHAPES)


def test_field_smooth_and_resize_bounds_hold_for_the_emulation():
    w = 0.0
    for ks in R.SMOOTH_KS:
        for si in range(len(R.SMOOTH_SHAPES)):
            c = R.smooth_case(ks, si)
            w = max(w, worst(c["emu"], c["ref"], c["tol"]))
    report("field smooth", w)
    w = 0.0
    for i in range(len(R.RESIZE_CASES)):
        c = R.resize_case(i)
        e = R.emu_resize(c)
        w = max(w, worst(e, c["ref"], c["tol"]))
        if c["same"]:
            assert torch.equal(e, c["x"])                                 # equal sizes: the identity, bit for bit
    report("field resize", w)
    assert any(c[1] == 1 for c in R.RESIZE_CASES) and any(c[3] > c[1] for c in R.RESIZE_CASES) and any(c[3] < c[1] for c in R.RESIZE_CASES)


# ---- the comparison helpers reject planted errors ------------------------------------------------------------------------------------------
def test_helpers_reject_planted_errors():
    c = R.softmax_case(5)
    for k in ("prob", "maxp", "ent"):
        good = c["ref"][k].float()
        assert worst(good, c["ref"][k], c["tol"][k]) <= 1.0               # the rounded reference itself passes
        bad = good.clone()
        j = bad.numel() // 2
        bad.view(-1)[j] += 4 * float(c["tol"][k].reshape(-1)[j]) + 2 * float(good.view(-1)[j].abs()) * 2.0 ** -23
        assert worst(bad, c["ref"][k], c["tol"][k]) > 1.0                 # one wrong element
    s = R.sup_case(4)
    dx = s["ref"]["dx"].float()
    bad = dx.clone()
    bad[100, 1] += 4 * float(s["tol"]["dx"][100, 1]) + 2.0 ** -22 * float(dx[100, 1].abs())
    assert worst(dx, s["ref"]["dx"], s["tol"]["dx"]) <= 1.0 < worst(bad, s["ref"]["dx"], s["tol"]["dx"])
    nan = dx.clone()
    nan[7, 0] = math.nan
    assert worst(nan, s["ref"]["dx"], s["tol"]["dx"]) == math.inf
    buf = torch.full((s["M"], s["ldo"]), SENTINEL)
    buf[:, :s["C"]] = dx
    assert pad_ok(buf, s["C"])
    buf[s["M"] - 1, s["C"]] = 0.0                                         # one touched pad column
    assert not pad_ok(buf, s["C"])
    o = R.onehot_case(1)
    assert exact(o["ref"].clone(), o["ref"])
    lab = o["lab"].clone()
    lab[17] = (lab[17].clamp_min(0) + 1) % o["C"]                         # a label off by one
    moved = torch.zeros((o["M"], o["C"]), dtype=torch.int64)
    moved[torch.arange(o["M"]), lab.clamp_min(0)] = 1
    assert not exact(moved.view(o["M"] // o["P"], o["P"], o["C"]).permute(0, 2, 1).contiguous(), o["ref"])
    a = R.softmax_case(5)["amax"].clone()
    a[3] += 1
    assert not exact(a, R.softmax_case(5)["amax"])
    e = R.ent_case(8)
    low = e["low"].clone()
    low[e["n_l"] + 5] = 1 - low[e["n_l"] + 5]
    assert exact(e["low"].clone(), e["low"]) and not exact(low, e["low"])
    ov = R.overlap_case(2)
    cnt = ov["ref"].clone()
    cnt[4] += 1
    assert not exact(cnt, ov["ref"])


# ---- argument checks (host side) ---------------------------------------------------------------------------------------------------------
def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses that are
    never dereferenced."""
    import arco_amd._lib as L
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    bad = -1
    assert lib.arco_softmax_rows(p, 33, 4, 33, 4, p, p, p, p, None) == bad
    assert lib.arco_softmax_rows(p, 4, 4, 0, 4, p, p, p, p, None) == bad
    assert lib.arco_overlap_counts(p, p, 4, 33, p, None) == bad
    assert lib.arco_field_smooth(p, 1, 2, 3, 2, 2, p, p, None) == bad and lib.arco_field_smooth(p, 1, 2, 3, 2, 11, p, p, None) == bad
    # label_onehot: lab, M, C, P, out
    for args in ((None, 4, 4, 4, p), (p, 4, 4, 4, None), (p, 0, 4, 4, p), (p, 4, 0, 4, p), (p, 4, 4, 0, p)):
        assert lib.arco_label_onehot(*args, None) == bad, args
    # sup_loss_bwd: X, ld, M, C, lab, ws, g_ce, g_dice, dX, ldo
    ok = [p, 4, 4, 4, p, p, p, p, p, 4]
    for pos, val in ((0, None), (4, None), (5, None), (6, None), (7, None), (8, None), (2, 0), (3, 0), (3, 33)):
        args = list(ok)
        args[pos] = val
        assert lib.arco_sup_loss_bwd(*args, None) == bad, (pos, val)
    # unsup_loss_bwd: X, ld, B, P, C, lab, ws, g, dX, ldo
    ok = [p, 4, 2, 4, 4, p, p, p, p, 4]
    for pos, val in ((0, None), (5, None), (6, None), (7, None), (8, None), (2, 0), (3, 0), (4, 0), (4, 33)):
        args = list(ok)
        args[pos] = val
        assert lib.arco_unsup_loss_bwd(*args, None) == bad, (pos, val)
    # eqv_loss_bwd: P, ldp, Q, ldq, mask, B, P, C, ws, g, dP, ldo
    ok = [p, 4, p, 4, p, 2, 4, 4, p, p, p, 4]
    for pos, val in ((0, None), (2, None), (4, None), (8, None), (9, None), (10, None), (5, 0), (6, 0), (7, 0)):
        args = list(ok)
        args[pos] = val
        assert lib.arco_eqv_loss_bwd(*args, None) == bad, (pos, val)
    # the forward partners keep their checks
    assert lib.arco_sup_loss_fwd(p, 33, 4, 33, p, p, p, None) == bad and lib.arco_unsup_loss_fwd(p, 33, 1, 4, 33, p, p, 0.5, p, p, None) == bad
    assert lib.arco_dice_probs_fwd(p, 33, 4, 33, p, None, p, p, None) == bad and lib.arco_dice_probs_bwd(p, 33, 4, 33, p, None, p, p, p, 33, None) == bad
    assert lib.arco_eqv_loss_fwd(p, 4, p, 4, p, 0, 4, 4, p, p, None) == bad
