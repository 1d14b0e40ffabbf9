"""Every entry point of csrc/glue.hip called DIRECTLY (arco_amd._lib), one kernel at a time, against a plain float64 / int64 reference
on the CPU computed from the same input values (tests/glue_kernel_refs.py) - not through the wrappers of glue.py / augment.py /
adv_morph.py, not against the oracle, a golden file or another HIP route - at the sizes one element past every grid cap, at every
class-count instantiation, with padded strides, and at the edges listed beside each case table.  Every output buffer is prefilled
with a sentinel (untouched pad columns and the guard elements behind each buffer must keep it); every test prints its worst
err / bound.  The backward kernels read the float64 sums / stats / denominators of the REFERENCE, written into the workspace by the
test, so that each kernel is held alone.

  exact (torch.equal): arco_label_onehot, arco_entropy_masks and arco_entropy_masks_phase (masks; the two forms agree bit for bit on
  the threshold pair), arco_mix_unsup, arco_label_presence, arco_overlap_counts, arco_window_accumulate + arco_score_finalize, the
  arg-max of arco_softmax_rows on every decided row, the unselected rows of the unsupervised-CE gradient, arco_field_resize at equal
  sizes.

  per-element bounds k u sum|terms| (u = 2^-24; derivations in tests/glue_kernel_refs.py; worst err / bound: CPU emulation | GPU)
  * arco_softmax_rows     prob 0.90 | 0.90   max 0.31 | 0.32   entropy 0.19 | 0.21
  * arco_sup_loss_fwd     out  0.23 | 0.23   sums 0.54 | 0.54  arco_sup_loss_bwd   0.76 | 0.74
  * arco_dice_probs_fwd   out  0.70 | 0.70   sums 0.84 | 0.84  arco_dice_probs_bwd 0.66 | 0.66
  * arco_unsup_loss_fwd   0.15 | 0.15                          arco_unsup_loss_bwd 0.49 | 0.48
  * arco_eqv_loss_fwd     0.06 | 0.06                          arco_eqv_loss_bwd   0.49 | 0.49
  * arco_tps_grid         0.99 | 0.99   arco_grid_sample_fwd 0.37 | 0.37
  * arco_field_axpb       0.32 | 0.25   arco_field_smooth    0.21 | 0.24   arco_field_resize 0.27 | 0.26
The emulation's figures are the largest printed by tests/test_glue_kernels_cpu.py, the GPU's the largest printed by this file on an
MI355X (every test prints its worst err / bound).  arco_tps_grid at NR = 1 is one rounded product against u |r m|: a ratio close
to 1 is the rounding itself."""
import ctypes

import numpy as np
import pytest
import torch

import glue_kernel_refs as R
from loss_kernel_refs import SENTINEL, exact, pad_ok, worst

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 8                                             # sentinel elements kept behind every output buffer


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def filled(n, dtype=torch.float32, value=SENTINEL):
    """n elements + GUARD, all holding the sentinel"""
    return torch.full((int(n) + GUARD,), value, dtype=dtype, device=DEV)


def body(buf, n, shape=None):
    """the first n elements of a guarded buffer on the CPU, after checking that the guard still holds the sentinel"""
    torch.cuda.synchronize()
    sent = SENTINEL if buf.dtype.is_floating_point else R.ISENT
    assert bool((buf[n:] == sent).all()), "the guard behind the buffer was written"
    out = buf[:n].cpu()
    return out if shape is None else out.view(shape)


def report(name, ratio):
    print(f"{name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def held(name, got, ref, tol):
    report(name, worst(got, ref, tol))


def ids(cases):
    return lambda i: "-".join(str(v) for v in cases[i])


# ---- (1) arco_softmax_rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SOFTMAX_CASES)), ids=ids(R.SOFTMAX_CASES))
def test_softmax_rows(L, i):
    """all four outputs together, then each alone (null pointers for the rest): the same bits.  Probabilities, max and entropy within
    their bounds; arg-max exact on every decided row (bit-equal rows: the first class); saturated rows: p == 1, entropy -0.0."""
    c = R.softmax_case(i)
    C, M, P, ld = c["C"], c["M"], c["P"], c["ld"]
    X = dev(c["X"])
    sizes = dict(prob=M * C, maxp=M, amax=M, ent=M)

    def run(which):
        b = {k: (filled(n, torch.int64, R.ISENT) if k == "amax" else filled(n)) if k in which else None for k, n in sizes.items()}
        L.call("arco_softmax_rows", L.ptr(X), ld, M, C, P, L.ptr(b["prob"]), L.ptr(b["maxp"]), L.ptr(b["amax"]), L.ptr(b["ent"]))
        return {k: body(v, sizes[k]) for k, v in b.items() if v is not None}

    got = run(tuple(sizes))
    held(f"softmax case {i} prob", got["prob"].view(M // P, C, P), c["ref"]["prob"], c["tol"]["prob"])
    held(f"softmax case {i} max", got["maxp"], c["ref"]["maxp"], c["tol"]["maxp"])
    held(f"softmax case {i} entropy", got["ent"], c["ref"]["ent"], c["tol"]["ent"])
    dec = c["decided"]
    assert exact(got["amax"][dec], c["amax"][dec])
    assert bool((got["amax"][c["equal"]] == 0).all())
    sat = c["sat"]
    if bool(sat.any()):
        assert bool((got["maxp"][sat] == 1.0).all()) and bool((got["ent"][sat] == 0).all()) and bool(torch.signbit(got["ent"][sat]).all())
    for k in sizes:
        alone = run((k,))
        assert torch.equal(alone[k], got[k]), k


# ---- (2) arco_label_onehot -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.ONEHOT_CASES)), ids=ids(R.ONEHOT_CASES))
def test_label_onehot(L, i):
    c = R.onehot_case(i)
    C, M, P = c["C"], c["M"], c["P"]
    lab = dev(c["lab"])
    out = filled(M * C, torch.int64, R.ISENT)
    L.call("arco_label_onehot", L.ptr(lab), M, C, P, L.ptr(out))
    assert exact(body(out, M * C, (M // P, C, P)), c["ref"])
    print(f"label onehot case {i}: exact")


# ---- (3) supervised CE + Dice, Dice on probabilities ------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.SUP_CASES)), ids=ids(R.SUP_CASES))
def test_sup_loss_fwd_and_bwd(L, i):
    c = R.sup_case(i)
    C, M, ld, ldo = c["C"], c["M"], c["ld"], c["ldo"]
    npq = 2 + 3 * C
    X, lab = dev(c["X"]), dev(c["lab"])
    nws = L.query("arco_seg_ws_doubles", M, C, 1)
    off = 1024 * npq
    assert off + npq <= nws
    ws, out = filled(nws, torch.float64), filled(2)
    L.call("arco_sup_loss_fwd", L.ptr(X), ld, M, C, L.ptr(lab), L.ptr(ws), L.ptr(out))
    held(f"sup loss fwd case {i} out", body(out, 2), c["ref"]["out"], c["tol"]["out"])
    held(f"sup loss fwd case {i} sums", body(ws, nws)[off:off + npq], c["ref"]["sums"], c["tol"]["sums"])
    ws2 = filled(nws, torch.float64)
    ws2[off:off + npq] = dev(c["ref"]["sums"])
    dx = filled(M * ldo)
    g_ce, g_dice = dev(torch.tensor([R.G_CE])), dev(torch.tensor([R.G_DICE]))
    L.call("arco_sup_loss_bwd", L.ptr(X), ld, M, C, L.ptr(lab), L.ptr(ws2), L.ptr(g_ce), L.ptr(g_dice), L.ptr(dx), ldo)
    got = body(dx, M * ldo, (M, ldo))
    assert pad_ok(got, C)
    held(f"sup loss bwd case {i}", got[:, :C], c["ref"]["dx"], c["tol"]["dx"])


@pytest.mark.parametrize("weighted", (False, True), ids=("w_null", "w"))
@pytest.mark.parametrize("i", range(len(R.SUP_CASES)), ids=ids(R.SUP_CASES))
def test_dice_probs_fwd_and_bwd(L, i, weighted):
    c = R.dice_case(i, weighted)
    C, M, ld, ldo = c["C"], c["M"], c["ld"], c["ldo"]
    Pm, lab, w = dev(c["Pm"]), dev(c["lab"]), dev(c["w32"])
    nws = L.query("arco_seg_ws_doubles", M, C, 1)
    off = 1024 * 3 * C
    assert off + 3 * C <= nws
    ws, out = filled(nws, torch.float64), filled(1)
    L.call("arco_dice_probs_fwd", L.ptr(Pm), ld, M, C, L.ptr(lab), L.ptr(w), L.ptr(ws), L.ptr(out))
    held(f"dice probs fwd case {i} out", body(out, 1), c["ref"]["out"], c["tol"]["out"])
    held(f"dice probs fwd case {i} sums", body(ws, nws)[off:off + 3 * C], c["ref"]["sums"], c["tol"]["sums"])
    ws2 = filled(nws, torch.float64)
    ws2[off:off + 3 * C] = dev(c["ref"]["sums"])
    dp = filled(M * ldo)
    g = dev(torch.tensor([R.G_DICE]))
    L.call("arco_dice_probs_bwd", L.ptr(Pm), ld, M, C, L.ptr(lab), L.ptr(w), L.ptr(ws2), L.ptr(g), L.ptr(dp), ldo)
    got = body(dp, M * ldo, (M, ldo))
    assert pad_ok(got, C)
    held(f"dice probs bwd case {i}", got[:, :C], c["ref"]["dp"], c["tol"]["dp"])


# ---- (4) unsupervised CE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.UNSUP_CASES)), ids=ids(R.UNSUP_CASES))
def test_unsup_loss_fwd_and_bwd(L, i):
    """An image whose labels are all -1 contributes nothing (the reference arithmetic never selects one of its pixels): the loss stays
    finite and its gradient rows are zero.  unsup_loss_final_kernel skips such an image: its w_b = n_conf / 0 is inf or NaN, and
    w_b * S_b with S_b = 0 would turn the loss of the whole batch into NaN.  All images invalid: NaN on both sides."""
    c = R.unsup_case(i)
    B, P, C, M, ld, ldo = c["B"], c["P"], c["C"], c["M"], c["ld"], c["ldo"]
    X, lab, conf = dev(c["X"]), dev(c["lab"]), dev(c["conf"])
    nblk = L.query("arco_loss_slabs", B)
    off, nws = nblk * 4 * B, nblk * 4 * B + B + 1
    ws, out = filled(nws, torch.float64), filled(1)
    L.call("arco_unsup_loss_fwd", L.ptr(X), ld, B, P, C, L.ptr(lab), L.ptr(conf), R.UNSUP_THR, L.ptr(ws), L.ptr(out))
    loss = body(out, 1)
    print(f"unsup loss fwd case {i}: loss {float(loss):.6f}  reference {float(c['ref']['loss']):.6f}")
    held(f"unsup loss fwd case {i}", loss, c["ref"]["loss"], c["tol"]["loss"])
    stats = body(ws, nws)[off:]
    assert float(stats[B]) == float(c["ref"]["stats"][B])                                    # the number of selected rows
    has = c["has"]
    held(f"unsup loss fwd case {i} weights", stats[:B][has], c["ref"]["stats"][:B][has], 1e-15 * c["ref"]["stats"][:B][has] + R.TINY)
    ws2 = filled(nws, torch.float64)
    ws2[off:off + B + 1] = dev(c["ref"]["stats"])
    dx = filled(M * ldo)
    g = dev(torch.tensor([R.G_UNSUP]))
    L.call("arco_unsup_loss_bwd", L.ptr(X), ld, B, P, C, L.ptr(lab), L.ptr(ws2), L.ptr(g), L.ptr(dx), ldo)
    got = body(dx, M * ldo, (M, ldo))
    assert pad_ok(got, C)
    assert bool((got[:, :C][~c["sel"]] == 0).all())                                          # invalid and constructed-zero rows
    held(f"unsup loss bwd case {i}", got[:, :C], c["ref"]["dx"], c["tol"]["dx"])


# ---- (5) equivariance KL ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.EQV_CASES)), ids=ids(R.EQV_CASES))
def test_eqv_loss_fwd_and_bwd(L, i):
    c = R.eqv_case(i)
    B, P, C, M, ldp, ldq, ldo = c["B"], c["P"], c["C"], c["M"], c["ldp"], c["ldq"], c["ldo"]
    Pm, Qm, m = dev(c["Pm"]), dev(c["Qm"]), dev(c["m"])
    nblk = L.query("arco_loss_slabs", B)
    off, nws = nblk * 2 * B, nblk * 2 * B + B
    ws, out = filled(nws, torch.float64), filled(1)
    L.call("arco_eqv_loss_fwd", L.ptr(Pm), ldp, L.ptr(Qm), ldq, L.ptr(m), B, P, C, L.ptr(ws), L.ptr(out))
    held(f"eqv loss fwd case {i}", body(out, 1), c["ref"]["loss"], c["tol"]["loss"])
    held(f"eqv loss fwd case {i} den", body(ws, nws)[off:], c["ref"]["den"], c["tol"]["den"])
    ws2 = filled(nws, torch.float64)
    ws2[off:off + B] = dev(c["ref"]["den"])
    dp = filled(M * ldo)
    g = dev(torch.tensor([R.G_EQV]))
    L.call("arco_eqv_loss_bwd", L.ptr(Pm), ldp, L.ptr(Qm), ldq, L.ptr(m), B, P, C, L.ptr(ws2), L.ptr(g), L.ptr(dp), ldo)
    got = body(dp, M * ldo, (M, ldo))
    assert pad_ok(got, C)
    held(f"eqv loss bwd case {i}", got[:, :C], c["ref"]["dp"], c["tol"]["dp"])
    if c["special"] == "zero_mask":
        b = B // 2
        assert bool((got[b * P:(b + 1) * P, :C] == 0).all())


# ---- (6) percentile masks --------------------------------------------------------------------------------------------------------------
def same_f32(a, b):
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("i", range(len(R.ENT_CASES)), ids=ids(R.ENT_CASES))
def test_entropy_masks_one_shot_and_in_phases(L, i):
    c = R.ent_case(i)
    n_l, n_u, (q_lo, q_hi) = c["n_l"], c["n_u"], c["q"]
    n = n_l + n_u
    ent, lab_u = dev(c["ent"]), dev(c["lab_u"])
    lab_l = dev(torch.cat((c["lab_l"], torch.zeros(1, dtype=torch.int64))))                  # never empty; the extra label is not read
    nbytes = L.query("arco_sel_state_bytes")
    o_thr = L.query("arco_sel_state_offset", 1) - 16                                          # double thr[2] stands in front of hist
    assert nbytes % 8 == 0 and o_thr % 8 == 0

    def thr_bits(state):
        torch.cuda.synchronize()
        return state.cpu().view(torch.int64)[o_thr // 8:o_thr // 8 + 2].clone()

    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    low, high = filled(n), filled(n)
    L.call("arco_entropy_masks", L.ptr(ent), L.ptr(lab_l), L.ptr(lab_u), n_l, n_u, q_lo, q_hi, L.ptr(state), L.ptr(low), L.ptr(high))
    low1, high1, thr1 = body(low, n), body(high, n), thr_bits(state)
    t32 = thr1.view(torch.float64).float()
    print(f"entropy masks case {i}: thr {thr1.view(torch.float64).tolist()}  reference {c['thr']}")
    assert same_f32(t32, c["thr32"]) or same_f32(t32, c["alt32"])
    assert exact(low1, c["low"]) and exact(high1, c["high"])
    assert exact(low1[:n_l], (c["lab_l"] >= 0).float())

    state2 = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    low2, high2 = filled(n), filled(n)

    def phase(ph, ps=0):
        L.call("arco_entropy_masks_phase", ph, ps, L.ptr(ent), L.ptr(lab_l), L.ptr(lab_u), n_l, n_u, q_lo, q_hi, L.ptr(state2),
               L.ptr(low2), L.ptr(high2))
    phase(0)
    phase(1)
    for ps in range(4):
        phase(2, ps)
        phase(3, ps)
    phase(4)
    assert torch.equal(thr_bits(state2), thr1)                                                # the same threshold pair, bit for bit
    assert torch.equal(body(low2, n), low1) and torch.equal(body(high2, n), high1)


# ---- (7) mixer, label presence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.MIX_CASES)), ids=ids(R.MIX_CASES))
def test_mix_unsup(L, i):
    c = R.mix_case(i)
    B, Z, Cimg, H, W = c["B"], c["Z"], c["Cimg"], c["H"], c["W"]
    HW = H * W * Z
    data, target, logits = dev(c["data"]), dev(c["target"]), dev(c["logits"])
    desc = (ctypes.c_int * (8 * B))(*[int(v) for v in c["desc"].flatten().tolist()])
    od, ot, ol = filled(B * Cimg * HW), filled(B * HW, torch.int64, R.ISENT), filled(B * HW)
    L.call("arco_mix_unsup", L.ptr(data), Cimg, L.ptr(target), L.ptr(logits), B, H, W, Z, desc, c["mode"], L.ptr(od), L.ptr(ot), L.ptr(ol))
    assert exact(body(od, B * Cimg * HW, (B, Cimg, HW)), c["odata"])
    assert exact(body(ot, B * HW, (B, HW)), c["otarget"])
    assert exact(body(ol, B * HW, (B, HW)), c["ologits"])
    print(f"mix unsup case {i}: exact")


@pytest.mark.parametrize("hw", R.PRESENCE_HW)
def test_label_presence(L, hw):
    c = R.presence_case(hw)
    out = filled(3, torch.int64, R.ISENT)
    t = dev(c["target"])
    L.call("arco_label_presence", L.ptr(t), 3, hw, L.ptr(out))
    assert exact(body(out, 3), c["ref"])
    print(f"label presence HW {hw}: exact")


# ---- (8) overlap counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.OVERLAP_CASES)), ids=ids(R.OVERLAP_CASES))
def test_overlap_counts(L, i):
    c = R.overlap_case(i)
    out = filled(3 * c["C"], torch.int64, R.ISENT)
    pred, gt = dev(c["pred"]), dev(c["gt"])
    L.call("arco_overlap_counts", L.ptr(pred), L.ptr(gt), c["n"], c["C"], L.ptr(out))
    assert exact(body(out, 3 * c["C"]), c["ref"])
    print(f"overlap counts case {i}: exact")


# ---- (9) sliding-window accumulation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pz", sorted(R.WINDOW_SETS))
@pytest.mark.parametrize("C", R.WINDOW_C)
def test_window_accumulate_and_finalize(L, C, pz):
    c = R.window_case(C, pz)
    ww, hh, dd = R.WINDOW_VOL
    vol = ww * hh * dd
    px, py, pz_ = c["patch"]
    score, cnt = filled(C * vol), filled(vol)
    score[:C * vol], cnt[:vol] = dev(c["score0"]).flatten(), dev(c["cnt0"]).flatten()
    for p, (xs, ys, zs) in zip(c["probs"], c["starts"]):
        assert xs + px <= ww and ys + py <= hh and zs + pz_ <= dd
        pd = dev(p)
        L.call("arco_window_accumulate", L.ptr(pd), C, px, py, pz_, L.ptr(score), L.ptr(cnt), ww, hh, dd, xs, ys, zs)
    assert exact(body(score, C * vol, (C, ww, hh, dd)), c["acc_score"]) and exact(body(cnt, vol, (ww, hh, dd)), c["acc_cnt"])
    label = filled(vol, torch.int64, R.ISENT)
    L.call("arco_score_finalize", L.ptr(score), L.ptr(cnt), C, vol, L.ptr(label))
    s = body(score, C * vol, (C, ww, hh, dd))
    lab = body(label, vol, (ww, hh, dd))
    assert exact(s, c["score"])
    assert exact(lab, torch.from_numpy(np.argmax(s.numpy(), 0))) and exact(lab, c["label"])   # the first maximum of its own scores
    print(f"window accumulate C {C} pz {pz}: exact")


# ---- (10) TPS grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr", R.TPS_NR)
def test_tps_grid(L, nr):
    w = 0.0
    for b in R.TPS_B:
        for hw in R.TPS_HW:
            c = R.tps_case(nr, b, hw)
            rep, mp = dev(c["rep"]), dev(c["mapping"])
            grid = filled(b * hw * 2)
            L.call("arco_tps_grid", L.ptr(rep), L.ptr(mp), b, hw, nr, L.ptr(grid))
            w = max(w, worst(body(grid, b * hw * 2, (b, hw, 2)), c["ref"], c["tol"]))
    report(f"tps grid NR {nr}", w)


# ---- (11) grid_sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", (0, 1))
@pytest.mark.parametrize("i", range(len(R.GS_CASES)), ids=ids(R.GS_CASES))
def test_grid_sample_fwd(L, i, border):
    c = R.gs_case(i, border)
    rows = c["NB"] * c["Ho"] * c["Wo"] * c["D3"]
    X, grid = dev(c["X"]), dev(c["grid"])
    Y = filled(rows * c["ldy"])
    L.call("arco_grid_sample_fwd", L.ptr(X), c["ldx"], c["NB"], c["H"], c["W"], c["D3"], c["C"], L.ptr(grid), c["Ho"], c["Wo"], border,
           L.ptr(Y), c["ldy"])
    got = body(Y, rows * c["ldy"], (rows, c["ldy"]))
    assert pad_ok(got, c["C"])
    held(f"grid sample case {i} border {border}", got[:, :c["C"]], c["ref"], c["tol"])


# ---- (12) AdvMorph fields ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.AXPB_SHAPES)), ids=ids(R.AXPB_SHAPES))
def test_field_axpb(L, i):
    w = 0.0
    for has_in in (False, True):
        for has_in2 in (False, True):
            for clamp in (False, True):
                c = R.axpb_case(i, has_in, has_in2, clamp)
                n = c["B"] * c["H"] * c["W"] * 2
                a, b = dev(c["a"]), dev(c["b"])
                out = filled(n)
                L.call("arco_field_axpb", L.ptr(a), R.AXPB_ALPHA, R.AXPB_BETA, L.ptr(b), R.AXPB_GAMMA, c["B"], c["H"], c["W"], int(clamp),
                       L.ptr(out))
                w = max(w, worst(body(out, n, (c["B"], c["H"], c["W"], 2)), c["ref"], c["tol"]))
    report(f"field axpb shape {i}", w)


@pytest.mark.parametrize("si", range(len(R.SMOOTH_SHAPES)))
@pytest.mark.parametrize("ks", R.SMOOTH_KS)
def test_field_smooth(L, ks, si):
    c = R.smooth_case(ks, si)
    n = c["B"] * c["H"] * c["W"] * c["C"]
    x = dev(c["x"])
    wh = (ctypes.c_float * (ks * ks))(*c["w"].flatten().tolist())
    out = filled(n)
    L.call("arco_field_smooth", L.ptr(x), c["B"], c["H"], c["W"], c["C"], ks, wh, L.ptr(out))
    held(f"field smooth ks {ks} shape {si}", body(out, n, tuple(c["ref"].shape)), c["ref"], c["tol"])


@pytest.mark.parametrize("i", range(len(R.RESIZE_CASES)), ids=ids(R.RESIZE_CASES))
def test_field_resize(L, i):
    c = R.resize_case(i)
    n = c["B"] * c["H"] * c["W"] * c["C"]
    x = dev(c["x"])
    out = filled(n)
    L.call("arco_field_resize", L.ptr(x), c["B"], c["h"], c["w"], c["C"], c["H"], c["W"], L.ptr(out))
    got = body(out, n, tuple(c["ref"].shape))
    held(f"field resize case {i}", got, c["ref"], c["tol"])
    if c["same"]:
        assert exact(got, c["x"])                                                             # equal sizes: the identity, bit for bit
