"""CPU companion of tests/test_loss_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * every toleranced comparison: the kernel's formula emulated in torch fp32 (torch's own summation order, the one f16 widening where
    it applies) stays inside the SAME per-element bound against the SAME float64 reference; the worst ratios are printed and recorded
    in the GPU file's docstring;
  * the input conditions the GPU file relies on hold for its inputs: share of pixels with tied probabilities (>= 20 % wherever C > 1),
    the forced pixels, every counter column zero in one case and nonzero in another, the 0 / 1 / 63 / 64 wave block, the capped grids
    (more than one trip, a short last slab), every lpr and both NDI (and never NDI 4), cosines of exactly +1 / -1 / 0, finite references
    in the deepest-underflow case, rows on both sides of the eps clamp;
  * every comparison helper rejects a planted error: one element off by 4 x its tolerance, two swapped list entries, a count off by
    one, a dropped last row, a nonzero pad column;
  * the alignment contract of arco_gather_rows is rejected on the host (ARCO_ERR_ARG before anything is launched)."""
import ctypes
import math

import pytest
import torch

import loss_kernel_refs as R


def report(name, ratio, limit=1.0):
    print(f"emulated {name}: worst err / bound {ratio:.3f}")
    assert ratio <= limit, (name, ratio)


# ---- mask inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.MASK_CASES)))
def test_mask_inputs_tie_and_the_kernel_formula_matches_the_sort(i):
    c = R.mask_case(i)
    C, n = c["C"], c["n_pix"]
    print(f"case {i}: n_pix {n}  C {C}  tie share {c['tie_share']:.3f}")
    if C > 1:
        assert c["tie_share"] >= 0.2                                   # a single class cannot tie
    assert torch.equal(R.emulate_mask_codes(c), c["codes"])            # comparison-count rank == stable descending sort rank
    p = c["prob"]
    assert bool((p[n - 1] == p[n - 1, 0]).all())                       # all C probabilities equal
    if n >= 3 and not c["forced"]:
        assert float(p[n - 2, 0]) == R.DELTA_P and float(p[n - 3, 0]) == R.DELTA_N
        # p == delta_p is NOT an anchor, p == delta_n is NOT hard (strict comparisons)
        assert not bool(c["anchor"][0, n - 2]) and not bool(c["neg"][0, n - 3])
    if c["forced"]:
        waves = c["anchor"][0, :256].view(4, 64).sum(1).tolist()
        assert waves == [0, 1, 63, 64], waves
    if n > 65536:
        per = (c["nblocks"] + 255) // 256
        assert c["nblocks"] > 256 and per == 2 and 255 * per >= c["nblocks"]        # threads with an empty range


def test_mask_cases_cover_the_listed_edges():
    cases = [R.mask_case(i) for i in range(len(R.MASK_CASES))]
    assert {c["C"] for c in cases} == {1, 2, 4, 19, 21}
    assert {c["n_pix"] for c in cases} == {1, 255, 256, 257, 65536 + 300}
    assert {(c["n_l"], c["n_u"]) for c in cases} >= {(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)}
    assert any(c["forced"] for c in cases)
    assert any(c["n_pix"] >= 3 and not c["forced"] and c["totals"].sum() > 0 for c in cases)
    for C in (1, 2, 4, 19, 21):
        tot = torch.stack([c["totals"] for c in cases if c["C"] == C])
        assert bool((tot == 0).any(0).all()) and bool((tot > 0).any(0).all()), C      # every column zero once and nonzero once
        ranks = {(c["low"], c["high"]) for c in cases if c["C"] == C}
        assert any(lo == 0 for lo, hi in ranks) or C >= 19
    allr = {(c["low"], c["high"], c["C"]) for c in cases}
    assert any(lo == 0 for lo, hi, C in allr) and any(hi == C for lo, hi, C in allr) and any(lo == C for lo, hi, C in allr)
    assert any(lo == hi for lo, hi, C in allr)


# ---- row sums ------------------------------------------------------------------------------------------------------------------------
def test_row_sum_cases_reach_every_path():
    lprs, ndis = set(), set()
    for (d, C, n, _, _, _) in R.ROW_SUM_CASES:
        geo = R.row_sum_geometry(n, d, 64, 1024)
        lprs.add(geo["lpr"])
        ndis.add(geo["ndi"])
    assert lprs == {1, 2, 8, 16, 64} and ndis == {1, 2}
    for d in range(4, 513, 4):                                         # D <= 512: lpr reaches 64, so NDI is 1 or 2 - never 4
        assert R.row_sum_geometry(1000, d, 64, 1024)["ndi"] <= 2
    big = R.row_sum_geometry(1024 * 64 + 77, 4, 64, 1024)
    # 1024 slabs of 65 rows: one row more than the 64 rows of a wave step (a second wave of the block works), a short last slab,
    # and - rows_per_block being rounded up - slabs past the end that must come out as zeros
    assert big["grid"] == 1024 and big["rpb"] > big["rpw"] and 0 < big["last"] < big["rpb"] and big["empty"] > 0
    big = R.row_sum_geometry(2048 * 256 + 777, 4, 256, 2048)
    assert big["grid"] == 2048 and big["trips"] > 1 and 0 < big["last"] < big["rpb"] and big["empty"] > 0
    assert {c[1] for c in R.ROW_SUM_CASES} == {1, 8, 9, 21} and {c[0] for c in R.ROW_SUM_CASES} == {4, 8, 20, 64, 260, 496, 512}
    assert {1, 63, 64, 65, 1000} <= {c[2] for c in R.ROW_SUM_CASES}


@pytest.mark.parametrize("half", (False, True))
@pytest.mark.parametrize("i", range(len(R.ROW_SUM_CASES)))
def test_weighted_row_sum_bound_holds_for_the_emulation(i, half):
    c = R.weighted_case(i, half)
    d, C = c["d"], c["C"]
    if half:
        sub = (c["T"][:, :d].float().abs() < 2.0 ** -14) & (c["T"][:, :d] != 0)
        assert bool(sub.any()) or c["n"] < 8                           # f16 subnormals present
    w = c["W"][:, :C]
    assert bool((w == 0).any() or c["n"] < 8) and bool((w == 1).any() or c["n"] < 8) and bool(((w > 0) & (w < 1)).any() or c["n"] < 8)
    got = R.emulate_row_sum(c["T"][:, :d], w, None if c["totals"] is None else c["totals"].view(-1, 1))
    if C > 1:
        assert bool(torch.isnan(c["ref"][C - 1]).all()) if c["totals"] is not None else bool((c["ref"][C - 1] == 0).all())
    report(f"weighted row sum {'f16' if half else 'f32'} case {i}", R.worst(got, c["ref"], c["tol"]))


@pytest.mark.parametrize("i", range(len(R.PROTO_CASES)))
def test_masked_proto_bound_holds_for_the_emulation(i):
    c = R.proto_case(i)
    got = R.emulate_row_sum(c["T"][:, :c["d"]], c["lv"], c["totals"][:c["C"]].view(-1, 1))
    if c["C"] > 1:
        assert bool(torch.isnan(c["ref"][c["C"] - 1]).all())
    report(f"masked proto case {i}", R.worst(got, c["ref"], c["tol"]))


# ---- normalisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.NORM_D)
def test_normalize_bound_holds_for_the_emulation(D):
    worst = 0.0
    for n in R.NORM_N:
        for seed in range(8):
            c = R.norm_case(D, n, seed)
            y, inv = R.emulate_normalize(c["x"])
            zero = c["nrm"] == 0
            assert bool((y[zero] == 0).all()) and bool((inv[zero] == R.INV_EPS_F).all())
            worst = max(worst, R.worst(y, c["y"], c["ytol"]), R.worst(inv, c["inv"], c["itol"]))
        c = R.norm_case(D, 5, 0)
        assert float(c["nrm"][0]) == 0 and R.EPS_F < float(c["nrm"][1]) < R.EPS_F * 1.002 and R.EPS_F * 0.998 < float(c["nrm"][2]) < R.EPS_F
        assert float(c["inv"][2]) == 1 / R.EPS_F and float(c["inv"][1]) < 1 / R.EPS_F
    for lp in R.BANK_LP:
        c = R.banks_case(D, lp)
        assert set(c["lens"]) == {l for l in (1, 15, 16, 17, lp) if l <= lp}
        for e, b in enumerate(c["banks"]):
            y, _ = R.emulate_normalize(b)
            worst = max(worst, R.worst(y, c["bn"][e, :b.shape[0]], c["tol"][e, :b.shape[0]]))
            assert bool((c["bn"][e, b.shape[0]:] == 0).all())
    report(f"normalisation D={D}", worst)


# ---- InfoNCE -------------------------------------------------------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def emulate_staged(c, s32):
    """infonce_fwd_kernel / infonce_fused_kernel in fp32: running maximum, the sum of exponentials in double, lse = mx + (float) log"""
    E, q, dp = c["E"], c["q"], c["dp"]
    it = _f32(1.0) / _f32(c["temp"])
    m = c["M"]
    pos = (c["An"].view(E, q, dp) * c["Pn"][c["prow"]][:, None, :]).sum(-1)
    x = s32 * it
    mx = torch.maximum(pos * it, torch.where(m > 0, x, torch.full_like(x, -math.inf)).max(-1).values)
    ex = torch.where(m > 0, torch.exp(x - mx.unsqueeze(-1)), torch.zeros_like(x))
    tot = (m.double() * ex.double()).sum(-1) + torch.exp(pos * it - mx).double()
    lse = mx + tot.log().float()
    w = torch.where(m > 0, m.float() * torch.exp(x - lse.unsqueeze(-1)) * it, torch.zeros_like(x))
    return lse - pos * it, w, (torch.exp(pos * it - lse) - 1.0) * it


def emulate_score(c):
    """nce_score_kernel + nce_finish_kernel in fp32: fixed shift exp((s - 1) / T), bank norms from the raw rows, fp32 row sums"""
    E, q, dp, d, lp = c["E"], c["q"], c["dp"], c["d"], c["lp"]
    it, eps = _f32(1.0) / _f32(c["temp"]), _f32(R.EPS)
    an = c["An"].view(E, q, dp)
    pos = (an * c["Pn"][c["prow"]][:, None, :]).sum(-1)
    s = torch.zeros((E, q, lp))
    ib = torch.full((E, lp), float(1.0 / eps))
    for e, b in enumerate(c["banks"]):
        ib[e, :b.shape[0]] = 1.0 / torch.clamp((b * b).sum(1).sqrt(), min=eps)
        s[e, :, :b.shape[0]] = an[e, :, :d] @ b.t()
    s = s * ib.unsqueeze(1)
    m = c["M"]
    ex = torch.where(m > 0, m.float() * torch.exp((s - 1.0) * it), torch.zeros_like(s))
    wu = ex * ib.unsqueeze(1)
    epos = torch.exp((pos - 1.0) * it)
    tot = (ex.sum(-1).double() + epos.double()).float()
    loss = tot.log() - (pos - 1.0) * it
    return loss, wu, (epos / tot - 1.0) * it, it / tot, pos


@pytest.mark.parametrize("i", range(len(R.NCE_CASES)))
def test_nce_bounds_hold_for_the_emulated_routes(i):
    c = R.nce_case(i)
    s32 = c["cos"].float()
    ref = R.nce_ref(s32.double(), c["M"], c["pos"], c["temp"])
    assert all(bool(torch.isfinite(v).all()) for k, v in ref.items() if k in ("loss", "W", "gpos", "lse"))
    e_s, e_pos = R.staged_logit_errors(c, s32, ref)
    tols = R.nce_tols(ref, e_s, e_pos, R.staged_round_mag(ref))
    loss, w, gpos = emulate_staged(c, s32)
    assert bool((w[c["M"] == 0] == 0).all())
    report(f"staged InfoNCE case {i}", max(R.worst(loss, ref["loss"], tols["loss"]), R.worst(w, ref["W"], tols["W"]),
                                           R.worst(gpos, ref["gpos"], tols["gpos"])))
    ref = R.nce_ref(c["cos"], c["M"], c["pos"], c["temp"])
    assert all(bool(torch.isfinite(v).all()) for k, v in ref.items() if k in ("loss", "W", "gpos", "lse"))
    e_s, e_pos, k_ib = R.score_logit_errors(c, ref)
    tols = R.nce_tols(ref, e_s, e_pos, R.score_round_mag(ref), extra_rel=R.gamma(k_ib) + 4 * R.U)
    loss, wu, gpos, gscale, pos = emulate_score(c)
    wgt = gscale.double().unsqueeze(-1) * wu.double() * c["bnorm"].unsqueeze(1)
    report(f"score InfoNCE case {i}", max(R.worst(loss, ref["loss"], tols["loss"]), R.worst(wgt, ref["W"], tols["W"]),
                                          R.worst(gpos, ref["gpos"], tols["gpos"]), R.worst(pos, c["pos"], e_pos * ref["t"] + R.TINY)))


def test_nce_cases_hold_the_cosines_and_the_deepest_underflow():
    assert {c[0] for c in R.NCE_CASES} >= {1, 63, 64, 65} and {l for c in R.NCE_CASES for l in c[1]} >= {1, 127, 128, 129, 300}
    assert {c[2] for c in R.NCE_CASES} == {4, 16, 20, 496} and {c[3] for c in R.NCE_CASES} == {0.05, 0.5, 4.0}
    assert {len(c[1]) for c in R.NCE_CASES} >= {1, 3} and {l for c in R.NCE_CASES[6:] for l in c[1]} == {1, 2, 33, 257} and {c[4] for c in R.NCE_CASES} >= {1, 300, 4097}
    deep = 0
    for i in range(len(R.NCE_CASES)):
        c = R.nce_case(i)
        for e, l in enumerate(c["lens"]):
            cos = c["cos"][e, 0]
            assert float(c["pos"][e, 0]) == -1.0                           # anchor 0 against its prototype
            assert float(cos[0]) == 1.0
            if l > 2:
                assert float(cos[1]) == -1.0 and float(cos[2]) == 0.0
            if l > 3 and c["q"] > 2:
                assert bool((c["banks"][e][3] == 0).all()) and int(c["M"][e, 2, 3]) > 0       # zero bank row, sampled
                assert bool((c["cos"][e, :, 3] == 0).all())
            if l > 1:
                assert int(c["M"][e, 0, 1]) == c["nn"]                       # query 0: all negatives are row 1, cosine -1
                if c["temp"] == 0.05:
                    deep += 1
                    ref = R.nce_ref(c["cos"], c["M"], c["pos"], c["temp"])
                    assert math.isfinite(float(ref["loss"][e, 0])) and abs(float(ref["loss"][e, 0]) - math.log(c["nn"] + 1)) < 1e-9
                    assert math.exp(-2 / c["temp"]) > 2.0 ** -126             # exp((s - 1) / T) at s = -1 is a normal fp32 number
            if c["q"] > 1:
                assert int(c["M"][e, 1, l - 1]) == c["nn"]                   # query 1: one row Nn times through index -1
            assert bool((c["M"][e, :, l:] == 0).all())
    assert deep >= 2


# ---- anchor gradients, scatter, sum --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,dp", [(1, 4, 16), (4, 16, 16), (5, 20, 32), (5, 496, 496), (4, 65, 80)])
def test_anchor_grad_bound_holds_for_the_emulation(n, d, dp):
    worst = 0.0
    for shared in (True, False):
        for scaled in (False, True):
            c = R.grad_case(n, d, dp, shared)
            prow = torch.zeros(n, dtype=torch.int64) if shared else torch.arange(n)
            ref, tol = R.grad_ref(c, prow, scaled)
            assert bool(torch.isfinite(ref).all())
            assert bool((c["inv"][0] == R.INV_EPS_F).all()) and (n < 3 or float(c["inv"][2]) < R.INV_EPS_F)
            worst = max(worst, R.worst(R.emulate_anchor_grad(c, prow, scaled), ref, tol))
    report(f"anchor gradient n={n} D={d} Dp={dp}", worst)


@pytest.mark.parametrize("d,n,m", [(1, 0, 0), (4, 1, 1), (65, 9, 3), (16, 130, 64)])
def test_scatter_bound_holds_for_the_emulation(d, n, m):
    c = R.scatter_case(d, n, m, False)
    assert c["mult"] == m
    cl = R.scatter_case(d, n, m, True)
    assert torch.equal(cl["list"].long()[cl["idx"]], cl["rows"])
    ref, tol = R.scatter_ref(c, 1.5)
    got = c["dst"][:, :d].clone()
    got.index_add_(0, c["rows"], _f32(1.5) * c["src"][:, :d])
    report(f"scatter-add m={m}", R.worst(got, ref, tol))


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("n", R.SUM_N)
def test_sum_scale_bound_holds_for_the_emulation(n, accumulate):
    c = R.sum_case(n)
    assert bool((c["x"] > 0).any() or n == 1) and bool((c["x"] < 0).any() or n == 1)
    v = (c["x"].double().sum() * c["scale"]).float()
    got = _f32(c["before"]) + v if accumulate else v
    ref, tol = R.sum_ref(c, accumulate)
    report(f"sum_scale n={n}", R.worst(got.view(1), ref, tol))


# ---- the comparison helpers reject planted errors ------------------------------------------------------------------------------------
def test_helpers_reject_planted_errors():
    c = R.weighted_case(2, False)
    good = c["ref"].clone()
    assert R.worst(good, c["ref"], c["tol"]) == 0.0                     # NaN == NaN where the reference is NaN
    bad = good.clone()
    bad[1, 3] += 4 * c["tol"][1, 3]                                     # one element off by 4 x its tolerance
    assert 3.9 < R.worst(bad, c["ref"], c["tol"]) < 4.1
    bad = good.clone()
    bad[0, 0] = math.nan                                                # a NaN where none belongs
    assert R.worst(bad, c["ref"], c["tol"]) == math.inf
    bad = good.clone()
    bad[c["C"] - 1, 0] = 0.0                                            # a number where NaN belongs
    assert R.worst(bad, c["ref"], c["tol"]) == math.inf
    zero_tol = torch.zeros(3, dtype=torch.float64)
    assert R.worst(torch.tensor([0.0, 1e-30, 0.0]), zero_tol, zero_tol) == math.inf     # an exact zero is required: any value fails
    # lists
    m = R.mask_case(8)
    masks = torch.cat((m["anchor"], m["neg"]), 0)
    lists = torch.full(masks.shape, R.ISENT, dtype=torch.int32)
    for k in range(masks.shape[0]):
        nz = torch.nonzero(masks[k]).flatten().to(torch.int32)
        lists[k, :nz.shape[0]] = nz
    assert R.lists_ok(lists, masks)
    cnt = int(masks[0].sum())
    assert cnt >= 2
    bad = lists.clone()
    bad[0, 0], bad[0, 1] = lists[0, 1], lists[0, 0]                     # two swapped list entries
    assert not R.lists_ok(bad, masks)
    bad = lists.clone()
    bad[0, cnt - 1] = R.ISENT                                           # a dropped last row
    assert not R.lists_ok(bad, masks)
    bad = lists.clone()
    bad[0, cnt] = 0                                                     # an entry written beyond the prefix
    assert not R.lists_ok(bad, masks)
    # counts
    assert R.exact(m["counts"].to(torch.int32), m["counts"])
    bad = m["counts"].to(torch.int32).clone()
    bad[5, 1] += 1                                                      # a count off by one
    assert not R.exact(bad, m["counts"])
    mc = R.mult_case(3)
    bad = mc["ref"].to(torch.int32).clone()
    bad[0, mc["L"] - 1] -= 1
    assert R.exact(mc["ref"].to(torch.int32), mc["ref"]) and not R.exact(bad, mc["ref"])
    bank = torch.arange(12.0).view(4, 3)
    assert R.exact(bank.clone(), bank) and not R.exact(bank[:3], bank)  # a dropped last row
    # pads
    buf = torch.full((3, 8), R.SENTINEL)
    buf[:, :5] = 1.0
    assert R.pad_ok(buf, 5)
    buf[2, 6] = 0.0                                                     # a nonzero / overwritten pad column
    assert not R.pad_ok(buf, 5)
    bn = R.banks_case(16, 48)
    bad = bn["bn"].clone()
    bad[0, 40, 3] = 1e-20                                               # a pad row of Bn must be exactly 0
    assert R.worst(bad, bn["bn"], bn["tol"]) == math.inf


# ---- the alignment contract of arco_gather_rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,esize", [("arco_gather_rows", 4), ("arco_gather_rows_h", 2)])
def test_gather_rows_alignment_is_an_argument_error(name, esize):
    """Host side only: ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU.  D % 4 == 0 with a stride that is
    no multiple of 4, or a base pointer off its four-element alignment, is rejected; n == 0 with a valid layout is accepted."""
    import arco_amd._lib as L
    fn = getattr(L.load(), name)
    src = torch.zeros(64, dtype=torch.float64)                          # host memory: only the ADDRESS is looked at
    out = torch.zeros(64, dtype=torch.float64)
    ps, po = src.data_ptr() // 64 * 64 + 64, out.data_ptr() // 64 * 64 + 64
    V = ctypes.c_void_p
    assert fn(V(ps), 12, 8, None, None, None, 0, 0, V(po), 12, None) == 0
    for (a, lds, b, ldo) in [(ps, 9, po, 12), (ps, 12, po, 10), (ps + esize, 12, po, 12), (ps, 12, po + 4, 12), (ps, 12, po + 8, 12)]:
        assert fn(V(a), lds, 8, None, None, None, 0, 2, V(b), ldo, None) == -1, (a - ps, lds, b - po, ldo)
