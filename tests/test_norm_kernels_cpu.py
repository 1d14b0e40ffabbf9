"""CPU companion of tests/test_norm_kernels_gpu.py (no GPU): the fp32 emulation of every kernel of the BatchNorm / GroupNorm family
(same order of operations, tests/norm_kernel_refs.py) stays inside the SAME bounds against the SAME float64 references the GPU file
uses; every input condition the GPU file relies on holds for its inputs; every comparison rejects a planted error; the host-side
argument checks return the error code without a launch.  Every toleranced test prints its worst err / bound."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import norm_kernel_refs as R
from loss_kernel_refs import U, exact, worst


def report(name, ratio):
    print(f"{name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


# ---- emulations inside the bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.STATS_CASES)))
def test_slab_bounds_hold_for_the_emulation(i, half):
    c = R.stats_case(i, half)
    X = c["X"]
    s, q = R.emu_slabs(X.numpy(), (X * X).numpy(), c["groups"], c["C"])
    s, q = R.stats_layout(s), R.stats_layout(q)
    if c["kind"] == "exact":
        assert exact(s, c["s"].float()) and exact(q, c["q"].float())
    report(f"chan_stats {R.STATS_CASES[i]} sum", worst(s, c["s"], c["ts"]))
    report(f"chan_stats {R.STATS_CASES[i]} sumsq", worst(q, c["q"], c["tq"]))


@pytest.mark.parametrize("i", range(len(R.FIN_CASES)))
def test_finalize_bounds_hold_for_the_emulation(i):
    c = R.fin_case(i)
    e = R.emu_finalize(c["s"], c["q"], c["C"], c["groups"], c["cnt"])
    f = c["fin"]
    report(f"bn_finalize {R.FIN_CASES[i]} mean", worst(e["m"], f["m"], f["tm"]))
    report(f"bn_finalize {R.FIN_CASES[i]} istd", worst(e["istd"], f["istd"], f["ti"]))
    upto = R.defer_from(c["mode"], c["groups"])
    rm, rv, tm, tv = R.running_ref(c["rm0"], c["rv0"], f, c["groups"], upto=upto)
    em, ev = R.emu_running(c["rm0"], c["rv0"], e, c["groups"], upto=upto)
    report(f"bn_finalize {R.FIN_CASES[i]} running_mean", worst(em, rm, tm))
    report(f"bn_finalize {R.FIN_CASES[i]} running_var", worst(ev, rv, tv))
    if c["C"] >= 3:                                                           # the clamp channel
        assert bool((f["raw"][:, -1] < 0).all()) and bool((f["var"][:, -1] == 0).all())
        assert exact(e["istd"][:, -1], torch.full((c["groups"],), 1.0 / np.sqrt(R.EPS_BN)).float())


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.FWD_CASES)))
def test_forward_bounds_hold_for_the_emulation(i, half):
    C, M, groups, kind, slope, nomean = R.FWD_CASES[i]
    for with_r in (False, True):
        c = R.fwd_case(C, M, groups, kind, slope, nomean, half, None, with_r)
        got = R.emu_fwd(c["Z"], c["prm"], slope, groups, None, c["R"], half, nomean)
        report(f"bn_act{'_add' if with_r else ''}_fwd {R.FWD_CASES[i]}", worst(got, c["ref"], c["tol"]))
        if c["bit_exact"]:
            assert exact(got, c["ref"].half() if half else c["ref"].float())
        print(f"  moved away from zero: {c['moved']}")
        if kind != "exact" and not nomean:
            assert R.margin(c["Z"], c["prm"], groups) > 1.0


@pytest.mark.parametrize("i", range(len(R.DROP_CASES)))
def test_dropout_conditions_and_bounds(i):
    C, img, groups, kind, mode, p, salt = R.DROP_CASES[i]
    drop = R.drop_of(R.DROP_CASES[i])
    M = img * R.P_ROWS
    for half in (False, True):
        c = R.fwd_case(C, M, groups, kind, 0.25, False, half, drop)
        got = R.emu_fwd(c["Z"], c["prm"], 0.25, groups, drop, None, half)
        report(f"dropout forward {R.DROP_CASES[i]}", worst(got, c["ref"], c["tol"]))
        # no kept activation is 0 (exact kind: beta shifted by an odd multiple of 2^-6), so 'zeroed' and 'dropped' coincide
        y, _, _ = R.preact(c["Z"], c["prm"], groups)
        assert bool((y != 0).all()) and bool(((c["ref"] == 0) == ~c["keep"]).all())
        assert exact(got.float() == 0, ~c["keep"])
        frac = float((~c["keep"]).double().mean())
        assert 0.0 < frac < 1.0
        b = R.bwd_case(C, M, groups, kind, 0.25, False, half, drop)
        e = R.emu_bwd(b["dA"], b["Z"], b["prm"], 0.25, groups, drop, half)
        report(f"dropout backward {R.DROP_CASES[i]}", worst(e["dz"], b["dz"], b["tz"]))
    if mode == 2:                                                             # one decision per (image, channel)
        k = c["keep"].view(groups * img, R.P_ROWS, C)
        assert bool((k == k[:, :1]).all())


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.FWD_CASES)))
def test_backward_bounds_hold_for_the_emulation(i, half):
    C, M, groups, kind, slope, nomean = R.FWD_CASES[i]
    c = R.bwd_case(C, M, groups, kind, slope, nomean, half)
    if nomean:
        y = c["Z"]
        got = torch.where(y >= 0, c["dA"], c["dA"] * torch.tensor(slope))
        report(f"bn_act_bwd {R.FWD_CASES[i]} activation only", worst(got.half() if half else got, c["dz"], c["tz"]))
        return
    e = R.emu_bwd(c["dA"], c["Z"], c["prm"], slope, groups, None, half)
    for k, t in (("slab_s", "tslab_s"), ("slab_q", "tslab_q"), ("sums", "tsums"), ("dgamma", "tg"), ("dbeta", "tb"), ("dz", "tz")):
        report(f"bn_act_bwd {R.FWD_CASES[i]} {k}", worst(e[k], c[k], c[t]))
    if kind == "exact" and slope != 0.01:
        assert R.bwd_quanta(c) < 2 ** 24
        assert exact(e["slab_s"], c["slab_s"].float()) and exact(e["slab_q"], c["slab_q"].float())
    if kind != "exact":
        assert R.margin(c["Z"], c["prm"], groups) > 1.0


@pytest.mark.parametrize("i", range(len(R.GN_CASES)))
def test_groupnorm_bounds_hold_for_the_emulation(i):
    C, cpg, N, V = R.GN_CASES[i]
    g = R.gen(41, i)
    npg = R.chan_blocks(V)
    s, q = R.fin_slabs(g, C, N, npg, V)
    q = q + 1.0                                                               # no clamp channel here: the clamp is bn_finalize's test
    f = R.gn_finalize_ref(s, q, C, cpg, N, V)
    e = R.emu_gn_finalize(s, q, C, cpg, N, V)
    report(f"gn_finalize {R.GN_CASES[i]} mean", worst(e["m"], f["m"], f["tm"]))
    report(f"gn_finalize {R.GN_CASES[i]} istd", worst(e["istd"], f["istd"], f["ti"]))
    sets = f["m"].view(N, C // cpg, cpg)
    assert bool((sets == sets[:, :, :1]).all())
    c = R.bwd_case(C, V, N, "wide", 0.01, False, False, None, cpg)
    e = R.emu_bwd(c["dA"], c["Z"], c["prm"], 0.01, N, None, False, cpg)
    for k, t in (("sums", "tsums"), ("dgamma", "tg"), ("dbeta", "tb"), ("dz", "tz")):
        report(f"gn_act_bwd {R.GN_CASES[i]} {k}", worst(e[k], c[k], c[t]))


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("kind", ("wide", "offset"))
def test_chain_bounds_hold_for_the_emulation(kind, half):
    C, M, groups, slope = R.CHAIN_C, R.CHAIN_M, R.CHAIN_G, 0.01
    X, dA, ga, be, moved = R.chain_inputs(5, C, M, groups, kind, slope, half)
    c = R.chain_ref(X, dA, ga, be, slope, groups, 0, half)
    s, q = R.emu_slabs(X.numpy(), (X * X).numpy(), groups, C)
    e = R.emu_finalize(R.stats_layout(s), R.stats_layout(q), C, groups, M)
    f = c["fin"]
    live = slice(0, C - 1) if kind == "offset" else slice(0, C)
    print(f"chain {kind}: moved {moved}, conditioning E[x^2] / (var + eps) {c['cond_live']:.3g}")
    report(f"chain {kind} mean", worst(e["m"], f["m"], f["tm"]))
    report(f"chain {kind} istd", worst(e["istd"], f["istd"], f["ti"]))
    prm = dict(mu=e["m"], istd=e["istd"], ga=ga, be=be)
    a = R.emu_fwd(X, prm, slope, groups, None, None, half)
    report(f"chain {kind} forward", worst(a, c["a"], c["ta"]))
    b = R.emu_bwd(dA, X, prm, slope, groups, None, half)
    report(f"chain {kind} dz", worst(b["dz"], c["dz"], c["tz"]))
    report(f"chain {kind} dgamma", worst(b["dgamma"], c["dgamma"], c["tg"]))
    report(f"chain {kind} dbeta", worst(b["dbeta"], c["dbeta"], c["tb"]))
    prm64 = dict(mu=f["m"], istd=f["istd"], ga=ga, be=be)
    assert R.margin(X[:, live], {k: (v[..., live]) for k, v in prm64.items()}, groups, c["ey"][:, live]) > 1.0
    if kind == "offset":                                                      # the constant channel: variance exactly 0 through the clamp
        assert bool((e["istd"][:, -1] == torch.tensor(1.0 / np.sqrt(R.EPS_BN)).float()).all()) and bool((e["m"][:, -1] == 1.5).all())
        lb = be[-1] if be[-1] >= 0 else be[-1] * torch.tensor(slope)
        want = lb.half() if half else lb
        assert bool((a[:, -1] == want).all())


@pytest.mark.parametrize("i", [k for k in range(len(R.GN_CASES)) if R.GN_CASES[k][3] * R.GN_CASES[k][1] > 1])
def test_groupnorm_chain_bounds_hold_for_the_emulation(i):
    C, cpg, N, V = R.GN_CASES[i]
    slope = 0.01
    X, dA, ga, be, moved = R.chain_inputs(7, C, V, N, "wide", slope, False, cpg)
    c = R.chain_ref(X, dA, ga, be, slope, N, cpg)
    s, q = R.emu_slabs(X.numpy(), (X * X).numpy(), N, C)
    e = R.emu_gn_finalize(R.stats_layout(s), R.stats_layout(q), C, cpg, N, V)
    f = c["fin"]
    print(f"gn chain {R.GN_CASES[i]}: moved {moved}, conditioning {c['cond_live']:.3g}")
    report("gn chain mean", worst(e["m"], f["m"], f["tm"]))
    report("gn chain istd", worst(e["istd"], f["istd"], f["ti"]))
    prm = dict(mu=e["m"], istd=e["istd"], ga=ga, be=be)
    report("gn chain forward", worst(R.emu_fwd(X, prm, slope, N), c["a"], c["ta"]))
    b = R.emu_bwd(dA, X, prm, slope, N, None, False, cpg)
    report("gn chain dz", worst(b["dz"], c["dz"], c["tz"]))
    report("gn chain dgamma", worst(b["dgamma"], c["dgamma"], c["tg"]))
    report("gn chain dbeta", worst(b["dbeta"], c["dbeta"], c["tb"]))
    assert all(bool(torch.isfinite(c[k]).all()) for k in ("ta", "tz", "tg", "tb"))
    prm64 = dict(mu=f["m"], istd=f["istd"], ga=ga, be=be)
    assert R.margin(X, prm64, N, c["ey"]) > 1.0


# ---- conditions ---------------------------------------------------------------------------------------------------------------------
def test_block_geometry_matches_the_library():
    import arco_amd._lib as L
    L.load()
    Ms = sorted({c[1] for c in R.STATS_CASES} | {R.STATS_BIG[1], R.FWD_BIG_M, R.BWD_BIG_M, 1025, 7, 33, 16, 8192, 8208, 512 * 2048, 512 * 2048 + 1}
                | {8 * g[0] * g[1] * g[2] * g[3] for g in R.D2S_GRIDS})
    for M in Ms:
        assert L.query("arco_chan_stats_blocks", M) == R.chan_blocks(M), M
    g = R.geometry(8193, 4)
    assert (g["nblk"], g["rpb"], g["empty"]) == (512, 17, 30)
    g = R.geometry(R.STATS_BIG[1], 4)
    assert (g["nblk"], g["rpb"]) == (2048, 513)
    assert R.geometry(R.BWD_BIG_M, 4)["nblk"] == 2048 and -(-R.BWD_BIG_M // 512) > 2048          # crosses the 2048-slab cap
    assert R.slab_ranges(5, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)]


def test_exact_kind_quantum_budget():
    for C, M, groups, kind, pad, off in R.STATS_CASES + [R.STATS_BIG]:
        assert R.quantum_budget(M, C) < 2 ** 24, (C, M)
    x = R.values(R.gen(1), 4096, 8, "exact")
    k = x * 8
    assert bool((k == k.round()).all()) and float(k.abs().max()) == 32 and 0.15 < float((x == 0).float().mean()) < 0.3
    w = R.values(R.gen(1), 4096, 8, "wide")
    nz = w[w != 0].abs()
    assert float(nz.max() / nz.min()) > 5e5 and bool((w < 0).any()) and 0.15 < float((w == 0).float().mean()) < 0.25
    h = R.values(R.gen(1), 4096, 8, "wide", True)
    assert exact(h.half().float(), h)
    o = R.values(R.gen(1), 4096, 8, "offset")
    assert bool((o[:, -1] == 1.5).all()) and abs(float(o[:, 0].mean()) - 100) < 0.1 and abs(float(o[:, 0].std()) - 1) < 0.1
    p = R.params(R.gen(2), 3, 16, "exact")
    y = (x[:48].view(3, 16, 8)[..., :1] - p["mu"][:, None, :1])                # fp32 throughout: exact means equal to float64
    assert exact((x.view(-1, 1) - p["mu"][0, 0]).double(), x.view(-1, 1).double() - p["mu"][0, 0].double()) and y.dtype == torch.float32


def test_large_grids_exceed_the_grid_cap_by_the_stated_factor():
    # forward: work items = M * C / 4 (fp32, C = 4) or M * C / 8 (f16 eight-channel path, C = 8) = M
    assert R.FWD_BIG_M == 4 * R.GRID_CAP + 3 and R.FWD_BIG_M * 4 // 4 > 4 * R.GRID_CAP and R.FWD_BIG_M * 8 // 8 > 4 * R.GRID_CAP
    assert R.BWD_BIG_M == 2 * R.GRID_CAP + 3 and R.BWD_BIG_M > 2 * R.GRID_CAP
    # rstride = 4096 * 256 / q = GRID_CAP rows: rows u = 1 .. 3 (u = 1) exist, and the last 3 rows need a second trip
    assert R.FWD_BIG_M - 4 * R.GRID_CAP == 3 and R.BWD_BIG_M - 2 * R.GRID_CAP == 3
    assert R.FWD_BIG_M < 2 ** 24 and R.BWD_BIG_M < 2 ** 24                     # (float)M is exact
    assert R.FWD_BIG_M * 4 * 4 * 2 < 300e6 and R.BWD_BIG_M * 4 * 4 * 3 < 300e6 and R.FWD_BIG_M * 8 * 2 * 2 < 300e6


def test_case_tables_cover_the_listed_edges():
    assert {c[0] for c in R.STATS_CASES} == set(R.STATS_C) and {c[1] for c in R.STATS_CASES} == set(R.STATS_M)
    assert {(c[2], c[3]) for c in R.STATS_CASES} == {(g, k) for g in (1, 2, 3) for k in R.KINDS}
    assert any(c[5] for c in R.STATS_CASES) and any(c[4] and not c[5] for c in R.STATS_CASES)
    paths = {(R.geometry(c[1], c[0])["shuffle"], 256 % (c[0] // 4) == 0) for c in R.STATS_CASES}
    assert paths == {(True, True), (False, True), (False, False)}
    assert {c[0] for c in R.FIN_CASES} == set(R.FIN_NPG) and {c[1] for c in R.FIN_CASES} == set(R.FIN_C)
    assert {c[3] for c in R.FIN_CASES} == set(R.FIN_CNT) and {(c[2], c[4]) for c in R.FIN_CASES} >= {(3, m) for m in R.FIN_MODES}
    assert {R.defer_from(c[4], c[2]) for c in R.FIN_CASES if c[2] == 3} == {None, 0, 1, 2}
    assert {c[0] for c in R.FWD_CASES} == set(R.FWD_C) and {c[1] for c in R.FWD_CASES} >= set(R.FWD_M)
    assert {c[2] for c in R.FWD_CASES} == {1, 2, 3} and {c[4] for c in R.FWD_CASES} == set(R.SLOPES) and any(c[5] for c in R.FWD_CASES)
    assert {256 % (c[0] // 4) == 0 for c in R.FWD_CASES} == {True, False}
    assert {c[0] % 8 == 0 and 256 % (c[0] // 8) == 0 for c in R.FWD_CASES} == {True, False}
    assert {(c[2], c[4], c[5], c[6] is None) for c in R.DROP_CASES} == {(g, m, p, s) for g in (1, 2) for m in (1, 2) for p in (0.1, 0.5)
                                                                        for s in (True, False)}
    assert {(c[0], c[1]) for c in R.GN_CASES} == set(R.GN_SETS) and {c[2] for c in R.GN_CASES} == {1, 2, 3}
    assert {c[3] for c in R.GN_CASES} == {1, 33, 1025}
    assert {c[0] for c in R.D2S_CASES} == set(R.D2S_GRIDS) and {c[1] for c in R.D2S_CASES} == {1, 2}
    assert {(c[0], c[1]) for c in R.POOL_CASES} == {(1, 1), (4, 1), (4, 2)} and {c[4] for c in R.POOL_CASES} == {4, 20}


def test_dropout_restatement():
    assert R.drop_thr(0.5) == 32768 and R.drop_thr(0.1) == 6554 and R.drop_thr(0.0) == 0
    assert int(R.pcg(np.array([0], dtype=np.uint32))[0]) == 129708002              # pcg_hash(0), worked by hand from common.h
    e = np.arange(1 << 16, dtype=np.uint64)
    for p in (0.1, 0.5):
        frac = 1.0 - R.keep_mask(R.DROP_SEED, e, p).mean()
        assert abs(frac - p) < 0.01
    assert R.keep_mask(R.DROP_SEED, e, 0.0).all()
    assert (R.keep_mask(R.drop_seed(R.DROP_SEED, 5), e, 0.5) != R.keep_mask(R.DROP_SEED, e, 0.5)).any()
    assert R.drop_seed(7, None) == 7 and R.drop_seed(0, 1) == 0x9E3779B97F4A7C15 and R.drop_seed(0, 2) == (2 * 0x9E3779B97F4A7C15) % 2 ** 64
    big = np.array([2 ** 33 + 5, 2 ** 33 + 4], dtype=np.uint64)                      # the high word of e >> 1 enters the hash
    assert R.keep_mask(1, big, 0.5).shape == (2,)


# ---- planted errors -----------------------------------------------------------------------------------------------------------------
def test_helpers_reject_planted_errors():
    # a group's slab range shifted by one slab
    c = R.stats_case(R.STATS_CASES.index(next(k for k in R.STATS_CASES if k[1] == 513 and k[3] == "wide")), False)
    bad = R.stats_ref(c["X"], c["groups"], c["C"], shift=1)
    assert worst(c["s"].float(), c["s"], c["ts"]) <= 1.0 and worst(bad["s"].float(), c["s"], c["ts"]) > 1e3
    ce = R.stats_case(R.STATS_CASES.index(next(k for k in R.STATS_CASES if k[1] == 8193 and k[3] == "exact")), False)
    assert not exact(R.stats_ref(ce["X"], ce["groups"], ce["C"], shift=1)["s"].float(), ce["s"].float())
    # biased in place of unbiased variance in the running update (count 2: a factor of two)
    i = next(k for k, f in enumerate(R.FIN_CASES) if f[3] == 2 and f[4] == "running")
    f = R.fin_case(i)
    rm, rv, tm, tv = R.running_ref(f["rm0"], f["rv0"], f["fin"], f["groups"])
    _, bv, _, _ = R.running_ref(f["rm0"], f["rv0"], f["fin"], f["groups"], biased=True)
    live = f["fin"]["var"].sum(0) > 0
    assert worst(rv.float(), rv, tv) <= 1.0 and worst(bv.float()[live], rv[live], tv[live]) > 1e3
    # the two deferred groups applied in swapped order
    g = R.gen(3)
    terms = R.values(g, 2 * 2, 300, "wide").view(2, 2, 300)
    rm0, rv0 = torch.randn(300, generator=g), torch.rand(300, generator=g)
    rm, rv, tm, tv = R.deferred_ref(rm0, rv0, terms, R.MOM)
    sm, sv, _, _ = R.deferred_ref(rm0, rv0, terms.flip(0), R.MOM)
    assert worst(rm, rm.double(), tm) <= 1.0 and worst(sm, rm.double(), tm) > 1e3 and worst(sv, rv.double(), tv) > 1e3
    # sum_dy and sum_dyx swapped
    C, M, groups, kind, slope, nomean = next(k for k in R.FWD_CASES if k[3] == "wide" and k[1] == 1025 and not k[5])
    b = R.bwd_case(C, M, groups, kind, slope, nomean)
    bad = R.bwd_ref(b["dA"], b["Z"], b["prm"], slope, groups, swap_sums=True)
    assert worst(bad["dz"].float(), b["dz"], b["tz"]) > 1e3 and worst(bad["sums"].float(), b["sums"], b["tsums"]) > 1e3
    # dropout element index without the group's row0
    dc = next(k for k in R.DROP_CASES if k[2] == 2 and k[4] == 1 and k[5] == 0.5)
    drop = R.drop_of(dc)
    rows = dc[1] * R.P_ROWS * 2
    good, wrong = R.drop_keep(drop, rows, dc[0], 2), R.drop_keep(drop, rows, dc[0], 2, with_row0=False)
    assert exact(good[:rows // 2], wrong[:rows // 2]) and not exact(good[rows // 2:], wrong[rows // 2:])
    dc2 = next(k for k in R.DROP_CASES if k[2] == 2 and k[4] == 2 and k[5] == 0.5)
    assert not exact(R.drop_keep(R.drop_of(dc2), rows, dc2[0], 2), R.drop_keep(R.drop_of(dc2), rows, dc2[0], 2, with_row0=False))
    # one tap of the depth-to-space map permuted
    grid = R.D2S_GRIDS[1]
    Y = R.values(R.gen(4), 8 * 2 * 1 * 2 * 3, 4, "exact")
    A = R.d2s(Y, grid, 4)
    assert exact(R.s2d(A, grid, 4), Y) and not exact(R.d2s(Y, grid, 4, taps=(0, 2, 1, 3, 4, 5, 6, 7)), A)
    nv, x2, y2, z2 = grid
    A5 = A.view(nv, 2 * x2, 2 * y2, 2 * z2, 4)
    Y6 = Y.view(nv, x2, y2, z2, 8, 4)
    for tap in range(8):                                                      # the reshape / permute form against the index formula
        dx, dy, dz = tap >> 2, (tap >> 1) & 1, tap & 1
        assert exact(A5[1, dx::2, dy::2, dz::2], Y6[1, :, :, :, tap])
    # gamma left out of the GroupNorm set sums
    C, cpg, N, V = next(k for k in R.GN_CASES if k[1] == 4 and k[3] == 33)
    gb = R.bwd_case(C, V, N, "wide", 0.01, False, False, None, cpg)
    bad = R.bwd_ref(gb["dA"], gb["Z"], gb["prm"], 0.01, N, cpg=cpg, gn_gamma=False)
    assert worst(bad["sums"].float(), gb["sums"], gb["tsums"]) > 1e3 and worst(bad["dz"].float(), gb["dz"], gb["tz"]) > 1e3
    # one element one ulp beside a bit-exact result; a NaN
    fc = R.fwd_case(8, 7, 2, "exact", 0.25, False)
    good = fc["ref"].float()
    one = good.clone()
    one[3, 5] = torch.nextafter(one[3, 5], torch.tensor(100.0))
    assert exact(good, fc["ref"].float()) and not exact(one, fc["ref"].float())
    one[0, 0] = float("nan")
    assert worst(one, fc["ref"], fc["tol"] + 1.0) == float("inf")


# ---- argument checks (host side) ----------------------------------------------------------------------------------------------------
def test_descriptor_layout():
    import arco_amd._lib as L
    L.load()
    assert struct.calcsize(R.DEFER_FMT) == L.query("arco_bn_defer_desc_bytes") == 40


def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced.  Every list below is a VALID call with one argument spoilt at a time; the valid call itself is never
    made."""
    import arco_amd._lib as L
    L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())

    def spoil(name, ok, cases):
        for pos, val in cases:
            args = list(ok)
            args[pos] = val
            assert L.query(name, *args, None) == -1, (name, pos, val)

    # chan_stats(_h): X, ldx, M, C, ssum, ssq, groups
    for name in ("arco_chan_stats", "arco_chan_stats_h"):
        spoil(name, [p, 8, 6, 8, p, p, 2], [(3, 6), (3, 0), (3, 1028), (1, 6), (2, 7), (6, 4)])
    # bn_finalize: ssum, ssq, nblk, C, count, eps, momentum, mean, istd, rm, rv, nbt, groups, defer_from, deferred
    ok = [p, p, 6, 3, 12, 1e-5, 0.1, p, p, p, p, p, 2, 1, p]
    spoil("arco_bn_finalize", ok, [(2, 7), (2, 0), (3, 0), (4, 13), (4, 0), (13, 2), (13, -1), (12, 4)])
    assert L.query("arco_bn_apply_deferred", None, 0, None) == 0 and L.query("arco_bn_apply_deferred", None, 1, None) == -1
    # bn_act_fwd(_h): Z, ldz, M, C, mean, istd, gamma, beta, slope, drop_mode, p, seed, P, A, lda, seed_dev, groups
    ok = [p, 8, 6, 8, p, p, p, p, 0.01, 1, 0.5, 1, 1, p, 8, None, 2]
    for name in ("arco_bn_act_fwd", "arco_bn_act_fwd_h"):
        spoil(name, ok, [(3, 6), (3, 0), (1, 6), (14, 6), (2, 7), (10, 1.0), (10, 1.5), (16, 4)])
    # bn_act_add_fwd(_h): Z, ldz, M, C, mean, istd, gamma, beta, slope, R, ldr, A, lda, groups
    ok = [p, 8, 6, 8, p, p, p, p, 0.01, p, 8, p, 8, 2]
    for name in ("arco_bn_act_add_fwd", "arco_bn_act_add_fwd_h"):
        spoil(name, ok, [(9, None), (3, 6), (1, 6), (10, 6), (12, 6), (2, 7)])
    # bn_act_d2s_fwd(_h): Y, M8, C, mean, istd, gamma, beta, slope, R, ldr, A, lda, X2, Y2, Z2, groups
    ok = [p, 96, 8, p, p, p, p, 0.01, p, 8, p, 8, 1, 2, 3, 2]
    for name in ("arco_bn_act_d2s_fwd", "arco_bn_act_d2s_fwd_h"):
        spoil(name, ok, [(1, 88), (1, 104), (12, 0), (13, 0), (14, 0), (2, 6), (9, 6), (11, 6), (15, 5)])
    # bn_act_bwd(_h): dA, ldd, Z, ldz, M, C, mean, istd, gamma, beta, slope, drop_mode, p, seed, P, ws, dgamma, dbeta, accumulate, dZ, ldo,
    # seed_dev, groups
    ok = [p, 8, p, 8, 6, 8, p, p, p, p, 0.01, 0, 0.0, 0, 1, p, p, p, 0, p, 8, None, 2]
    for name in ("arco_bn_act_bwd", "arco_bn_act_bwd_h"):
        spoil(name, ok, [(5, 6), (5, 0), (5, 1028), (1, 6), (3, 6), (20, 6), (4, 7), (22, 4)])
    # bn_act_d2s_bwd(_h): dA, ldd, Y, M8, C, mean, istd, gamma, beta, slope, ws, dgamma, dbeta, accumulate, dY, X2, Y2, Z2, groups
    ok = [p, 8, p, 96, 8, p, p, p, p, 0.01, p, p, p, 0, p, 1, 2, 3, 2]
    for name in ("arco_bn_act_d2s_bwd", "arco_bn_act_d2s_bwd_h"):
        spoil(name, ok, [(3, 88), (15, 0), (16, 0), (17, 0), (5, None), (4, 6), (4, 1028), (1, 6), (18, 5)])
    # gn_finalize: ssum, ssq, nblk, C, cpg, N, count, eps, mean, istd
    ok = [p, p, 6, 12, 3, 2, 5, 1e-5, p, p]
    spoil("arco_gn_finalize", ok, [(0, None), (1, None), (8, None), (9, None), (4, 5), (4, 0), (4, 257), (3, 0), (5, 0), (2, 7), (6, 0)])
    # gn_act_bwd: dA, ldd, Z, ldz, M, C, mean, istd, gamma, beta, slope, ws, dgamma, dbeta, accumulate, dZ, ldo, N, cpg
    ok = [p, 12, p, 12, 6, 12, p, p, p, p, 0.01, p, p, p, 0, p, 12, 2, 3]
    spoil("arco_gn_act_bwd", ok, [(6, None), (7, None), (8, None), (9, None), (18, 0), (18, 5), (5, 6), (5, 1028), (1, 6), (3, 6), (16, 6), (4, 7)])
    # bn_act_pool_fwd: Z, ldz, NB, H, W, C, mean, istd, gamma, beta, slope, A, lda, P, ldp, groups
    ok = [p, 8, 4, 4, 6, 8, p, p, p, p, 0.01, p, 8, p, 8, 2]
    spoil("arco_bn_act_pool_fwd", ok, [(0, None), (6, None), (7, None), (8, None), (9, None), (11, None), (13, None), (5, 6), (5, 0), (1, 6),
                                       (12, 6), (14, 6), (3, 3), (4, 5), (15, 3)])
