"""CPU companion of tests/test_hconv_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * every case reaches the route it names: arco_conv_config_mma(..., 4) / arco_conv_mblocks_mma(..., 4) are host-only (with no device the
    CU count falls back to 256, the MI355X figure); the two streaming 1x1 kernels, which no query describes, have the conditions of
    hconv1x1_stream_dispatch restated here, and each near-miss case misses exactly one of them; the unit arithmetic of
    launch_hconv_rw and the tile count of the persistent hconv_fc_kernel are restated for the cases with more work than workgroups;
  * the input conditions of every case and kind: the 2^24 budget per output channel's quantum, f16-representability of every operand,
    the spacing of the impulses, the ties and the subnormal outputs really present in the fixed kind, |ref| < 65504, S > 0 wherever the
    reference is not zero, and the float64 reference exactly representable in fp32 for the exact kinds;
  * the wide kind emulated on the CPU (exact products, fp32 accumulation in one fixed order, one rounding to f16) stays inside the
    same bounds; the ratios are printed and recorded in the GPU file's docstring;
  * each comparison helper rejects each planted error: one tap mirrored, one border column not zero-padded, the two taps that share one
    32-k MFMA step exchanged, the output truncated instead of rounded to nearest even, the output rounded twice, a subnormal output
    flushed to zero, statistics taken from the unrounded fp32 values, one slab counted in the wrong group, the bias added twice on one tile;
  * the host-side rejections of mma 4 return before anything is launched and note no route."""
import ctypes

import pytest
import torch

import hconv_kernel_refs as R
import test_conv_kernels_cpu as TC
from conv_kernel_refs import conv64, impulse_positions, representable, select_passes, stat_totals
from loss_kernel_refs import worst

EMU = ["h2-64x16", "h2-64x32", "h2-32x32", "v128x16", "v64x32", "v32x32", "f128x16", "f64x32", "f32x32", "g256x16", "g256x16-n2",
       "g128x32", "g32x64", "rw-plane", "fc-7-32-32", "image3-plane", "image3"]
EMU_ROWS = ["nout-k8-n4", "nout-k16-n2", "nout-k32-n4", "nin-k2-n16", "nin-k3-n32"]           # the streams: the first 4096 rows


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def names(cases):
    return [c["name"] for c in cases]


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
def stream_route(c):
    """hconv1x1_stream_dispatch restated: the id of the streaming kernel a launch of this case takes, or None (the buffers of the GPU
    file start on 16-byte boundaries: an operand is off one by its column offset, the output also by out_shift f16 elements)"""
    K, N, M = c["k"], c["n"], c["M"]
    if c["taps"] != 1 or c["stats"] or M < 65536:
        return None
    if 1 <= N <= 4 and K in (8, 16, 32) and c["ld_in"] % 8 == 0 and (2 * c["in_off"]) % 16 == 0:
        return 1800000 + K * 1000 + 4
    if 1 <= K <= 4 and N in (8, 16, 32) and c["ld_out"] % 8 == 0 and (2 * c["out_shift"]) % 16 == 0:
        return 1900000
    return None


def query(L, c, groups=None):
    args = (c["taps"], c["nv"] * c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_in"])
    prev = L.query("arco_conv3d_fl_set", c["fl"]) if c["fl"] is not None else None
    try:
        return (L.query("arco_conv_config_mma", *args, 4),
                L.query("arco_conv_mblocks_mma", *args, max(1, c["stats"] if groups is None else groups), 4))
    finally:
        if prev is not None:
            L.query("arco_conv3d_fl_set", prev)


@pytest.mark.parametrize("c", R.CASES + R.DGRAD, ids=names(R.CASES + R.DGRAD))
def test_case_reaches_its_route(L, c):
    got, nmb = query(L, c)
    assert nmb >= max(1, c["stats"])
    if c["fam"] not in ("nout", "nin"):
        assert stream_route(c) is None                                                             # nothing else slips onto a stream
    if not c["launch_only"]:
        assert got == c["route"], (c["name"], got)
        return
    if c["fam"] in ("nout", "nin"):
        assert stream_route(c) == c["route"], c["name"]
        assert got == (1256016 if R.ceil_to(c["n"], 16) <= 16 else 1128032)                        # what the query, blind to the streams, says
    else:                                                                                          # g64x64-groups: the query takes no group count
        tiles64 = -(-c["M"] // 64) * -(-R.ceil_to(c["n"], 16) // 64)
        assert c["stats"] == 2 and tiles64 < 192 and got == 1032064 and c["route"] == 1064064
        assert c["M"] * R.ceil_to(c["n"], 16) <= 4096 * 1024 and R.ceil_to(c["n"], 16) > 32
        assert nmb == 2 * -(-(c["M"] // 2) // 64) and query(L, c, 1)[1] == -(-c["M"] // 32)        # 64-row slabs per group / 32-row slabs


def test_spatial_tiles_follow_the_256_workgroup_threshold():
    """every hconv_kernel<9,..> case sits where the restated tile choice (HCONV_WANT_BLOCKS = 256) puts it"""
    assert R.WANT == 256
    for c in R.H2D + R.H3D + [c for c in R.DGRAD if c["fam"] in ("h2d", "h3d")]:
        assert R.spatial_tile(c) == c["route"], c["name"]


def test_near_misses_miss_exactly_one_condition():
    fix = {"nout-miss-m": dict(h=257), "nout-miss-ld": dict(in_pad=8), "nin-miss-shift": dict(out_shift=0), "nin-miss-m": dict(h=257)}
    want = {"nout-miss-m": 1816004, "nout-miss-ld": 1808004, "nin-miss-shift": 1900000, "nin-miss-m": 1900000}
    assert sorted(fix) == sorted(names(R.NEAR))
    for c in R.NEAR:
        assert stream_route(c) is None
        o = {k: c[k] for k in ("in_pad", "in_off", "out_pad", "out_shift", "bias", "stats")}
        o.update({k: v for k, v in fix[c["name"]].items() if k in o})
        h = fix[c["name"]].get("h", c["h"])
        mended = R.C("mended", 1, c["nv"], c["d3"], h, c["w"], c["k"], c["n"], 0, c["fam"], **o)
        assert stream_route(mended) == want[c["name"]], c["name"]
    assert R.by_name("nout-miss-m")["M"] == 65535 == R.by_name("nin-miss-m")["M"]


def test_persistent_kernels_get_more_work_than_workgroups(L):
    S, nseg, units, slots = R.rw_units(R.by_name("rw-rounds"))
    assert (S, nseg, slots) == (2, 17, 1024) and slots < units < 2 * slots                          # 1088 units: a ragged second round
    S, nseg, _, _ = R.rw_units(R.by_name("rw-odd"))
    assert S == 2 and R.by_name("rw-odd")["d3"] % 2 == 1 and nseg == 3                              # the last unit of a column holds one plane
    assert R.rw_units(R.by_name("rw-plane"))[:2] == (1, 1)
    c = R.by_name("fc-7-32-32-rounds")
    a_t, bn = (c["route"] - 9260000) // 1000, c["route"] % 1000
    tiles = c["nv"] * c["d3"] * -(-(c["h"] * (c["w"] + 2)) // (64 * a_t)) * (c["n"] // bn)
    assert 256 < tiles < 512 and query(L, c)[1] == 4 * tiles // (c["n"] // bn)
    for c in R.CASES:                                                                               # hconv_rw_eligible, restated
        if c["fam"] == "rw":
            assert c["k"] == 16 == c["n"] and c["h"] % 8 == 0 and c["w"] % 16 == 0 and c["ld_in"] % 8 == 0 and c["ld_out"] % 4 == 0


def test_every_family_has_every_edge():
    """in_pad and in_off, out_pad with ld_out % 4 == 0 and != 0, bias and none, statistics with 1 and 2 groups, N no multiple of 4 and
    of 16, a plane smaller than a tile - in every family, except where the kernel's own conditions rule an edge out (stated per line)"""
    def small(c):                                                                                   # fewer positions than one tile holds
        if c["fam"] == "fc":
            return c["h"] * (c["w"] + 2) < 64 * ((c["route"] - 9260000) // 1000)
        return (c["h"] < 16 and c["w"] < 16) if c["fam"] == "image" else c["h"] * c["w"] < c["route"] % 1000000 % 500000 // 1000
    for fam in R.FAMS:
        cs = [c for c in R.CASES if c["fam"] == fam]
        assert cs, fam
        assert any(c["in_off"] > 0 and c["in_pad"] > 0 for c in cs) or fam == "image"               # image: one fp32 channel, ld_in = 1
        assert any(c["out_pad"] > 0 and c["ld_out"] % 4 == 0 for c in cs)
        assert any(c["bias"] for c in cs) and any(not c["bias"] for c in cs)
        if fam not in ("rw", "fc", "image", "nin"):                                                 # these need ld_out % 4 == 0 (nin: % 8)
            assert any(c["out_pad"] > 0 and c["ld_out"] % 4 != 0 for c in cs), fam
        if fam not in ("nout", "nin"):                                                              # the streams take no statistics
            assert {1, 2} <= {c["stats"] for c in cs}, fam
        if fam not in ("rw", "fc", "image", "nin"):                                                 # N = 16 / N % 32 == 0 / N % 4 == 0 / N in {8, 16, 32}
            assert any(c["n"] % 4 for c in cs), fam
        if fam not in ("rw", "fc"):
            assert any(c["n"] % 16 for c in cs), fam
        if fam in ("h2d", "h3d", "fc", "image"):                                                    # (rw: H % 8 == 0 and W % 16 == 0 - whole tiles only)
            assert any(small(c) for c in cs), fam
        if fam == "h1x1":
            assert any(c["M"] < 256 for c in cs) and any(c["stats"] == 2 and (c["M"] // 2) % 128 for c in cs)     # m_lim of the grouped GEMM form
    both = lambda f: {bool(c["k"] % 8 == 0 and c["ld_in"] % 8 == 0) for c in R.CASES if c["fam"] == f}
    assert both("h2d") == {True, False} == both("h1x1")                                             # 16-byte pieces and element-wise staging
    assert any(c["d3"] == 1 and c["taps"] == 27 for c in R.CASES if c["fam"] in ("h3d", "rw", "image"))           # volumes of one plane


def test_every_route_is_covered_and_every_case_runs_four_kinds():
    have = {(c["taps"], c["route"]) for c in R.CASES}
    for r in R.ROUTES:
        assert r in have, r
    fc = {c["route"] for c in R.CASES if c["fam"] == "fc"}
    assert any(r % 1000 == 64 for r in fc) and any(r % 1000 == 32 for r in fc)
    assert {c["k"] for c in R.FC} >= {32, 64, 128} and {c["n"] for c in R.FC} >= {32, 64, 128} and {c["w"] for c in R.FC} >= {7, 12, 24, 45}
    assert any(c["n"] == 32 and c["w"] % 16 for c in R.FC)
    assert {(c["route"], c["n"]) for c in R.NEAR} >= {(1256016, 2), (1256016, 16), (1128032, 32)}
    assert sorted({c["fam"] for c in R.DGRAD}) == sorted(set(R.FAMS) - {"image"})
    assert all(c["kinds"] == R.ALL for c in R.CASES)                                               # no case carries fewer than four kinds
    assert [c["name"] for c in R.CASES if c["grouped"]] == ["g64x64-groups"]


# ---- input conditions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=names(R.CASES))
def test_input_conditions(c):
    K, T, N = c["k"], c["taps"], c["n"]
    d = R.data(c, "fixed")
    assert R.f16_ok(d["x"]) and R.f16_ok(d["w"]) and representable(d["ref"]) and float(d["ref"].abs().max()) < R.MAXH
    assert float((d["S"] / d["q"]).max()) < 2 ** 24                                                # the budget, in each channel's own quantum
    m = d["ref"] / d["q"]
    assert bool((m == m.round()).all())
    fl = [R.flavour(n, N) for n in range(N)]
    ex = [n for n in range(N) if fl[n] == "exact"]
    if ex:
        assert float(m[:, ex].abs().max()) < 2 ** 11 and torch.equal(R.expected_h(d["ref"])[:, ex].double(), d["ref"][:, ex])    # the store is an identity
    sub = [n for n in range(N) if fl[n] == "sub"]
    if sub:
        r = d["ref"][:, sub]
        assert float(r.abs().max()) < R.SUBN and bool((r != 0).any())                              # outputs in the subnormal range
        assert bool(R.ties(r).any())                                                                # ... with ties among them
        assert not torch.equal(R.expected_h(r).double(), r)                                         # ... that the store really rounds
    if "tie" in fl:
        r = d["ref"][:, [n for n in range(N) if fl[n] == "tie"]]
        assert bool((R.ties(r) & (r.abs() >= R.SUBN)).any())                                        # ties in the normal range
    if "big" in fl and K >= 2:
        r = m[:, [n for n in range(N) if fl[n] == "big"]]
        assert float(r.abs().max()) >= 2 ** 20                                                      # more than 20 significant bits before rounding
    assert N == 1 or len(ex) == (N + 1) // 2
    if "impulse" in c["kinds"]:
        d = R.data(c, "impulse")
        rows = impulse_positions(c)
        assert R.f16_ok(d["w"]) and len(set(rows)) == len(rows) >= 1 and int((d["x"] != 0).sum()) == len(rows)
        hits = conv64((d["x"] != 0).double(), torch.ones_like(d["w"]).double(), c)
        assert float(hits.max()) <= 1.0 and representable(d["ref"])                                 # one product per output at most
        spanned = [] if T == 1 else [c["h"], c["w"]] + ([c["d3"]] if T == 27 else [])
        assert 0 in rows and (c["M"] - 1 in rows or T == 1 or min(spanned) < 5)
        nz = d["ref"] != 0
        assert bool(torch.isin(d["ref"][nz].float(), d["w"].flatten()).all())                       # every output is one weight
        a = d["ref"][nz].abs()
        assert bool((a < R.SUBN).any()) and bool((a == R.MAXH).any())                               # subnormal weights and 65504 reach the output
    if "select" in c["kinds"]:
        used = set()
        for p in range(select_passes(c)):
            d = R.data(c, "select", p)
            assert R.f16_ok(d["x"]) and bool(((d["w"] != 0).sum((1, 2)) == 1).all()) and representable(d["ref"])
            assert R.f16_ok(d["ref"].float()) and float(d["ref"].abs().max()) <= R.MAXH             # the product stays representable
            assert bool(((d["x"] != 0) & (d["x"].abs() < R.SUBN)).any())                            # subnormal activations
            used |= set(torch.nonzero(d["w"])[:, 2].tolist())
        assert used == set(range(T))                                                                # every tap used by some channel
    d = R.data(c, "wide")
    assert bool(((d["S"] > 0) | (d["ref"] == 0)).all()) and float(d["ref"].abs().max()) < R.MAXH
    assert float((d["x"] == 0).float().mean()) > 0.1
    if c["fam"] != "image":
        assert R.f16_ok(d["x"]) and R.f16_ok(d["w"])
        nzx = d["x"][d["x"] != 0].abs()
        assert float(nzx.min()) >= R.SUBN and (nzx.numel() < 1000 or float(nzx.max() / nzx.min()) > 1e4)      # four decades, all normal


STATS = [c for c in R.CASES if c["stats"]]


@pytest.mark.parametrize("c", STATS, ids=names(STATS))
def test_stats_kind_fits_the_budget_and_is_really_rounded(c):
    d = R.data(c, "stats")
    y = R.expected_h(d["ref"]).double()
    assert R.f16_ok(d["x"]) and R.f16_ok(d["w"])
    assert bool((y / R.SQ == (y / R.SQ).round()).all()) and float(y.abs().max()) > 0
    assert float((y ** 2).sum(0).max()) / R.SQ ** 2 < 2 ** 24 and float(y.abs().sum(0).max()) / R.SQ < 2 ** 24
    t1, t2 = stat_totals(c, y, c["stats"])
    u1, u2 = stat_totals(c, d["ref"], c["stats"])
    assert bool((t2 != u2).all()) and not torch.equal(t1, u1)                                       # rounded and unrounded statistics differ


@pytest.mark.parametrize("c", R.DGRAD, ids=names(R.DGRAD))
def test_data_gradient_reference_is_float64_autograd(c):
    f = R.data(c, "fixed", 0, True)
    assert torch.equal(R.dgrad_autograd(c, f), f["ref"]) and representable(f["ref"])
    d = R.data(c, "wide", 0, True)
    n, u64 = c["taps"] * c["k"], 2.0 ** -53
    assert worst(R.dgrad_autograd(c, d), d["ref"], 2 * n * u64 / (1 - n * u64) * d["S"]) <= 1.0


# ---- the emulation stays inside the bounds --------------------------------------------------------------------------------------------
def _head(c, d, rows):
    """the first `rows` rows of a 1x1 case as a case of its own (a GEMM's rows are independent)"""
    cc = dict(c, M=rows, h=1, w=rows, nv=1, d3=1)
    dd = dict(d, x=d["x"][:rows], ref=d["ref"][:rows], S=d["S"][:rows], sxw=d["sxw"][:rows])
    return cc, dd


@pytest.mark.parametrize("name", EMU + EMU_ROWS)
def test_bounds_hold_for_the_emulation(name):
    c = R.by_name(name)
    cut = (lambda d: _head(c, d, 4096)) if name in EMU_ROWS else (lambda d: (c, d))
    cc, d = cut(R.data(c, "wide"))
    assert R.held(f"emulated {name} [{c['fam']}]", R.emulate(cc, d), cc, d) <= 1.0
    for kind in ("fixed", "impulse", "select"):                                                    # the exact kinds are exact in ANY fp32 order
        cc, e = cut(R.data(c, kind))
        assert R.equal_h(R.emulate(cc, e), e["ref"]), kind


def test_families_of_the_emulation():
    assert {R.by_name(n)["fam"] for n in EMU + EMU_ROWS} == set(R.FAMS)


# ---- planted errors ------------------------------------------------------------------------------------------------------------------------
def _exact(c, d, x=None, w=None):
    y = conv64((d["x"] if x is None else x).double(), (d["w"] if w is None else w).double(), c)
    return y if d["bias"] is None else y + d["bias"].double()


def _got(c, d, x=None, w=None):
    return _exact(c, d, x, w).float().half()


def _ok(c, d):
    return (lambda g: R.equal_h(g, d["ref"])) if d["kind"] != "wide" else (lambda g: R.held("planted", g, c, d) <= 1.0)


@pytest.mark.parametrize("name", ["h2-64x32", "v64x32", "f64x32", "rw-plane", "fc-7-32-32"])
def test_helpers_reject_planted_geometry_errors(name):
    c = R.by_name(name)
    T, K = c["taps"], c["k"]
    for kind in c["kinds"]:
        d = R.data(c, kind)
        ok = _ok(c, d)
        assert ok(_got(c, d))                                                                       # the unplanted result passes
        n = 1
        # (1) one tap mirrored: taps dx = 0 and dx = 2 of one output channel exchanged
        w = d["w"].clone().view(c["n"], K, T // 3, 3)
        w[n] = w[n].flip(-1)
        if not torch.equal(_exact(c, d, w=w.view_as(d["w"])), _exact(c, d)):
            assert not ok(_got(c, d, w=w.view_as(d["w"]))), (kind, "mirrored")
        # (3) the two taps that share one 32-k MFMA step (taps 2 s and 2 s + 1) exchanged
        for s in range(T // 2):
            w = d["w"].clone()
            w[n, :, [2 * s, 2 * s + 1]] = w[n, :, [2 * s + 1, 2 * s]]
            if not torch.equal(_exact(c, d, w=w), _exact(c, d)):                                    # (the depth taps of a one-plane volume meet padding only)
                assert not ok(_got(c, d, w=w)), (kind, "pair", s)
    for kind in ("fixed", "wide"):
        d = R.data(c, kind)
        ok = _ok(c, d)
        # (2) one border column not zero-padded: the left neighbours of column 0 read the last column of the row above
        bad = TC._leaky(c, dict(d, res=None)).half()
        assert not torch.equal(bad, _got(c, d)) and not ok(bad), (kind, "leaky")
        # (9) the bias added twice on one tile
        if d["bias"] is not None:
            g = _got(c, d).float()
            g[:16] += d["bias"]
            assert not ok(g.half()), (kind, "bias")


@pytest.mark.parametrize("name", ["h2-64x32", "g128x32", "nout-k16-n2", "nin-k2-n16", "image3", "rw-plane", "fc-7-32-32"])
def test_helpers_reject_planted_rounding_errors(name):
    c = R.by_name(name)
    d = R.data(c, "fixed")
    exp = R.expected_h(d["ref"])
    assert R.equal_h(exp, d["ref"])
    # (4) truncated instead of rounded to nearest even: the ties alone catch it
    t = R.ties(d["ref"])
    cut = R.trunc_h(d["ref"])
    assert bool(t.any()) and bool((cut[t] != exp[t]).any()) and not R.equal_h(cut, d["ref"])
    assert bool((cut.double().abs() <= d["ref"].abs()).all())
    # (5) rounded twice: through bf16, and through 13 significant bits (a tie made by the first rounding goes the other way)
    assert not R.equal_h(R.bf16_then_h(d["ref"]), d["ref"])
    assert c["n"] < 6 or not R.equal_h(R.twice_h(d["ref"]), d["ref"])                              # (needs a tie or big channel: N >= 6)
    # (6) a subnormal output flushed to zero
    assert not R.equal_h(R.flush_h(d["ref"]), d["ref"])
    for kind in ("impulse", "select"):
        e = R.data(c, kind)
        assert R.equal_h(R.expected_h(e["ref"]), e["ref"]) and not R.equal_h(R.flush_h(e["ref"]), e["ref"]), kind
    # ... and the per-element bound of the wide kind rejects a truncating store as well
    dw = R.data(c, "wide")
    assert R.held("rounded", R.expected_h(dw["ref"].float().double()), c, dw) <= 1.0
    assert R.held("truncated", R.trunc_h(dw["ref"].float().double()), c, dw) > 1.0


@pytest.mark.parametrize("name", ["fc-7-32-32", "g64x64", "image3"])
def test_stats_helpers_reject_planted_errors(name):
    c = R.by_name(name)
    d = R.data(c, "stats")
    groups, nmb = 2, 4
    per = c["M"] // nmb
    slabs = lambda v, pw: torch.stack([(v[i * per:(i + 1) * per].double() ** pw).sum(0) for i in range(nmb)], 1).float()
    y = R.expected_h(d["ref"])
    assert c["M"] % nmb == 0 and R.stats_exact(c, slabs(y, 1), slabs(y, 2), nmb, groups, y)
    # (7) statistics taken from the unrounded fp32 values
    assert not R.stats_exact(c, slabs(d["ref"], 1), slabs(d["ref"], 2), nmb, groups, y)
    assert not R.stats_exact(c, slabs(y, 1), slabs(d["ref"], 2), nmb, groups, y)
    # (8) one slab counted in the wrong group
    swap = [0, 2, 1, 3]
    assert not R.stats_exact(c, slabs(y, 1)[:, swap], slabs(y, 2)[:, swap], nmb, groups, y)
    half = slabs(y, 1)
    half[0, 0] += R.SQ / 2                                                                          # not an integer number of quanta
    assert not R.stats_exact(c, half, slabs(y, 2), nmb, groups, y)
    # the toleranced form: the exact slabs pass, a slab moved between the groups does not
    dw = R.data(c, "wide")
    yw = R.expected_h(dw["ref"].float().double())
    t1, _ = stat_totals(c, dw["ref"], groups)
    tol1, _ = R.stats_tol(c, dw, groups)
    assert worst(R.slab_sums(slabs(yw, 1), nmb, groups), t1, tol1) <= 1.0
    assert worst(R.slab_sums(slabs(yw, 1)[:, swap], nmb, groups), t1, tol1) > 1.0


# ---- host-side rejections of mma 4, before any launch ------------------------------------------------------------------------------------
def test_mma4_rejections_on_the_host(L):
    lib = L.load()
    before = L.query("arco_conv_last_route")                                                       # (0 on a machine without a GPU)
    buf = (ctypes.c_char * 65536)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)

    def fwd(**kw):
        a = dict(inp=p, ld_in=16, K=16, Wp=p, N=32, out=p, ld_out=32, res=None, taps=9, D3=1)
        a.update(kw)
        return lib.arco_conv3d_fwd(a["inp"], a["ld_in"], a["K"], a["Wp"], a["N"], a["out"], a["ld_out"], None, a["res"], a["N"], None, None,
                                   a["taps"], 2, a["D3"], 4, 4, 1, 4, None)

    for taps in (1, 9, 27):
        assert fwd(taps=taps, res=p) == R.ERR_UNSUPPORTED, taps                                     # no residual in mma 4
        assert fwd(taps=taps, Wp=off) == R.ERR_ARG, taps                                            # the packed weights off a 16-byte boundary
        assert fwd(taps=taps, inp=off) == R.ERR_ARG, taps                                           # ... the input, with K % 8 == 0
    assert fwd(taps=27, K=20, ld_in=20) == R.ERR_UNSUPPORTED                                        # 3x3x3 needs whole 16-byte pieces
    assert fwd(taps=27, K=16, ld_in=20) == R.ERR_UNSUPPORTED
    assert fwd(taps=5) == R.ERR_UNSUPPORTED
    assert L.query("arco_conv_last_route") == before                                               # a rejected call notes no route
