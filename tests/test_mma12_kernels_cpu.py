"""CPU companion of tests/test_mma12_kernels_gpu.py (the reduced-operand modes mma 1 / 2 of arco_conv3d_fwd): what makes that file
trustworthy on a machine without a GPU.
  * every case reaches the route it names through arco_conv_config_mma(.., mma) - the id does not encode the mode, so it is also what
    mma 0 reports - and the narrow shape that mma 0 hands to a stream kernel meets that kernel's conditions except for the mode;
  * the input conditions of every case and kind (tests/mma12_kernel_refs.py): the 2^24 budget before and after rounding, ties on both
    operands, the three rounding rules giving three different references, the rounded reference representable in fp32 and different
    from the unrounded one on at least a quarter of the outputs, one product per output in the impulse and select kinds, subnormal
    and near-65504 operands in the f16 range kinds;
  * the wide kind emulated in fp32 numpy (rounded operands, exact products, fp32 accumulation in k order, epilogue) stays inside the
    derived bound on the small cases; the worst ratios per family are printed and recorded in the GPU file's docstring;
  * planted errors: operands truncated, only A rounded, only B rounded, the other format, no rounding, ties away from zero - each fails
    the fixed kind of EVERY case, and the impulse / select kind wherever it touches that kind's 24-bit operand (unit impulses and
    powers of two are unchanged by any rule; a random 24-bit value is a tie once in 2^13); an accumulation that lands two ulps off at every
    step fails the wide kind;
  * the rejections of arco_conv3d_fwd in the two modes, and that the modes accept exactly the shapes mma 0 accepts."""
import ctypes

import pytest
import torch

import conv_kernel_refs as R
import mma12_kernel_refs as Q
from loss_kernel_refs import worst
from mma12_kernel_refs import CASES, DGRAD, EVERY, FALLBACK, OVERFLOW, names

EMU = ["g256x16", "g128x32", "g32x64", "v128x16", "v64x32", "v32x32", "v64x32-plane", "f128x16", "f64x32", "f32x32", "f64x32-plane"]
EMU = [f"{n}-m{m}" for n in EMU for m in (1, 2)]


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EVERY, ids=names(EVERY))
def test_case_reaches_its_route(L, c):
    args = (c["taps"], c["nv"] * c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_in"])
    assert L.query("arco_conv_config_mma", *args, c["mma"]) == c["route"], c["name"]
    assert L.query("arco_conv_config_mma", *args, 0) == c["route"]                                # the id does not encode the mode
    assert L.query("arco_conv_mblocks_mma", *args, max(1, c["stats"]), c["mma"]) >= max(1, c["stats"])


def test_narrow_shape_meets_the_stream_kernel_except_for_the_mode():
    """conv1x1_stream_dispatch takes M >= 65536, no statistics, no residual, N <= 4, K in {4, 8, 16, 32}, ld_in % 4 == 0 - in mma 0 and 3
    only; the fp32 file runs this very shape (nout-q4-n3-m0) on conv1x1_narrow_out_kernel<4>, id 1616004"""
    for m in (1, 2):
        c = Q.by_name(f"narrow-miss-m{m}")
        assert c["M"] >= 65536 and not c["res"] and not c["stats"] and 1 <= c["n"] <= 4 and c["k"] in (4, 8, 16, 32) and c["ld_in"] % 4 == 0
        assert c["route"] == 1256016 and c["mma"] not in (0, 3)
    f = R.by_name("nout-q4-n3-m0")
    assert (f["M"], f["k"], f["n"], f["route"]) == (257 * 257, 16, 3, 1616004)


def test_every_tile_and_edge_has_a_case_in_both_modes():
    for fam, ids in ((Q.CASES_1X1, (1256016, 1128032, 1032064, 1064064, 1064224, 1128128)),
                     (Q.CASES_RECT, (9128016, 9128032, 9064032, 9128064, 9064064, 9032032)),
                     (Q.CASES_FLAT, (9628016, 9628032, 9564032, 9628064, 9564064, 9532032))):
        for i in ids:
            assert {1, 2} == {c["mma"] for c in fam if c["route"] == i}, i
        for m in (1, 2):
            f = [c for c in fam if c["mma"] == m]
            assert any(c["bias"] and c["res"] and c["in_pad"] > 0 and c["in_off"] > 0 for c in f) or fam is Q.CASES_FLAT
            assert any(c["out_pad"] > 0 for c in f) and (any(c["stats"] == 2 for c in f) or fam is Q.CASES_FLAT)
    assert {7, 14, 28} == {c["w"] for c in Q.CASES_FLAT} and all(c["w"] + 2 <= 64 and c["w"] % 16 for c in Q.CASES_FLAT)
    assert all(c["w"] % 16 == 0 for c in Q.CASES_RECT)
    assert any(c["nv"] * c["d3"] == 1 for c in Q.CASES_RECT) and any(c["nv"] * c["d3"] == 1 for c in Q.CASES_FLAT)
    c = Q.by_name("g64x224-m1")
    assert c["n"] == 448 and 4096 * 1024 < c["M"] * 448 < 4096 * 1024 * 1.01
    assert {c["taps"] for c in DGRAD} == {1, 27} and all(c["mma"] == 2 for c in DGRAD)
    fb = {(c["taps"], c["mma"]) for c in FALLBACK}
    assert fb == {(t, m) for t in (1, 9, 27) for m in (1, 2)}
    assert any(c["k"] == 19 for c in FALLBACK) and any(c["ld_in"] % 4 for c in FALLBACK) and any(c["k"] == 1 and c["taps"] == 27 for c in FALLBACK)
    assert all(c["d3"] == 1 for c in FALLBACK if c["taps"] == 9)


# ---- the rounding rules ---------------------------------------------------------------------------------------------------------------
def test_rounding_rules_on_known_values():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)
    x = t(2049, 2051, -2049, -2051, 2050, 65519.996, 65520, 1e6, 2.0 ** -25, 2.0 ** -25 * 1.5, 2.0 ** -24 * 2.5, 0)
    assert Q.rne_f16(x).tolist() == [2048, 2052, -2048, -2052, 2050, 65504, float("inf"), float("inf"), 0, 2.0 ** -24, 2.0 ** -23, 0]
    assert Q.trunc_f16(x).tolist() == [2048, 2050, -2048, -2050, 2050, 65504, 65504, 65504, 0, 0, 2.0 ** -23, 0]
    assert Q.away_f16(x)[:5].tolist() == [2050, 2052, -2050, -2052, 2050] and Q.away_f16(x)[8:].tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -24 * 3, 0]
    y = t(257, 259, -257, -259, 258, 256.5, 0)
    assert Q.rne_bf16(y).tolist() == [256, 260, -256, -260, 258, 256, 0]
    assert Q.trunc_bf16(y).tolist() == [256, 258, -256, -258, 258, 256, 0]
    assert Q.away_bf16(y).tolist() == [258, 260, -258, -260, 258, 256, 0]
    v = R._wide_values((4096,), R.gen(3), 3, 0.1)
    assert torch.equal(Q.rne_bf16(v), v.bfloat16().float())                                        # the integer form against torch's own
    for rule in (Q.away_f16, Q.trunc_f16):                                                          # off the ties: nearest / the neighbour below
        assert bool(((rule(v) - v).abs() < 2.0 ** -10 * v.abs() + 2.0 ** -24).all())
    off = Q.trunc_f16(v) + (Q.rne_f16(v) - Q.trunc_f16(v)) / 2 != v                                 # not half way between two neighbours
    assert torch.equal(Q.away_f16(v)[off], Q.rne_f16(v)[off]) and float(off.float().mean()) > 0.85        # (the rest: the 10 % zeros)


# ---- input conditions ------------------------------------------------------------------------------------------------------------------
def _quanta(c, d, rx, rw):
    s = R.conv64(rx(d["x"]).double().abs(), rw(d["w"]).double().abs(), c)
    for t in (d["bias"], d["res"]):
        if t is not None:
            s = s + t.double().abs()
    return float(s.max()) / R.QUANT


@pytest.mark.parametrize("c", CASES + DGRAD + FALLBACK, ids=names(CASES + DGRAD + FALLBACK))
def test_fixed_kind_conditions(c):
    m, K = c["mma"], c["k"]
    d = Q.data(c, "fixed")
    rne = Q.RNE[m]
    assert _quanta(c, d, rne, rne) < 2 ** 24 and _quanta(c, d, Q.ident, Q.ident) < 2 ** 24       # the budget, after rounding and before
    assert Q.representable(d["ref"])
    raw = Q.unrounded(c, d)
    assert Q.representable(raw) and Q.differs(d["ref"], raw) >= 0.25, Q.differs(d["ref"], raw)
    if K > 1:
        tx, tw = Q.tie_channels(c)
        assert tx and tw and not set(tx) & set(tw)
        bits = Q.TIE_BITS[m]
        for vals, q in ((d["x"][:, tx], R.QX), (d["w"][:, tw, :], R.QW)):                          # ties present in both operands
            i = (vals.double() / q)
            assert bool((i == i.round()).all()) and bool((i.abs() % 2 == 1).all()) and bool((i.abs() > 2 ** (bits - 1)).all()) and bool((i.abs() < 2 ** bits).all())
            assert {1, 3} == set((i.abs() % 4).long().flatten().tolist()) and bool((i > 0).any()) and bool((i < 0).any())
            assert bool((rne(vals) != vals).all()) and bool((Q.TRUNC[m](vals) != Q.AWAY[m](vals)).all())
        assert bool((d["x"][:, tw].abs() <= 3 * R.QX).all()) and bool((d["w"][:, tx, :].abs() <= 3 * R.QW).all())   # against small integers
    # round-to-nearest-even, truncation and half-away-from-zero: three different references
    tr, aw = Q.with_rules(c, d, Q.TRUNC[m], Q.TRUNC[m]), Q.with_rules(c, d, Q.AWAY[m], Q.AWAY[m])
    assert Q.differs(d["ref"], tr) > 0.25 and Q.differs(d["ref"], aw) > 0.25 and Q.differs(tr, aw) > 0.25


@pytest.mark.parametrize("c", Q.having("impulse"), ids=names(Q.having("impulse")))
def test_impulse_kind_conditions(c):
    m, T = c["mma"], c["taps"]
    d = Q.data(c, "impulse")
    rows = Q.impulse_rows(c)
    assert len(set(rows)) == len(rows) and int((d["x"] != 0).sum()) == len(rows) and bool((d["x"][d["x"] != 0] == 1).all())
    hits = R.conv64((d["x"] != 0).double(), torch.ones_like(d["w"]).double(), c)
    assert float(hits.max()) == 1.0                                                               # one product per output at most
    assert Q.representable(d["ref"]) and Q.differs(d["ref"], Q.unrounded(c, d)) >= 0.25
    nz = d["ref"] != 0
    assert bool(torch.isin(d["ref"][nz].float(), Q.RNE[m](d["w"]).flatten()).all())               # every output is rne(w) or zero
    a = d["w"].abs()
    assert bool(torch.isfinite(Q.RNE[m](d["w"])).all())
    if m == 1:
        assert bool(((a >= 2.0 ** -24) & (a < 2.0 ** -14)).any()) and bool(((a > 65504 - 32) & (a < 65520) & (a != 65504)).any())
        assert float(a.max()) < 65520 and bool(((a > 0) & (a <= 2.0 ** -25)).any())              # (flushed to zero by the rounding itself)
    else:
        assert float(a.max()) > 2.0 ** 40 and float(a[a > 0].min()) < 2.0 ** -40
    assert 0 in rows and float((hits > 0).double().mean()) > 0.5                                  # most outputs are one product


@pytest.mark.parametrize("c", Q.having("select"), ids=names(Q.having("select")))
def test_select_kind_conditions(c):
    m = c["mma"]
    used = set()
    for p in range(Q.select_passes(c)):
        d = Q.data(c, "select", p)
        assert bool(((d["w"] != 0).sum((1, 2)) == 1).all()) and torch.equal(Q.RNE[m](d["w"]), d["w"])     # +-2^e: unchanged by the rounding
        assert Q.representable(d["ref"]) and Q.differs(d["ref"], Q.unrounded(c, d)) >= 0.25, p
        assert bool(torch.isfinite(Q.RNE[m](d["x"])).all()) and float((d["x"] == 0).float().mean()) > 0.1
        used |= set(torch.nonzero(d["w"])[:, 2].tolist())
    assert used == set(range(c["taps"]))                                                          # every tap used by some channel
    a = Q.data(c, "select")["x"].abs()
    if m == 1 and a.numel() >= 4000:
        assert bool(((a >= 2.0 ** -24) & (a < 2.0 ** -14)).any()) and bool((a > 65504 - 32).any())


@pytest.mark.parametrize("c", Q.having("wide", CASES + DGRAD), ids=names(Q.having("wide", CASES + DGRAD)))
def test_wide_kind_conditions(c):
    d = Q.data(c, "wide")
    assert bool(((d["S"] > 0) | (d["ref"] == 0)).all()) and bool(torch.isfinite(d["ref"]).all())
    assert float((d["x"] == 0).float().mean()) > 0.1
    nzx = d["x"][d["x"] != 0].abs()
    assert nzx.numel() < 1000 or float(nzx.max() / nzx.min()) > 1e6                               # six decades
    assert c["mma"] == 2 or (float(d["x"].abs().max()) <= Q.MAXH and float(d["w"].abs().max()) <= Q.MAXH)
    assert Q.differs(d["ref"], Q.unrounded(c, d)) > 0.9


@pytest.mark.parametrize("c", [c for c in CASES if c["stats"]], ids=names([c for c in CASES if c["stats"]]))
def test_stats_kind_fits_the_budget(c):
    d = Q.data(c, "stats")
    assert Q.representable(d["ref"]) and torch.equal(d["ref"], Q.unrounded(c, d))                 # {-1, 0, 1}: no rounding in either format
    assert float((d["ref"] ** 2).sum(0).max()) / R.QUANT ** 2 < 2 ** 24 and float(d["ref"].abs().max()) > 0
    t1, t2 = R.stat_totals(c, d["ref"], c["stats"])
    assert bool((t1 / R.QUANT == (t1 / R.QUANT).round()).all()) and t2.shape == (c["stats"], c["n"])


@pytest.mark.parametrize("c", DGRAD, ids=names(DGRAD))
def test_data_gradient_reference_is_float64_autograd_on_rounded_operands(c):
    f = Q.data(c, "fixed")
    assert torch.equal(Q.dgrad_autograd(c, f), f["ref"])
    d = Q.data(c, "wide")
    n, u64 = c["taps"] * c["k"], 2.0 ** -53
    assert worst(Q.dgrad_autograd(c, d), d["ref"], 2 * n * u64 / (1 - n * u64) * d["S"]) <= 1.0


def test_overflow_kind_is_ieee_on_the_rounded_operands():
    c, d = OVERFLOW, Q.data(OVERFLOW, "overflow")
    ref = d["ref"]
    assert c["mma"] == 1 and bool((ref == float("inf")).any()) and bool((ref == float("-inf")).any()) and bool(torch.isnan(ref).any())
    assert bool(torch.isfinite(ref).any()) and bool((d["x"] == 65520.0).any()) and bool((d["x"] == 1e6).any())
    xr = Q.rne_f16(d["x"])
    assert bool(torch.isinf(xr[d["x"].abs() >= 65520]).all()) and bool(torch.isfinite(xr[d["x"].abs() < 65520]).all())
    rows = torch.isinf(xr).any(1)
    assert bool(torch.isfinite(ref[~rows]).all()) and not bool(torch.isfinite(ref[rows]).any())   # inf * w, or inf * 0 = NaN, in those rows
    sat = (xr.clamp(-Q.MAXH, Q.MAXH).double() @ d["w"][:, :, 0].double().t())                      # what saturation would give: all finite
    assert bool(torch.isfinite(sat).all()) and not torch.equal(torch.nan_to_num(ref), torch.nan_to_num(sat))
    assert torch.equal(ref[~rows], sat[~rows])


def test_ops_problems_give_three_bit_patterns():
    """the single-product problems of the GPU file's ops.py tests: forward, data gradient and weight gradient each have an fp32, an
    f16-rounded and a bf16-rounded pattern that are representable in fp32 and pairwise different (asserted inside _patterns)"""
    import test_mma12_kernels_gpu as G
    for key in G.OPS:
        dims, c, x, w, dy, pat = G._problem(key)
        assert set(pat) == {0, 1, 2} and bool((Q.rne_f16(x) != x).all()) and bool((Q.rne_bf16(x) != Q.rne_f16(x)).all()), key
        assert int((w != 0).sum()) == c["n"] and bool(((dy != 0).sum(0) == 1).all())              # one weight, one gradient row per channel


# ---- the emulation stays inside the bound ---------------------------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize("name", EMU)
def test_bound_holds_for_the_emulation(name):
    c = Q.by_name(name)
    d = Q.data(c, "wide")
    r1, r2 = Q.held(f"emulated {name} [{Q.FAMILY[name]}]", Q.emulate(c, d), c, d)
    assert r1 <= 1.0
    key = (Q.FAMILY[name], c["mma"])
    _worst[key] = tuple(max(a, b) for a, b in zip(_worst.get(key, (0.0, 0.0)), (r1, r2)))
    for kind in Q.EXACT:                                                                          # the exact kinds are exact in ANY fp32 order
        e = Q.data(c, kind)
        assert Q.equal_bits(Q.emulate(c, e), e["ref"]), kind


def test_emulation_worst_ratios_per_family():
    """prints what the tests above gathered (nothing when run alone): the figures of the GPU file's docstring table"""
    for (fam, m), (r1, r2) in sorted(_worst.items()):
        print(f"emulation, {fam}, mma {m}: worst err / bound {r1:.4f}, err / (3e-6 S_r) {r2:.3f}")


# ---- planted errors --------------------------------------------------------------------------------------------------------------------
TOUCHES = {"impulse": ("operands truncated", "only A rounded", "the other format", "no rounding"),      # the kind's 24-bit operand is w
           "select": ("operands truncated", "only B rounded", "the other format", "no rounding")}       # ... is x


@pytest.mark.parametrize("c", CASES + DGRAD, ids=names(CASES + DGRAD))
def test_planted_operand_errors_fail_the_exact_kinds(c):
    d = Q.data(c, "fixed")
    assert Q.equal_bits(d["ref"].float(), d["ref"])
    for name, rx, rw in Q.planted(c["mma"]):
        assert not Q.equal_bits(Q.with_rules(c, d, rx, rw).float(), d["ref"]), name               # fixed: ties on both operands catch all six
    for kind, which in TOUCHES.items():
        if kind not in c["kinds"]:
            continue
        e = Q.data(c, kind)
        for name, rx, rw in Q.planted(c["mma"]):
            bad = Q.with_rules(c, e, rx, rw)
            if name in which:
                assert not (Q.representable(bad) and Q.equal_bits(bad.float(), e["ref"])), (kind, name)
            elif name != "ties away from zero":                                                   # 1.0 and +-2^e are fixed points of every rule
                assert torch.equal(bad, e["ref"]), (kind, name)                                   # (a random 24-bit value is a tie once in 2^13)


@pytest.mark.parametrize("name", ["g256x16-m1", "g32x64-m2", "v64x32-m1", "f64x32-m2"])
def test_planted_accumulation_error_fails_the_wide_kind(name):
    """an accumulator that lands two ulps further from zero at every step, on data of one sign (|x|, |w|: S = ref, the partial sums grow
    to it, and the error gathers about 3 u per step against the bound's 1 u); the unplanted emulation of the same data passes"""
    c = Q.by_name(name)
    d = dict(Q.data(c, "wide"))
    d["x"], d["w"], d["bias"], d["res"] = d["x"].abs(), d["w"].abs(), None, None
    d["ref"] = Q.reference(c, d["x"], d["w"], None, None, Q.RNE[c["mma"]], Q.RNE[c["mma"]])[0]
    d["S"] = d["ref"].clone()
    assert worst(Q.emulate(c, d), d["ref"], Q.tol_wide(c, d)) <= 1.0
    assert worst(Q.emulate(c, d, ulps=2), d["ref"], Q.tol_wide(c, d)) > 1.0


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_in_the_reduced_modes(L):
    """the argument checks of arco_conv3d_fwd hold in mma 1 / 2 as in mma 0 (ARCO_ERR_ARG on the host, no route noted), a tap count
    without a kernel is ARCO_ERR_UNSUPPORTED; and the modes accept exactly what mma 0 accepts - the split pack's preconditions
    (K % 4, ld_in % 4), which make mma 3 refuse a shape, do not refuse it here (it runs the fp32 arithmetic), and nothing mma 0
    refuses is accepted."""
    lib = L.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(**kw):
        a = dict(inp=p, ld_in=16, K=16, Wp=p, N=16, out=p, ld_out=16, bias=None, res=None, ld_res=0, s1=None, s2=None, taps=27, NV=2, D3=2, H=4,
                 W=4, groups=1, mma=1)
        a.update(kw)
        return lib.arco_conv3d_fwd(a["inp"], a["ld_in"], a["K"], a["Wp"], a["N"], a["out"], a["ld_out"], a["bias"], a["res"], a["ld_res"], a["s1"],
                                   a["s2"], a["taps"], a["NV"], a["D3"], a["H"], a["W"], a["groups"], a["mma"], None)

    before = L.query("arco_conv_last_route")
    for mma in (1, 2):
        for bad in (dict(inp=None), dict(Wp=None), dict(out=None), dict(K=0), dict(N=0), dict(NV=0), dict(H=0), dict(W=0), dict(D3=0),
                    dict(NV=3, groups=2)):
            assert fwd(mma=mma, **bad) == R.ERR_ARG, (mma, bad)
        assert L.query("arco_conv_last_route") == before
    for mma in (1, 2):
        assert fwd(mma=mma, taps=5) == R.ERR_UNSUPPORTED and L.query("arco_conv_last_route") == 0
    for taps in (1, 9, 27):
        for nb in (1, 8):
            for h, w in ((7, 5), (16, 16), (33, 45), (7, 28)):
                for cin, cout in ((1, 16), (16, 16), (19, 20), (20, 48), (64, 128)):
                    for ld in (cin, cin + 1, cin + 4):
                        shape = (taps, nb, h, w, cin, cout, ld)
                        want = lib.arco_conv_config_mma(*shape, 0)
                        assert want > 0
                        assert lib.arco_conv_config_mma(*shape, 1) == want and lib.arco_conv_config_mma(*shape, 2) == want, shape
                        if cin > 4 and (cin % 4 or ld % 4):
                            assert lib.arco_conv_config_mma(*shape, 3) == R.ERR_UNSUPPORTED, shape
                        for g in (1, 2):
                            nm = lib.arco_conv_mblocks_mma(*shape, g, 0)
                            assert lib.arco_conv_mblocks_mma(*shape, g, 1) == nm and lib.arco_conv_mblocks_mma(*shape, g, 2) == nm, shape
    assert lib.arco_conv_config_mma(5, 1, 8, 8, 16, 16, 16, 1) == R.ERR_UNSUPPORTED and lib.arco_conv_config_mma(5, 1, 8, 8, 16, 16, 16, 0) == R.ERR_UNSUPPORTED
