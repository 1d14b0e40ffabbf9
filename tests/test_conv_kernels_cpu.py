"""CPU companion of tests/test_conv_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * every case reaches the route it names: arco_conv_config_mma / arco_conv_mblocks_mma are host-only (with no device conv_sp_cus()
    falls back to 256, the MI355X figure); the launch-only routes (the 1x1 streams, gemm_sp_kernel), which no query describes, have
    their dispatch conditions restated here;
  * the input conditions of every case and kind: the 2^24 bit budget and the two-term operands of the fixed kind, the spacing of the
    impulses, one product per output in both impulse kinds, S > 0 wherever the reference is not zero, and the float64 reference
    exactly representable in fp32 for the exact kinds;
  * the wide kind emulated in fp32 (both split rules: split_bf16.h and the weight pack of igemm.hip, the six kept products formed exactly, one fixed accumulation
    order) stays inside the same bounds; the ratios are printed and recorded in the GPU file's docstring;
  * each comparison helper rejects a planted error: one tap mirrored, one border column not zero-padded, channels k and k + 16
    swapped, the plane-1 term of one weight dropped, the bias added twice on one tile, one slab counted in the wrong group;
  * the argument checks of the entry points return ARCO_ERR_ARG on the host, before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import conv_kernel_refs as R
from loss_kernel_refs import worst

EMU = ["nout-q2-n2-m3", "nout-q8-n4-m3", "nin-k3-n16-both", "g256x16-m0", "g256x16-m3", "g128x32-m3", "g32x64-m0", "g32x64-m3",
       "image1-k1-small", "image-k4-n12", "halo-32-16", "s64x16-m0", "s64x16-m3", "s64x32-m3", "s32x32-m3", "sp-4-1-small",
       "image3-small", "v64x32-m3", "f64x32-m3", "f32x32-m0", "f32x32-m3"]


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def names(cases):
    return [c["name"] for c in cases]


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES + R.DGRAD, ids=names(R.CASES + R.DGRAD))
def test_case_reaches_its_route(L, c):
    args = (c["taps"], c["nv"] * c["d3"], c["h"], c["w"], c["k"], c["n"], c["ld_in"])
    prev = L.query("arco_conv3d_fl_set", 0) if c["fl0"] else None
    try:
        got = L.query("arco_conv_config_mma", *args, c["mma"])
        nmb = L.query("arco_conv_mblocks_mma", *args, max(1, c["stats"]), c["mma"])
    finally:
        if prev is not None:
            L.query("arco_conv3d_fl_set", prev)
    assert nmb >= 1
    if not c["launch_only"]:
        assert got == c["route"], (c["name"], got)
        return
    # the launch-only routes: the conditions of conv1x1_stream_dispatch / gemm_sp_dispatch restated
    K, N, M = c["k"], c["n"], c["M"]
    if c["fam"] == "nout":
        assert M >= 65536 and not c["res"] and not c["stats"] and 1 <= N <= 4 and K in (4, 8, 16, 32) and c["ld_in"] % 4 == 0 and c["in_off"] % 4 == 0
        assert c["mma"] in (0, 3) and c["route"] == 1600000 + K * 1000 + 4
    elif c["fam"] == "nin":
        assert M >= 65536 and c["mma"] == 0 and 1 <= K <= 4 and N in (4, 8, 16, 32) and c["ld_out"] % 4 == 0 and (not c["res"] or c["ld_res"] % 4 == 0)
        assert c["route"] == 1700000
    else:
        npad, nb = R.ceil_to(N, 16), -(-R.ceil_to(N, 16) // 256)
        assert c["gsp"] and c["mma"] == 3 and K % 4 == 0 and N % 4 == 0 and c["ld_in"] % 4 == 0 and c["ld_out"] % 4 == 0 and c["ld_res"] % 4 == 0
        assert npad >= 64 and R.ceil_to(K, 32) >= 32 and nb * 256 - npad <= nb * 256 // 5 and c["route"] == 1464256


def test_plain_queries_are_the_mma0_case_of_their_twins(L):
    """arco_conv_mblocks / arco_conv_config answer what arco_conv_mblocks_mma / arco_conv_config_mma answer for mma = 0 (one shape record
    and one route behind all four), and arco_conv_config fills *kc_depth_db whenever it names a kernel.  Host only: 384 shapes."""
    lib = L.load()
    seen = 0
    for taps in (1, 9, 27):
        for nb in (1, 8):
            for h, w in ((7, 5), (16, 16), (33, 45), (64, 64)):
                for cin, cout in ((1, 16), (16, 16), (20, 48), (64, 128)):
                    for ld in (cin, cin + 4):
                        shape = (taps, nb, h, w, cin, cout, ld)
                        kdd = ctypes.c_int(-1)
                        cfg = lib.arco_conv_config(*shape, ctypes.byref(kdd))
                        assert cfg == lib.arco_conv_config_mma(*shape, 0), shape
                        if cfg > 0:
                            assert kdd.value > 0, (shape, cfg)
                            seen += 1
                        for groups in (1, 2):
                            assert lib.arco_conv_mblocks(*shape, groups) == lib.arco_conv_mblocks_mma(*shape, groups, 0), (shape, groups)
    assert seen > 0


def test_refused_width_of_the_pipelined_gemm_is_what_the_dispatcher_says():
    """N = 64 (one of the issue's widths) wastes three quarters of a 256-wide tile: gemm_sp_dispatch's padding rule refuses it at any tile
    threshold, and the case asserts igemm_kernel<1,32,64> instead; the narrowest width it takes is Npad = 208"""
    assert 256 - 64 > 256 // 5 and 256 - 208 <= 256 // 5 and 256 - 192 > 256 // 5
    assert R.by_name("gsp-n64-refused")["route"] == 1032064


def test_every_family_has_every_edge():
    for taps in (1, 9, 27):
        fam = [c for c in R.CASES if c["taps"] == taps]
        assert any(c["n"] in (19, 4, 2) for c in fam) and any(c["k"] in (20, 48) for c in fam)
        assert any(c["in_off"] > 0 and c["in_pad"] > 0 for c in fam) and any(c["out_pad"] > 0 for c in fam) and any(c["res_pad"] > 0 for c in fam)
        assert any(c["bias"] and not c["res"] for c in fam) and any(c["res"] and not c["bias"] for c in fam) and any(c["bias"] and c["res"] for c in fam)
        assert any(c["nv"] * c["d3"] == 1 for c in fam) and any(c["nv"] > 1 for c in fam)
        if taps > 1:
            assert any(c["h"] % 16 and c["w"] % 16 for c in fam) and any(c["h"] < 8 and c["w"] < 16 for c in fam)
    assert sorted({c["route"] for c in R.CASES if c["route"] // 1000 in (9301, 9302, 9304)}) == [9301032, 9301064, 9302032, 9302064, 9304016, 9304032, 9304064]
    assert {1604004, 1608004, 1616004, 1632004, 1700000, 1464256} <= {c["route"] for c in R.CASES}
    for t in (256016, 128016, 64016, 128032, 64032, 128064, 64064, 32032):
        assert {0, 3} == {c["mma"] for c in R.CASES if c["route"] == 9000000 + t and c["taps"] == 9}, t
    for t in (128016, 128032, 64032, 128064, 64064, 32032):
        for flat in (0, 500000):
            assert {0, 3} == {c["mma"] for c in R.CASES if c["route"] == 9000000 + flat + t and c["taps"] == 27}, (t, flat)


# ---- input conditions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=names(R.CASES))
def test_input_conditions(c):
    K, T = c["k"], c["taps"]
    if "fixed" in c["kinds"]:
        d = R.data(c, "fixed")
        assert float(d["S"].max()) / R.QUANT < 2 ** 24 and R.representable(d["ref"])
        wide = R.wide_channels(c)
        xs, ws = R.split_act(d["x"].numpy()[:, wide]), R.split_weight(d["w"].numpy()[:, wide, :])
        assert bool((R.n_terms(xs[:2]) == 2).all()) and bool((xs[2] == 0).all())                # two non-zero terms, planes 0 and 1
        assert bool((R.n_terms(ws[:2]) == 2).all()) and bool((ws[2] == 0).all())
        assert bool((xs[0] + xs[1] == d["x"].numpy()[:, wide]).all())
        if c["mma"] == 3 and K > 16:
            assert max(wide) >= 16 or len(wide) == 1                                              # the second 16-k group too
    if "impulse" in c["kinds"]:
        d = R.data(c, "impulse")
        rows = R.impulse_positions(c)
        assert len(set(rows)) == len(rows) >= 1 and int((d["x"] != 0).sum()) == len(rows)
        assert bool(((d["x"] != 0).sum(0) <= -(-len(rows) // K)).all())                           # each in a channel of its own (K < 16: in turn)
        hits = R.conv64((d["x"] != 0).double(), torch.ones_like(d["w"]).double(), c)
        assert float(hits.max()) <= 1.0 and R.representable(d["ref"])                             # one product per output at most
        spanned = [] if T == 1 else [c["h"], c["w"]] + ([c["d3"]] if T == 27 else [])
        assert 0 in rows and (c["M"] - 1 in rows or T == 1 or min(spanned) < 5)                   # both borders where the axis has room for two
        # every output is one weight, bit for bit
        nz = d["ref"] != 0
        assert bool(torch.isin(d["ref"][nz].float(), d["w"].flatten()).all())
    if "select" in c["kinds"]:
        used = set()
        for p in range(R.select_passes(c)):
            d = R.data(c, "select", p)
            assert bool(((d["w"] != 0).sum((1, 2)) == 1).all()) and R.representable(d["ref"])
            used |= set(torch.nonzero(d["w"])[:, 2].tolist())
        assert used == set(range(T))                                                              # every tap used by some channel
    if "wide" in c["kinds"]:
        d = R.data(c, "wide")
        assert bool(((d["S"] > 0) | (d["ref"] == 0)).all())
        assert float((d["x"] == 0).float().mean()) > 0.1
        nzx = d["x"][d["x"] != 0].abs()
        assert nzx.numel() < 1000 or float(nzx.max() / nzx.min()) > 1e6                            # six decades (a 15-pixel plane has too few values)


@pytest.mark.parametrize("c", [c for c in R.CASES if c["stats"]], ids=names([c for c in R.CASES if c["stats"]]))
def test_stats_kind_fits_the_budget(c):
    d = R.data(c, "stats")
    assert R.representable(d["ref"])
    assert float((d["ref"] ** 2).sum(0).max()) / R.QUANT ** 2 < 2 ** 24 and float(d["ref"].abs().max()) > 0
    t1, t2 = R.stat_totals(c, d["ref"], c["stats"])
    assert bool((t1 / R.QUANT == (t1 / R.QUANT).round()).all()) and t2.shape == (c["stats"], c["n"])


@pytest.mark.parametrize("c", R.DGRAD, ids=names(R.DGRAD))
def test_data_gradient_reference_is_float64_autograd(c):
    """the mode-1 pack read as a forward weight (conv64 of dY with the flipped, transposed weight) and float64 autograd of the forward
    layer are the same sums: equal on fixed-point data; on wide data two float64 summations of the same taps K products in different
    orders, each within gamma64(taps K) S of the exact sum (u64 = 2^-53)"""
    f = R.data(c, "fixed", 0, True)
    assert torch.equal(R.dgrad_autograd(c, f), f["ref"]) and R.representable(f["ref"])
    d = R.data(c, "wide", 0, True)
    n, u64 = c["taps"] * c["k"], 2.0 ** -53
    assert worst(R.dgrad_autograd(c, d), d["ref"], 2 * n * u64 / (1 - n * u64) * d["S"]) <= 1.0


# ---- the emulation stays inside the bounds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EMU)
def test_bounds_hold_for_the_emulation(name):
    c = R.by_name(name)
    d = R.data(c, "wide")
    r1, r2 = R.held(f"emulated {name} [{R.FAMILY[c['taps']]} {c['fam']}]", R.emulate(c, d), c, d)
    assert r1 <= 1.0 and r2 <= 1.0
    f = R.data(c, "fixed")
    assert R.equal_bits(R.emulate(c, f), f["ref"])                                                # the exact kinds are exact in ANY fp32 order
    for kind in ("impulse", "select"):
        if kind in c["kinds"]:
            e = R.data(c, kind)
            assert R.equal_bits(R.emulate(c, e), e["ref"])


def test_split_rules_are_exact_decompositions():
    v = R._wide_values((4096,), R.gen(5), 4, 0.1).numpy()
    for parts in (R.split_weight(v), R.split_act(v)):
        assert bool(((parts[2].astype(np.float64) + parts[1]) + parts[0] == v).all())
        for p in parts:
            assert bool((R.bf16_trunc(p) == p).all())                                              # every term a bf16 value
    t = R.split_act(v)
    assert bool((np.abs(t[1]) <= 2.0 ** -8 * np.abs(v)).all()) and bool((np.abs(t[2]) <= 2.0 ** -15 * np.abs(v)).all())


# ---- planted errors ------------------------------------------------------------------------------------------------------------------------
def _got(c, d, x=None, w=None):
    y = R.conv64((d["x"] if x is None else x).double(), (d["w"] if w is None else w).double(), c)
    for t in (d["bias"], d["res"]):
        if t is not None:
            y = y + t.double()
    return y.float()


def _leaky(c, d):
    """the convolution with the left padding column of every plane filled from the flat memory in front of the row (what a loader
    without its x >= 0 test reads) instead of zeros"""
    K, N, T = c["k"], c["n"], c["taps"]
    x, w = d["x"].double(), d["w"].double()
    flat = torch.cat([torch.zeros(1, K, dtype=torch.float64), x[:-1]])                             # row m - 1 at row m
    planes = c["nv"] * c["d3"]
    v = x.view(planes, c["h"], c["w"], K)
    left = flat.view(planes, c["h"], c["w"], K)[:, :, :1]                                         # what sits in front of column 0
    vp = torch.cat([left, v, torch.zeros_like(left)], 2)                                          # W padded by hand
    if T == 9:
        y = torch.nn.functional.conv2d(vp.permute(0, 3, 1, 2), w.view(N, K, 3, 3), padding=(1, 0)).permute(0, 2, 3, 1)
    else:
        v5 = vp.view(c["nv"], c["d3"], c["h"], c["w"] + 2, K).permute(0, 4, 1, 2, 3)
        y = torch.nn.functional.conv3d(v5, w.view(N, K, 3, 3, 3), padding=(1, 1, 0)).permute(0, 2, 3, 4, 1)
    y = y.reshape(-1, N)
    for t in (d["bias"], d["res"]):
        if t is not None:
            y = y + t.double()
    return y.float()


@pytest.mark.parametrize("name", ["s64x32-m3", "halo-32-16", "f64x32-m3", "v64x32-m0"])
def test_helpers_reject_planted_errors(name):
    c = R.by_name(name)
    T, K = c["taps"], c["k"]
    for kind in c["kinds"]:
        d = R.data(c, kind)
        ok = (lambda g: R.equal_bits(g, d["ref"])) if kind != "wide" else (lambda g: max(R.held("planted", g, c, d)) <= 1.0)
        assert ok(_got(c, d))                                                                     # the unplanted result passes
        if kind == "impulse":
            n, ch = 1, 0                                                                          # channel 0 holds the impulse at row 0
        else:
            n, ch = (1, int(torch.nonzero(d["w"][1])[0, 0])) if kind == "select" else (1, R.wide_channels(c)[0])
        # (1) one tap mirrored: taps dx = 0 and dx = 2 of one (n, channel) exchanged
        w = d["w"].clone().view(c["n"], K, T // 3, 3)
        w[n, ch] = w[n, ch].flip(-1)
        if not torch.equal(w.view_as(d["w"]), d["w"]):
            assert not ok(_got(c, d, w=w.view_as(d["w"])))
        # (3) channels k and k + 16 swapped in the activations
        x = d["x"].clone()
        a, b = ch, (ch + 16) % K                                                                  # (K = 20: 16 channels on, modulo K)
        x[:, [a, b]] = x[:, [b, a]]
        assert not ok(_got(c, d, x=x)) or torch.equal(_got(c, d, x=x), _got(c, d))
    # (2) one border column not zero-padded: the left neighbours of column 0 read the last column of the row above
    for kind in ("fixed", "wide"):
        d = R.data(c, kind)
        bad = _leaky(c, d)
        assert not torch.equal(bad, _got(c, d))
        assert not (R.equal_bits(bad, d["ref"]) if kind == "fixed" else max(R.held("planted", bad, c, d)) <= 1.0)
    # (4) the plane-1 term of one weight dropped
    for kind in ("fixed", "impulse"):
        d = R.data(c, kind)
        ch = R.wide_channels(c)[0] if kind == "fixed" else 0
        w = d["w"].clone()
        b = R.split_weight(w[0, ch, T // 2:T // 2 + 1].numpy())
        assert float(b[1][0]) != 0
        w[0, ch, T // 2] = float(b[0][0] + b[2][0])
        assert not R.equal_bits(_got(c, d, w=w), d["ref"])
    # (5) the bias added twice on one tile
    for kind in ("fixed", "wide"):
        d = R.data(R.by_name("s64x32-m3"), kind)
        cc = R.by_name("s64x32-m3")
        g = _got(cc, d)
        g[:16] += d["bias"]
        assert not (R.equal_bits(g, d["ref"]) if kind == "fixed" else max(R.held("planted", g, cc, d)) <= 1.0)


def test_stats_helper_rejects_a_slab_in_the_wrong_group():
    c = R.by_name("fl-7-64-32-d4")
    d = R.data(c, "stats")
    groups, nmb = 2, 4
    y = d["ref"].float()
    per = c["M"] // nmb
    ssum = torch.stack([y[i * per:(i + 1) * per].double().sum(0) for i in range(nmb)], 1).float()
    ssq = torch.stack([(y[i * per:(i + 1) * per].double() ** 2).sum(0) for i in range(nmb)], 1).float()
    assert R.stats_exact(c, ssum, ssq, nmb, groups, d["ref"])
    swap = [0, 2, 1, 3]                                                                           # slab 1 counted in group 1, slab 2 in group 0
    assert not R.stats_exact(c, ssum[:, swap], ssq[:, swap], nmb, groups, d["ref"])
    half = ssum.clone()
    half[0, 0] += R.QUANT / 2                                                                     # not an integer number of quanta
    assert not R.stats_exact(c, half, ssq, nmb, groups, d["ref"])
    # the toleranced form: the exact slabs pass, a slab moved between the groups does not
    dw = R.data(c, "wide")
    yw = dw["ref"].float()
    s1 = torch.stack([yw[i * per:(i + 1) * per].double().sum(0) for i in range(nmb)], 1).float()
    t1, _ = R.stat_totals(c, dw["ref"], groups)
    tol1, _ = R.stats_tol(c, dw, groups)
    assert worst(R.slab_sums(s1, nmb, groups), t1, tol1) <= 1.0
    assert worst(R.slab_sums(s1[:, swap], nmb, groups), t1, tol1) > 1.0


# ---- the packed layouts ---------------------------------------------------------------------------------------------------------------
def test_pack_restatement_round_trips():
    rs = np.random.RandomState(1)
    W = rs.standard_normal((5, 7, 9)).astype(np.float32)
    for mode in (0, 1):
        lg = R.pack_logical(W, 5, 7, 9, mode)
        n, k = (5, 7) if mode == 0 else (7, 5)
        assert lg.shape == (9, n, k) and lg[2, n - 1, k - 1] == (W[4, 6, 2] if mode == 0 else W[4, 6, 6])
        sp = R.pack_expected(lg, mode | 2, 16, 32).astype(np.int64).reshape(9, 16, 2, 3, 16)
        val = ((sp.astype(np.uint32) & 0xFFFF) << 16).astype(np.uint32).view(np.float32).astype(np.float64)
        assert bool((val.sum(3).reshape(9, 16, 32)[:, :n, :k] == lg).all()) and bool((val.sum(3).reshape(9, 16, 32)[:, n:, :] == 0).all())
    # the gather forms against torch's own k2 s2 convolutions written as GEMMs
    ci, co = 3, 4
    Wc = torch.randn(co, ci, 2, 2, 2, dtype=torch.float64)
    x = torch.randn(1, ci, 2, 2, 2, dtype=torch.float64)
    W2 = torch.from_numpy(R.pack_gather_logical(Wc.float().numpy(), co, 8 * ci, ci, 1, 0)[0]).double()
    cols_ = x[0].permute(1, 2, 3, 0).reshape(8 * ci)                                              # [t][c]
    assert torch.allclose(W2 @ cols_, torch.nn.functional.conv3d(x.float().double(), Wc.float().double(), stride=2).flatten())
    Wt = torch.randn(ci, co, 2, 2, 2, dtype=torch.float64)
    W2t = torch.from_numpy(R.pack_gather_logical(Wt.float().numpy(), 8 * co, ci, co, 2, 0)[0]).double()
    xin = torch.randn(1, ci, 1, 1, 1, dtype=torch.float64)
    up = torch.nn.functional.conv_transpose3d(xin.float().double(), Wt.float().double(), stride=2)[0]      # [co, 2, 2, 2]
    assert torch.allclose((W2t @ xin.float().double().flatten()).view(8, co), up.permute(1, 2, 3, 0).reshape(8, co))


# ---- argument checks on the host ----------------------------------------------------------------------------------------------------------
def test_argument_checks_reject_on_the_host(L):
    lib = L.load()
    before = L.query("arco_conv_last_route")                                                       # (0 on a machine without a GPU)
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(**kw):
        a = dict(inp=p, ld_in=16, K=16, Wp=p, N=16, out=p, ld_out=16, bias=None, res=None, ld_res=0, s1=None, s2=None, taps=9, NV=2, D3=1, H=4,
                 W=4, groups=1, mma=0)
        a.update(kw)
        return lib.arco_conv3d_fwd(a["inp"], a["ld_in"], a["K"], a["Wp"], a["N"], a["out"], a["ld_out"], a["bias"], a["res"], a["ld_res"], a["s1"],
                                   a["s2"], a["taps"], a["NV"], a["D3"], a["H"], a["W"], a["groups"], a["mma"], None)

    for bad in (dict(inp=None), dict(Wp=None), dict(out=None), dict(K=0), dict(N=0), dict(NV=0), dict(H=0), dict(W=0), dict(D3=0), dict(mma=5),
                dict(mma=-1), dict(NV=3, groups=2)):
        assert fwd(**bad) == R.ERR_ARG, bad
    assert lib.arco_conv_fwd(None, 16, 16, p, 16, p, 16, None, None, 0, None, None, 9, 1, 4, 4, None) == R.ERR_ARG
    for taps, mode in ((9, 6), (9, 7), (9, -1), (5, 0), (9, 8)):
        assert lib.arco_pack_conv_weight(p, 4, 4, taps, mode, p, None) == R.ERR_ARG, (taps, mode)
    assert lib.arco_pack_conv_weight(p, 0, 4, 9, 0, p, None) == R.ERR_ARG
    assert lib.arco_gemm_splitk(p, 16, 16, p, 16, p, 18, 4, 2, p, None) == R.ERR_ARG             # ld_out % 4
    assert lib.arco_gemm_splitk(p, 16, 16, p, 16, p, 16, 4, 0, p, None) == R.ERR_ARG             # splits < 1
    assert lib.arco_gemm_splitk(p, 16, 16, p, 16, p, 16, 4, 2, None, None) == R.ERR_ARG          # no workspace
    assert lib.arco_gemm_batched(p, 16, 16, p, 16, p, 16, 4, 0, 64, 256, 64, 1, None, None) == R.ERR_ARG      # batch < 1
    assert lib.arco_gemm_batched(p, 16, 16, p, 16, p, 16, 4, 2, 64, 256, 64, 2, None, None) == R.ERR_ARG      # splits > 1 without ws
    assert lib.arco_gemm_batched(p, 16, 16, p, 16, p, 16, 4, 2, 64, 256, 66, 2, p, None) == R.ERR_ARG         # stride_out % 4 with splits
    assert lib.arco_conv1x1_upres_fwd(p, 32, 32, p, 64, p, 64, None, 64, 1, 2, 2, 2, 4, 4, 4, None) == R.ERR_ARG
    assert lib.arco_conv1x1_upres_fwd(p, 32, 32, p, 64, p, 64, p, 64, 1, 0, 2, 2, 4, 4, 4, None) == R.ERR_ARG
    assert L.query("arco_conv_last_route") == before                                               # a rejected call notes no route
    assert fwd(taps=5) == R.ERR_UNSUPPORTED and L.query("arco_conv_last_route") == 0               # a launch that finds no kernel: no route
    lib.arco_conv_fwd(None, 16, 16, p, 16, p, 16, None, None, 0, None, None, 9, 1, 4, 4, None)
    assert L.query("arco_conv_last_route") == 0
