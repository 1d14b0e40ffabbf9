"""The BatchNorm / GroupNorm kernel family of csrc/elementwise.hip called DIRECTLY (arco_amd._lib), one entry point per test, against
a plain float64 reference on the CPU computed from the same input values (tests/norm_kernel_refs.py) - not through ops.py, a torch
module or the fp32 sibling.  Kernel inputs that are results of other kernels (slabs, mean / istd) are GIVEN by the host in the
single-kernel tests; the chain tests at the end tie the kernels together.  Every output buffer is prefilled with a sentinel: pad
columns of a padded stride, the columns around a channel-slice operand and GUARD elements behind the buffer must keep it.  Every
toleranced test prints its worst err / bound and asserts <= 1; the exact kind is compared bit for bit.

Worst err / bound per kernel (u = 2^-24; derivations in tests/norm_kernel_refs.py), CPU emulation | MI355X.  The emulation's figures
are the largest printed by tests/test_norm_kernels_cpu.py, the GPU's the largest printed by this file on an MI355X; both are measured
against the float64 reference.
  * arco_chan_stats(_h)      slabs of sum x 0.40 | 0.40 (f16 0.36)     slabs of sum x^2 0.51 | 0.51 (f16 0.47)     exact kind: bit for bit
  * arco_bn_finalize         mean 0.98 | 0.98   istd 0.98 | 0.98   running_mean 0.70 | 0.63   running_var 0.67 | 0.67
                             deferred mean / variance - | 0.98 / 0.96
  * arco_bn_apply_deferred   exact layer bit for bit; wide layer 0.00 (the sequential update with a rounding per step, reproduced)
  * arco_bn_act_fwd          0.99 | 0.98   _h 1.00 | 1.00   arco_bn_act_add_fwd(_h) 1.00 | 0.99 (1.00)   dropout 0.99 | 0.58 (_h 0.99)
                             large grid - | 0.79 (_h 1.00)   arco_bn_act_pool_fwd A - | 0.89, P and the tie to arco_bn_act_fwd bit for bit
  * arco_bn_act_d2s_fwd(_h)  - | 0.95 (0.99)     arco_bn_act_d2s_bwd(_h)  dY - | 0.23 (1.00)  slabs 0.22  sums 0.17  dgamma 0.20
  * arco_bn_act_bwd(_h)      slabs dy 0.34 | 0.34   slabs dy xh 0.26 | 0.26   sums 0.17 | 0.17   dgamma 0.15 | 0.15   dbeta 0.10 | 0.10
                             dZ 1.00 | 0.98 (_h 1.00)   activation only 0.98 | 0.87   dropout dZ 0.98 | 0.14 (_h 0.98)
                             large grid - | dZ 0.22 (_h 1.00)  slabs 0.11  sums 0.001
  * arco_gn_finalize         mean 0.98 | 0.98   istd 0.91 | 0.91
  * arco_gn_act_bwd          sums 0.13 | 0.13   dgamma 0.26 | 0.22   dbeta 0.20 | 0.20   dZ 0.20 | 0.17   accumulate (one more rounding) 0.91
  * GroupNorm chain          mean 0.10 | 0.10   istd 0.19 | 0.19   forward 0.56 | 0.56   dZ 0.23 | 0.18   dgamma 0.15 | 0.15   dbeta 0.22 | 0.22
  * BatchNorm chain, wide    mean 0.03 | 0.03   istd 0.15 | 0.15   forward 0.99 | 0.99   dZ 0.99 | 0.99 (both f16)   dgamma 0.03   dbeta 0.05
  * BatchNorm chain, offset  mean 0.09 | 0.09   istd 0.66 | 0.66   forward 0.61 | 0.61   dZ 0.93 | 0.93   running_mean - | 0.39
A figure of 0.98 - 1.00 is ONE rounding measured against its own bound: the fp32 rounding of mean / istd against u |ref|, or the f16
store against 2^-11 |ref| (every _h figure near 1).  The offset chain (mean / std = 100, conditioning E[x^2] / (var + eps) = 1.08e4)
holds the derived bound: its istd figure of 0.66 is the constant channel, whose variance is exactly 0 through the clamp and whose
istd is the single rounding of 1 / sqrt(eps); the fifteen other channels sit at 0.02 (f16 0.01) of a bound that carries the conditioning
(gamma(t) E[x^2] / (2 (var + eps)), about 2.4e-3 relative at 17 rows per slab), so the fp32 slab partials did not have to be changed.
No kernel or entry point was found wrong; none was changed.

Branches reached
  * the three apply paths of bn_act_fwd_kernel / bn_act_bwd_apply_kernel: hoisted quad (C = 4, 8, 16, 64, 256), generic (C = 12, 20 and
    mean == nullptr), f16 eight-channel (C = 8, 16, 64, 256 with every stride a multiple of 8) and its fall-back to the quad path (a
    stride of C + 4, a column offset of 4): the three f16 variants are anchored to float64 AND bit-equal to one another
  * both forms of block_channel_totals: shuffle tree (C/4 = 1 .. 64), serial LDS loop with 256 % (C/4) == 0 (C = 512, 1024) and with
    the tr < rstep guard (C = 12, 20, 48, 260)
  * in-flight rows u >= 1 and second trips: forward M = 4 x 4096 x 256 + 3 (fp32 C = 4, f16 C = 8), backward M = 2 x 4096 x 256 + 3
  * empty slabs (M = 8193: 512 blocks of 17 rows, the last 30 written as zeros), the 2048-slab cap (M = 2048 x 512 + 777, rpb = 513;
    the large backward), slab_sums2's 8 x 256 body and tail at 1, 255, 256, 257, 2047, 2048, 2049, 2053 slabs
  * groups 1, 2, 3; defer_from 0, 1, groups - 1 and no deferral; the pending flag set, cleared, and left alone
  * drop_mode 1 and 2 with and without seed_dev, with groups = 2 (the group's row offset in the element index); p = 0
  * accumulate 0 / 1 and null dgamma / dbeta; the gn form of the apply pass; both depth-to-space row maps; the skip addition
Not reached
  * six decades of magnitude in the f16 BACKWARD: dZ holds terms of the size xh^2 dy, which leave the f16 range (65504); there Z spans
    10^-3 .. 10^1 and dA 10^-4 .. 10^0 (norm_kernel_refs.bwd_case), every other input spans the six decades
  * C > 1024 (rejected on the host, tests/test_norm_kernels_cpu.py), element indices of the dropout mask past 2^32 (a tensor of
    more than 16 GB), a GroupNorm set of more than 256 channels (rejected on the host)
  * the conv-epilogue producers of the slabs (tests/test_conv_kernels_gpu.py) and the consumer-side activation of the conv loaders
    (tests/test_block_fuse_gpu.py, bit-equal to arco_bn_act_fwd, which this file anchors)"""
import struct

import numpy as np
import pytest
import torch

import norm_kernel_refs as R
from loss_kernel_refs import SENTINEL, U, exact, worst
from side_kernel_refs import GUARD, bits_equal, body, cols
from test_side_kernels_gpu import DEV, dev, filled, put, report

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def stop_on_device_error():
    """a device error ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, nothing more is launched: {e}", returncode=3)


def held(name, got, ref, tol):
    report(name, worst(got, ref, tol))


def dparams(L, prm, nomean=False):
    d = {k: dev(v) for k, v in prm.items()}
    return d, [None if nomean else L.ptr(d["mu"]), None if nomean else L.ptr(d["istd"]), L.ptr(d["ga"]), L.ptr(d["be"])]


def drop_args(drop):
    """-> (drop_mode, p, seed, P, seed_dev tensor or None)"""
    if drop is None:
        return 0, 0.0, 0, 1, None
    mode, p, seed, P, salt = drop
    return mode, p, seed, P, None if salt is None else torch.tensor([salt], dtype=torch.int64, device=DEV)


def dt(half):
    return F16 if half else F32


# ---- (1) arco_chan_stats(_h) ----------------------------------------------------------------------------------------------------------
def run_stats(L, c, half):
    C, M, groups = c["C"], c["M"], c["groups"]
    _, x = put(c["X"].to(dt(half)), c["ld"], c["off"])
    n = C * groups * c["g"]["nblk"]
    sb, qb = filled(n), filled(n)
    L.call("arco_chan_stats_h" if half else "arco_chan_stats", L.ptr(x), c["ld"], groups * M, C, L.ptr(sb), L.ptr(qb), groups)
    shape = (C, groups * c["g"]["nblk"])
    return body(sb, n, shape), body(qb, n, shape)


def check_stats(name, c, s, q):
    if c["kind"] == "exact":
        assert exact(s, c["s"].float()) and exact(q, c["q"].float()), name + ": exact slabs differ"
    held(name + " sum", s, c["s"], c["ts"])
    held(name + " sumsq", q, c["q"], c["tq"])
    nblk, e = c["g"]["nblk"], c["g"]["empty"]
    if e:                                                                     # empty row ranges: exactly 0, not the sentinel
        tail = s.view(c["C"], c["groups"], nblk)[:, :, nblk - e:], q.view(c["C"], c["groups"], nblk)[:, :, nblk - e:]
        assert bool((tail[0] == 0).all()) and bool((tail[1] == 0).all())
    if c["kind"] == "offset":                                                 # the constant channel: exact fp32 slabs
        assert exact(s[-1], c["s"][-1].float()) and exact(q[-1], c["q"][-1].float())


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.STATS_CASES)), ids=lambda i: "-".join(map(str, R.STATS_CASES[i])))
def test_chan_stats(L, i, half):
    c = R.stats_case(i, half)
    s, q = run_stats(L, c, half)
    check_stats(f"chan_stats{'_h' if half else ''} {R.STATS_CASES[i]}", c, s, q)


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
def test_chan_stats_block_cap(L, half):
    """M = 2048 x 512 + 777: the 2048-block cap, 513 rows per block"""
    c = R.stats_case(-1, half)
    assert c["g"]["nblk"] == 2048 and c["g"]["rpb"] == 513
    s, q = run_stats(L, c, half)
    check_stats(f"chan_stats{'_h' if half else ''} block cap", c, s, q)


# ---- (2) arco_bn_finalize on host-written slabs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.FIN_CASES)), ids=lambda i: "-".join(map(str, R.FIN_CASES[i])))
def test_bn_finalize(L, i):
    c = R.fin_case(i)
    C, groups, npg, cnt, mode, f = c["C"], c["groups"], c["npg"], c["cnt"], c["mode"], c["fin"]
    s, q = dev(c["s"]), dev(c["q"])
    mb, ib = filled(groups * C), filled(groups * C)
    running = mode != "none"
    rmb, rvb = filled(C), filled(C)
    rmb[:C], rvb[:C] = dev(c["rm0"]), dev(c["rv0"])
    nbt = filled(1, torch.int64)
    nbt[0] = 41
    df = R.defer_from(mode, groups)
    nd = 0 if df is None else (groups - df) * 2 * C + 1
    db = filled(nd + 3)                                                       # three more sentinels: nothing behind the flag is written
    L.call("arco_bn_finalize", L.ptr(s), L.ptr(q), groups * npg, C, cnt * groups, R.EPS_BN, R.MOM, L.ptr(mb), L.ptr(ib),
           L.ptr(rmb) if running else None, L.ptr(rvb) if running else None, L.ptr(nbt) if running else None, groups,
           0 if df is None else df, None if df is None else L.ptr(db))
    name = f"bn_finalize {R.FIN_CASES[i]}"
    held(name + " mean", body(mb, groups * C, (groups, C)), f["m"], f["tm"])
    istd = body(ib, groups * C, (groups, C))
    held(name + " istd", istd, f["istd"], f["ti"])
    if C >= 3:                                                                # var = -m^2 < 0: the clamp
        assert exact(istd[:, -1], torch.full((groups,), float(np.float32(1.0 / np.sqrt(R.EPS_BN)))))
    rm, rv, tm, tv = R.running_ref(c["rm0"], c["rv0"], f, groups, upto=df)
    got_rm, got_rv = body(rmb, C), body(rvb, C)
    if running:
        held(name + " running_mean", got_rm, rm, tm)
        held(name + " running_var", got_rv, rv, tv)
        assert int(body(nbt, 1)[0]) == 41 + groups
        if df == 0:
            assert exact(got_rm, c["rm0"]) and exact(got_rv, c["rv0"])
    else:
        assert exact(got_rm, c["rm0"]) and exact(got_rv, c["rv0"]) and int(body(nbt, 1)[0]) == 41
    d = body(db, nd + 3)
    assert bool((d[nd:] == SENTINEL).all())
    if df is not None:
        terms = d[:nd - 1].view(groups - df, 2, C)
        held(name + " deferred mean", terms[:, 0], f["m"][df:], f["tm"][df:])
        held(name + " deferred var", terms[:, 1], f["unb"][df:], f["dunb"][df:] + U * (f["unb"][df:] + f["dunb"][df:]))
        assert float(d[nd - 1]) == 1.0


# ---- (3) arco_bn_apply_deferred -------------------------------------------------------------------------------------------------------------
def test_bn_apply_deferred(L):
    assert L.query("arco_bn_defer_desc_bytes") == struct.calcsize(R.DEFER_FMT)
    g = R.gen(61)
    layers = []                                                               # (n, C, momentum, pending, kind)
    for n, C, mom, pending, kind in ((1, 5, 0.5, True, "exact"), (3, 300, R.MOM, True, "wide"), (2, 7, R.MOM, False, "wide")):
        terms = R.values(g, n * 2, C, kind).view(n, 2, C)
        rm0, rv0 = R.values(g, 1, C, kind)[0], R.values(g, 1, C, kind)[0].abs()
        rmb, rvb, db = filled(C), filled(C), filled(n * 2 * C + 1)
        rmb[:C], rvb[:C], db[:n * 2 * C] = dev(rm0), dev(rv0), dev(terms.reshape(-1))
        db[n * 2 * C] = 1.0 if pending else 0.0
        layers.append(dict(n=n, C=C, mom=mom, pending=pending, kind=kind, terms=terms, rm0=rm0, rv0=rv0, rmb=rmb, rvb=rvb, db=db))
    raw = b"".join(struct.pack(R.DEFER_FMT, l["rmb"].data_ptr(), l["rvb"].data_ptr(), l["db"].data_ptr(), l["C"], l["n"], l["mom"], 0)
                   for l in layers)
    desc = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    L.call("arco_bn_apply_deferred", None, 0)                                  # no layers: OK without a launch
    for call in range(2):
        L.call("arco_bn_apply_deferred", L.ptr(desc), len(layers))
        for k, l in enumerate(layers):
            n, C = l["n"], l["C"]
            got_rm, got_rv, d = body(l["rmb"], C), body(l["rvb"], C), body(l["db"], n * 2 * C + 1)
            assert exact(d[:-1], l["terms"].reshape(-1)) and float(d[-1]) == 0.0          # terms kept, flag cleared (or never set)
            if not l["pending"]:
                assert bits_equal(got_rm, l["rm0"]) and bits_equal(got_rv, l["rv0"])
                continue
            rm, rv, tm, tv = R.deferred_ref(l["rm0"], l["rv0"], l["terms"], float(np.float32(l["mom"])))
            if l["kind"] == "exact":
                assert exact(got_rm, rm) and exact(got_rv, rv)
            held(f"bn_apply_deferred layer {k} call {call} running_mean", got_rm, rm.double(), tm)
            held(f"bn_apply_deferred layer {k} call {call} running_var", got_rv, rv.double(), tv)


# ---- (4), (5) arco_bn_act_fwd(_h), arco_bn_act_add_fwd(_h) ------------------------------------------------------------------------------------
def run_fwd(L, c, layout, p0=False):
    """layout = (pad of Z, offset of Z, pad of A, offset of A); R (the add form) takes Z's layout in a buffer of its own.  p0: the
    dropout arguments with p = 0"""
    pz, oz, pa, oa = layout
    C, groups, half = c["C"], c["groups"], c["half"]
    rows = groups * c["M"]
    ldz, lda = C + pz, C + pa
    _, z = put(c["Z"].to(dt(half)), ldz, oz)
    ab = filled(rows * lda, dt(half))
    d, pp = dparams(L, c["prm"], c["nomean"])
    h = "_h" if half else ""
    if c["R"] is not None:
        _, r = put(c["R"].to(dt(half)), ldz, oz)
        L.call("arco_bn_act_add_fwd" + h, L.ptr(z), ldz, rows, C, *pp, c["slope"], L.ptr(r), ldz, L.ptr(ab[oa:]), lda, groups)
    else:
        mode, p, seed, P, sd = drop_args((1, 0.0, 5, 1, None) if p0 else c["drop"])
        L.call("arco_bn_act_fwd" + h, L.ptr(z), ldz, rows, C, *pp, c["slope"], mode, p, seed, P, L.ptr(ab[oa:]), lda, L.ptr(sd), groups)
    got, ok = cols(ab, rows, lda, oa, C)
    assert ok, "a pad column or a column around the slice was written"
    return got


def check_fwd(name, c, got):
    held(name, got, c["ref"], c["tol"])
    if c["bit_exact"]:
        assert exact(got, c["ref"].to(got.dtype)), name + ": the exact kind differs"
    if c["keep"] is not None:
        assert exact(got == 0, ~c["keep"]), name + ": the zeroed elements are not the restated mask"


def fwd_id(i):
    return "-".join(map(str, R.FWD_CASES[i]))


@pytest.mark.parametrize("with_r", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("i", range(len(R.FWD_CASES)), ids=fwd_id)
def test_bn_act_fwd(L, i, with_r):
    C, M, groups, kind, slope, nomean = R.FWD_CASES[i]
    c = R.fwd_case(C, M, groups, kind, slope, nomean, False, None, with_r)
    for layout in R.LAYOUTS:
        got = run_fwd(L, c, layout)
        check_fwd(f"bn_act{'_add' if with_r else ''}_fwd {R.FWD_CASES[i]} layout {layout}", c, got)
    if not with_r:                                                            # p = 0 with drop_mode = 1: the no-dropout result, bit for bit
        assert bits_equal(run_fwd(L, c, R.LAYOUTS[0], p0=True), got)


@pytest.mark.parametrize("with_r", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("i", range(len(R.FWD_CASES)), ids=fwd_id)
def test_bn_act_fwd_h(L, i, with_r):
    """the three alignment variants: each against float64, and bit-equal to one another"""
    C, M, groups, kind, slope, nomean = R.FWD_CASES[i]
    c = R.fwd_case(C, M, groups, kind, slope, nomean, True, None, with_r)
    outs = []
    for layout in R.H_VARIANTS:
        outs.append(run_fwd(L, c, layout))
        check_fwd(f"bn_act{'_add' if with_r else ''}_fwd_h {R.FWD_CASES[i]} variant {layout}", c, outs[-1])
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("kind", ("exact", "wide"))
def test_bn_act_fwd_large_grid(L, kind, half):
    """all four in-flight rows, a second trip of the loop, a ragged end: M = 4 x 4096 x 256 + 3 at C = 4 (fp32) / C = 8 (f16)"""
    C, M = (8 if half else 4), R.FWD_BIG_M
    g = R.gen(71, int(half))
    Z = R.values(g, M, C, kind, half)
    prm = R.params(g, 1, C, kind)
    if kind == "wide":
        Z, moved = R.settle(Z, prm, 1, half)
        print(f"  moved away from zero: {moved}")
    z = Z.to(dt(half)).to(DEV)
    ab = filled(M * C, dt(half))
    d, pp = dparams(L, prm)
    L.call("arco_bn_act_fwd" + ("_h" if half else ""), L.ptr(z), C, M, C, *pp, 0.25, 0, 0.0, 0, 1, L.ptr(ab), C, None, 1)
    got = body(ab, M * C, (M, C))
    del z, ab
    worst_ratio = 0.0
    for r0 in range(0, M, 1 << 20):                                           # the reference in row blocks: a few tens of MB at a time
        sl = slice(r0, min(M, r0 + (1 << 20)))
        a, b, _ = R.fwd_ref(Z[sl], prm, 0.25, 1, None, None, half)
        worst_ratio = max(worst_ratio, worst(got[sl], a, b))
        if kind == "exact" and not half:
            assert exact(got[sl], a.float())
    report(f"bn_act_fwd{'_h' if half else ''} large grid {kind}", worst_ratio)


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.DROP_CASES)), ids=lambda i: "-".join(map(str, R.DROP_CASES[i])))
def test_bn_act_fwd_dropout(L, i, half):
    C, img, groups, kind, mode, p, salt = R.DROP_CASES[i]
    c = R.fwd_case(C, img * R.P_ROWS, groups, kind, 0.25, False, half, R.drop_of(R.DROP_CASES[i]))
    for layout in (R.H_VARIANTS if half else R.LAYOUTS)[::2]:
        check_fwd(f"bn_act_fwd{'_h' if half else ''} dropout {R.DROP_CASES[i]} layout {layout}", c, run_fwd(L, c, layout))


# ---- (7) arco_bn_act_bwd(_h) ------------------------------------------------------------------------------------------------------------------
def run_bwd(L, c, layout, accumulate=0, null_grads=False, gn=False):
    """layout = (pad of dA and Z, their offset, pad of dZ, its offset).  -> dict of everything the call wrote"""
    pz, oz, po, oo = layout
    C, groups, half, cpg = c["C"], c["groups"], c["half"], c["cpg"]
    rows = groups * c["M"]
    ldz, ldo = C + pz, C + po
    _, z = put(c["Z"].to(dt(half)), ldz, oz)
    _, da = put(c["dA"].to(dt(half)), ldz, oz)
    ob = filled(rows * ldo, dt(half))
    d, pp = dparams(L, c["prm"], c["nomean"])
    nblk = R.chan_blocks(c["M"])
    nws = groups * (2 * C * nblk + 2 * C)
    ws, gb, bb = filled(nws), filled(C), filled(C)
    g0 = b0 = None
    if accumulate:
        g0, b0 = R.values(R.gen(83, C), 1, C, "wide")[0], R.values(R.gen(84, C), 1, C, "wide")[0]
        gb[:C], bb[:C] = dev(g0), dev(b0)
    pg, pb = (None, None) if null_grads else (L.ptr(gb), L.ptr(bb))
    if gn:
        L.call("arco_gn_act_bwd", L.ptr(da), ldz, L.ptr(z), ldz, rows, C, *pp, c["slope"], L.ptr(ws), pg, pb, accumulate, L.ptr(ob[oo:]),
               ldo, groups, cpg)
    else:
        mode, p, seed, P, sd = drop_args(c["drop"])
        L.call("arco_bn_act_bwd" + ("_h" if half else ""), L.ptr(da), ldz, L.ptr(z), ldz, rows, C, *pp, c["slope"], mode, p, seed, P,
               L.ptr(ws), pg, pb, accumulate, L.ptr(ob[oo:]), ldo, L.ptr(sd), groups)
    dz, ok = cols(ob, rows, ldo, oo, C)
    assert ok, "a pad column or a column around the slice was written"
    w = body(ws, nws)
    n = groups * C * nblk
    return dict(dz=dz, slab_s=w[:n].view(groups, C, nblk), slab_q=w[n:2 * n].view(groups, C, nblk), sums=w[2 * n:].view(groups, 2, C),
                dgamma=body(gb, C), dbeta=body(bb, C), g0=g0, b0=b0, ws=w)


def check_bwd(name, c, o, accumulate=0, null_grads=False):
    if c["nomean"]:
        held(name + " dz", o["dz"], c["dz"], c["tz"])
        if c["kind"] == "exact" and (not c["half"] or c["slope"] != 0.01):
            assert exact(o["dz"], c["dz"].to(o["dz"].dtype))
        # no statistics, no parameter gradients: the workspace and dgamma / dbeta keep what they held
        keep_g, keep_b = (o["g0"], o["b0"]) if accumulate else (torch.full_like(o["dgamma"], SENTINEL),) * 2
        assert bool((o["ws"] == SENTINEL).all()) and bits_equal(o["dgamma"], keep_g) and bits_equal(o["dbeta"], keep_b)
        return
    held(name + " slabs dy", o["slab_s"], c["slab_s"], c["tslab_s"])
    held(name + " slabs dy*xh", o["slab_q"], c["slab_q"], c["tslab_q"])
    if c["kind"] == "exact" and c["slope"] != 0.01 and c["drop"] is None and not c["cpg"]:
        assert exact(o["slab_s"], c["slab_s"].float()) and exact(o["slab_q"], c["slab_q"].float())
    held(name + " sums", o["sums"], c["sums"], c["tsums"])
    held(name + " dz", o["dz"], c["dz"], c["tz"])
    if null_grads:
        assert bool((o["dgamma"] == SENTINEL).all()) and bool((o["dbeta"] == SENTINEL).all())
    elif accumulate:
        rg, rb = c["dgamma"] + o["g0"].double(), c["dbeta"] + o["b0"].double()
        held(name + " dgamma (accumulate)", o["dgamma"], rg, c["tg"] + U * (rg.abs() + c["tg"]))
        held(name + " dbeta (accumulate)", o["dbeta"], rb, c["tb"] + U * (rb.abs() + c["tb"]))
    else:
        held(name + " dgamma", o["dgamma"], c["dgamma"], c["tg"])
        held(name + " dbeta", o["dbeta"], c["dbeta"], c["tb"])


@pytest.mark.parametrize("i", range(len(R.FWD_CASES)), ids=fwd_id)
def test_bn_act_bwd(L, i):
    C, M, groups, kind, slope, nomean = R.FWD_CASES[i]
    c = R.bwd_case(C, M, groups, kind, slope, nomean)
    for k, layout in enumerate(R.LAYOUTS):
        o = run_bwd(L, c, layout, accumulate=int(k == 1), null_grads=k == 2)
        check_bwd(f"bn_act_bwd {R.FWD_CASES[i]} layout {layout}", c, o, int(k == 1), k == 2)


@pytest.mark.parametrize("i", range(len(R.FWD_CASES)), ids=fwd_id)
def test_bn_act_bwd_h(L, i):
    C, M, groups, kind, slope, nomean = R.FWD_CASES[i]
    c = R.bwd_case(C, M, groups, kind, slope, nomean, True)
    outs = []
    for k, layout in enumerate(R.H_VARIANTS):
        o = run_bwd(L, c, layout, accumulate=int(k == 1), null_grads=k == 2)
        check_bwd(f"bn_act_bwd_h {R.FWD_CASES[i]} variant {layout}", c, o, int(k == 1), k == 2)
        outs.append(o["dz"].view(torch.int16))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.DROP_CASES)), ids=lambda i: "-".join(map(str, R.DROP_CASES[i])))
def test_bn_act_bwd_dropout(L, i, half):
    """the mask must be the forward's: both are run, and both zero sets are the restated mask"""
    C, img, groups, kind, mode, p, salt = R.DROP_CASES[i]
    drop = R.drop_of(R.DROP_CASES[i])
    M = img * R.P_ROWS
    f = R.fwd_case(C, M, groups, kind, 0.25, False, half, drop)
    c = R.bwd_case(C, M, groups, kind, 0.25, False, half, drop)
    assert exact(f["keep"], c["keep"])
    layout = (R.H_VARIANTS if half else R.LAYOUTS)[0]
    a = run_fwd(L, f, layout)
    o = run_bwd(L, c, layout)
    check_bwd(f"bn_act_bwd{'_h' if half else ''} dropout {R.DROP_CASES[i]}", c, o)
    assert exact(a == 0, ~c["keep"])
    # dz of a dropped element is the mean part alone; its dy is zero: the slabs, held above, are sums over the kept elements only
    dy_zero = (c["dA"] != 0) & ~c["keep"]
    assert bool(dy_zero.any())


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
def test_bn_act_bwd_large_grid(L, half):
    """M = 2 x 4096 x 256 + 3 at C = 4 (fp32) / C = 8 (f16): both in-flight rows and a second trip of the apply loop, and the 2048-slab
    cap of the reduce"""
    C, M = (8 if half else 4), R.BWD_BIG_M
    c = R.bwd_case(C, M, 1, "wide", 0.25, False, half)
    assert c["geo"]["nblk"] == 2048
    print(f"  moved away from zero: {c['moved']}")
    o = run_bwd(L, c, (0, 0, 0, 0))
    check_bwd(f"bn_act_bwd{'_h' if half else ''} large grid", c, o)
    R.bwd_case.cache_clear()


# ---- (6) depth-to-space forms -------------------------------------------------------------------------------------------------------------------
def d2s_id(i):
    return "-".join(map(str, R.D2S_CASES[i])).replace(" ", "")


def d2s_inputs(i, half, kind):
    grid, groups, C, with_r = R.D2S_CASES[i]
    M8 = 8 * grid[0] * grid[1] * grid[2] * grid[3]
    g = R.gen(91, i, int(half))
    Y = R.values(g, M8, C, kind, half, (-3, 1) if half else (-3, 3))
    prm = R.params(g, groups, C, kind)
    if kind != "exact":
        Y, _ = R.settle(Y, prm, groups, half)
    Rr = R.values(g, M8, C, kind, half) if with_r else None
    return grid, groups, C, M8, Y, prm, Rr, g


@pytest.mark.parametrize("kind", ("exact", "wide"))
@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.D2S_CASES)), ids=d2s_id)
def test_bn_act_d2s_fwd(L, i, half, kind):
    grid, groups, C, M8, Y, prm, Rr, _ = d2s_inputs(i, half, kind)
    slope = 0.25
    a, b, _ = R.fwd_ref(Y, prm, slope, groups)                                # rows in (voxel, tap) order
    a, b = R.d2s(a, grid, C), R.d2s(b, grid, C)                               # ... permuted to the voxels of the activation
    if Rr is not None:
        a = a + Rr.double()
        b = b + U * a.abs()
    if half:
        b = b + R.H_REL * (a.abs() + b) + R.H_ABS
    pad, off = 8, (0 if half else 4)
    y = Y.to(dt(half)).to(DEV)
    lda = C + pad
    ab = filled(M8 * lda, dt(half))
    r = (None, None) if Rr is None else put(Rr.to(dt(half)), lda, off)
    d, pp = dparams(L, prm)
    L.call("arco_bn_act_d2s_fwd" + ("_h" if half else ""), L.ptr(y), M8, C, *pp, slope, L.ptr(r[1]), lda if Rr is not None else 0,
           L.ptr(ab[off:]), lda, grid[1], grid[2], grid[3], groups)
    got, ok = cols(ab, M8, lda, off, C)
    assert ok
    name = f"bn_act_d2s_fwd{'_h' if half else ''} {R.D2S_CASES[i]} {kind}"
    held(name, got, a, b)
    if kind == "exact" and R.fwd_roundings(slope, None, Rr, half) <= 1:      # the permutation, bit for bit
        assert exact(got, a.to(got.dtype))


@pytest.mark.parametrize("kind", ("exact", "wide"))
@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", [k for k in range(len(R.D2S_CASES)) if not R.D2S_CASES[k][3]], ids=d2s_id)
def test_bn_act_d2s_bwd(L, i, half, kind):
    """dA in the activation's voxel order (a channel slice), dY returned dense in (voxel, tap) order"""
    grid, groups, C, M8, Y, prm, _, g = d2s_inputs(i, half, kind)
    slope = 0.25
    dA = R.values(g, M8, C, kind, half, (-4, 0) if half else (-3, 3))         # voxel order
    ref = R.bwd_ref(R.s2d(dA, grid, C), Y, prm, slope, groups, None, half)
    c = dict(ref, kind=kind, slope=slope, drop=None, cpg=0, nomean=False, half=half)
    ldd, off = C + 8, (0 if half else 4)
    _, da = put(dA.to(dt(half)), ldd, off)
    y = Y.to(dt(half)).to(DEV)
    nblk = R.chan_blocks(M8 // groups)
    nws = groups * (2 * C * nblk + 2 * C)
    ws, gb, bb, ob = filled(nws), filled(C), filled(C), filled(M8 * C, dt(half))
    d, pp = dparams(L, prm)
    L.call("arco_bn_act_d2s_bwd" + ("_h" if half else ""), L.ptr(da), ldd, L.ptr(y), M8, C, *pp, slope, L.ptr(ws), L.ptr(gb), L.ptr(bb), 0,
           L.ptr(ob), grid[1], grid[2], grid[3], groups)
    w = body(ws, nws)
    n = groups * C * nblk
    o = dict(dz=body(ob, M8 * C, (M8, C)), slab_s=w[:n].view(groups, C, nblk), slab_q=w[n:2 * n].view(groups, C, nblk),
             sums=w[2 * n:].view(groups, 2, C), dgamma=body(gb, C), dbeta=body(bb, C), ws=w)
    check_bwd(f"bn_act_d2s_bwd{'_h' if half else ''} {R.D2S_CASES[i]} {kind}", c, o)
    if kind == "exact":                                                       # the row map alone: a wrong tap moves exact slab values
        assert exact(o["slab_s"], c["slab_s"].float())


# ---- (8) arco_gn_finalize, arco_gn_act_bwd ---------------------------------------------------------------------------------------------------------
def gn_id(i):
    return "-".join(map(str, R.GN_CASES[i]))


@pytest.mark.parametrize("i", range(len(R.GN_CASES)), ids=gn_id)
def test_gn_finalize(L, i):
    """alone, on host-written slabs: mean / istd rows [N][C] hold the set's value in each of its channels"""
    C, cpg, N, V = R.GN_CASES[i]
    npg = R.chan_blocks(V)
    s, q = R.fin_slabs(R.gen(41, i), C, N, npg, V)
    q = q + 1.0
    f = R.gn_finalize_ref(s, q, C, cpg, N, V)
    mb, ib = filled(N * C), filled(N * C)
    sd, qd = dev(s), dev(q)
    L.call("arco_gn_finalize", L.ptr(sd), L.ptr(qd), N * npg, C, cpg, N, V, R.EPS_BN, L.ptr(mb), L.ptr(ib))
    m, istd = body(mb, N * C, (N, C)), body(ib, N * C, (N, C))
    held(f"gn_finalize {R.GN_CASES[i]} mean", m, f["m"], f["tm"])
    held(f"gn_finalize {R.GN_CASES[i]} istd", istd, f["istd"], f["ti"])
    sets = m.view(N, C // cpg, cpg), istd.view(N, C // cpg, cpg)
    assert bool((sets[0] == sets[0][:, :, :1]).all()) and bool((sets[1] == sets[1][:, :, :1]).all())


@pytest.mark.parametrize("i", range(len(R.GN_CASES)), ids=gn_id)
def test_gn_act_bwd(L, i):
    """alone, on given mean / istd: the merged sums are written back into every channel of the set"""
    C, cpg, N, V = R.GN_CASES[i]
    c = R.bwd_case(C, V, N, "wide", 0.01, False, False, None, cpg)
    for k, layout in enumerate(R.LAYOUTS[:2]):
        o = run_bwd(L, c, layout, accumulate=k, gn=True)
        check_bwd(f"gn_act_bwd {R.GN_CASES[i]} layout {layout}", c, o, k)
        sets = o["sums"].reshape(N * 2, C // cpg, cpg)
        assert bool((sets == sets[:, :, :1]).all())


@pytest.mark.parametrize("i", [k for k in range(len(R.GN_CASES)) if R.GN_CASES[k][3] * R.GN_CASES[k][1] > 1], ids=gn_id)
def test_gn_chain(L, i):
    """arco_chan_stats(groups = N) -> arco_gn_finalize -> arco_bn_act_fwd(groups = N) -> arco_gn_act_bwd against float64 F.group_norm +
    LeakyReLU and its autograd.  (Sets of ONE element - InstanceNorm of a single voxel - are left to the two tests above: their
    variance is 0 and the normalised value does not depend on the data.)"""
    C, cpg, N, V = R.GN_CASES[i]
    slope = 0.01
    X, dA, ga, be, moved = R.chain_inputs(7, C, V, N, "wide", slope, False, cpg)
    ch = R.chain_ref(X, dA, ga, be, slope, N, cpg)
    print(f"  moved away from zero: {moved}; conditioning {ch['cond_live']:.3g}")
    run_chain(L, f"gn chain {R.GN_CASES[i]}", ch, X, dA, ga, be, slope, N, cpg, False)


# ---- (9) arco_bn_act_pool_fwd ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("exact", "wide"))
@pytest.mark.parametrize("i", range(len(R.POOL_CASES)), ids=lambda i: "-".join(map(str, R.POOL_CASES[i])))
def test_bn_act_pool_fwd(L, i, kind):
    NB, groups, H, W, C = R.POOL_CASES[i]
    M = NB // groups * H * W
    rows, prow = groups * M, NB * (H // 2) * (W // 2)
    c = R.fwd_case(C, M, groups, kind, 0.01, False, False, None, False, seed=97)
    ldz, oz, lda, oa, ldp, op = C + 8, 4, C + 4, 0, C + 16, 8
    _, z = put(c["Z"], ldz, oz)
    ab, pb = filled(rows * lda), filled(prow * ldp)
    d, pp = dparams(L, c["prm"])
    L.call("arco_bn_act_pool_fwd", L.ptr(z), ldz, NB, H, W, C, *pp, 0.01, L.ptr(ab[oa:]), lda, L.ptr(pb[op:]), ldp, groups)
    A, ok_a = cols(ab, rows, lda, oa, C)
    P, ok_p = cols(pb, prow, ldp, op, C)
    assert ok_a and ok_p
    check_fwd(f"bn_act_pool_fwd {R.POOL_CASES[i]} {kind} A", c, A)
    assert bits_equal(P.contiguous(), R.pool2(A.contiguous(), NB, H, W, C)), "P is not the 2 x 2 maximum of the A that was returned"
    assert bits_equal(A.contiguous(), run_fwd(L, c, (8, 4, 4, 0)).contiguous()), "A differs from arco_bn_act_fwd of the same inputs"


# ---- (10) chains --------------------------------------------------------------------------------------------------------------------------------------
def run_chain(L, name, ch, X, dA, ga, be, slope, groups, cpg, half, running=None):
    rows, C = X.shape
    M = rows // groups
    h = "_h" if half else ""
    x, da = X.to(dt(half)).to(DEV), dA.to(dt(half)).to(DEV)
    nblk = R.chan_blocks(M)
    n = C * groups * nblk
    sb, qb = filled(n), filled(n)
    L.call("arco_chan_stats" + h, L.ptr(x), C, rows, C, L.ptr(sb), L.ptr(qb), groups)
    mb, ib = filled(groups * C), filled(groups * C)
    if cpg:
        L.call("arco_gn_finalize", L.ptr(sb), L.ptr(qb), groups * nblk, C, cpg, groups, M, R.EPS_BN, L.ptr(mb), L.ptr(ib))
    else:
        rmb, rvb, nbt = running
        L.call("arco_bn_finalize", L.ptr(sb), L.ptr(qb), groups * nblk, C, rows, R.EPS_BN, R.MOM, L.ptr(mb), L.ptr(ib), L.ptr(rmb), L.ptr(rvb),
               L.ptr(nbt), groups, 0, None)
    f = ch["fin"]
    m, istd = body(mb, groups * C, (groups, C)), body(ib, groups * C, (groups, C))
    live = slice(None)
    held(name + " mean", m, f["m"], f["tm"])
    held(name + " istd", istd[:, live], f["istd"][:, live], f["ti"][:, live])
    gd, bd = dev(ga), dev(be)
    ab, zb = filled(rows * C, dt(half)), filled(rows * C, dt(half))
    L.call("arco_bn_act_fwd" + h, L.ptr(x), C, rows, C, L.ptr(mb), L.ptr(ib), L.ptr(gd), L.ptr(bd), slope, 0, 0.0, 0, 1, L.ptr(ab), C, None, groups)
    a = body(ab, rows * C, (rows, C))
    held(name + " forward", a[:, live], ch["a"][:, live], ch["ta"][:, live])
    nws = groups * (2 * C * nblk + 2 * C)
    ws, gb, bb = filled(nws), filled(C), filled(C)
    if cpg:
        L.call("arco_gn_act_bwd", L.ptr(da), C, L.ptr(x), C, rows, C, L.ptr(mb), L.ptr(ib), L.ptr(gd), L.ptr(bd), slope, L.ptr(ws), L.ptr(gb),
               L.ptr(bb), 0, L.ptr(zb), C, groups, cpg)
    else:
        L.call("arco_bn_act_bwd" + h, L.ptr(da), C, L.ptr(x), C, rows, C, L.ptr(mb), L.ptr(ib), L.ptr(gd), L.ptr(bd), slope, 0, 0.0, 0, 1,
               L.ptr(ws), L.ptr(gb), L.ptr(bb), 0, L.ptr(zb), C, None, groups)
    body(ws, nws)
    dz = body(zb, rows * C, (rows, C))
    held(name + " dz", dz[:, live], ch["dz"][:, live], ch["tz"][:, live])
    held(name + " dgamma", body(gb, C)[live], ch["dgamma"][live], ch["tg"][live])
    held(name + " dbeta", body(bb, C), ch["dbeta"], ch["tb"])
    return m, istd, a, dz


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("kind", ("wide", "offset"))
def test_bn_chain(L, kind, half):
    """arco_chan_stats -> arco_bn_finalize -> arco_bn_act_fwd -> arco_bn_act_bwd, two independent batches (groups = 2), against float64
    F.batch_norm(training = True) + LeakyReLU and its autograd; running statistics updated in group order"""
    C, M, groups, slope = R.CHAIN_C, R.CHAIN_M, R.CHAIN_G, 0.01
    X, dA, ga, be, moved = R.chain_inputs(5, C, M, groups, kind, slope, half)
    ch = R.chain_ref(X, dA, ga, be, slope, groups, 0, half)
    print(f"  moved away from zero: {moved}; conditioning E[x^2] / (var + eps) {ch['cond_live']:.3g}")
    g = R.gen(101)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rmb, rvb, nbt = filled(C), filled(C), filled(1, torch.int64)
    rmb[:C], rvb[:C], nbt[0] = dev(rm0), dev(rv0), 0
    name = f"bn chain {kind} {'f16' if half else 'f32'}"
    m, istd, a, dz = run_chain(L, name, ch, X, dA, ga, be, slope, groups, 0, half, (rmb, rvb, nbt))
    rm, rv, tm, tv = R.running_ref(rm0, rv0, ch["fin"], groups)
    live = slice(None)
    held(name + " running_mean", body(rmb, C), rm, tm)
    held(name + " running_var", body(rvb, C)[live], rv[live], tv[live])
    assert int(body(nbt, 1)[0]) == groups
    if kind == "offset":
        report(name + " istd without the constant channel", worst(istd[:, :-1], ch["fin"]["istd"][:, :-1], ch["fin"]["ti"][:, :-1]))
        # the constant channel: variance exactly 0 through the clamp, istd == float(1 / sqrt(eps)), activation exactly lrelu(beta)
        assert bool((m[:, -1] == 1.5).all()) and bool((istd[:, -1] == float(np.float32(1.0 / np.sqrt(R.EPS_BN)))).all())
        lb = be[-1] if be[-1] >= 0 else be[-1] * torch.tensor(slope)
        assert bool((a[:, -1] == (lb.half() if half else lb)).all())
        held(name + " running_var of the constant channel", body(rvb, C)[-1:], rv[-1:], 2 * U * rv[-1:].abs())
