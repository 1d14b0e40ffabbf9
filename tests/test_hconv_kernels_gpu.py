"""Every forward and data-gradient route of the f16-storage convolutions (mma 4: csrc/conv_h.hip, and the f16 epilogue of
conv3d_image_kernel<3> in igemm.hip) called DIRECTLY (arco_amd._lib: arco_conv3d_fwd(..., mma = 4) on an arco_pack_conv_weight(mode 4)
pack), one route per test, against a plain float64 F.conv2d / F.conv3d of the same f16 input values (tests/hconv_kernel_refs.py) - not
through ops.py and not against another HIP route.  Every test asserts the kernel that ran through arco_conv_last_route (ids:
include/arco_hip.h; the conv_h.hip launches note theirs).  Every output and statistics buffer is prefilled with a sentinel: the pad
columns of ld_out > N and GUARD elements in front of and behind the buffer must keep it; operands are also passed as channel slices
(ld_in > K at a column offset).  No environment variable is read; the arco_conv3d_fl_set switch is restored in a `finally`.

Kinds of input (hconv_kernel_refs.py): `fixed` (integers times a power of two inside the 2^24 budget; half of the output channels an
identity store, the other half rounded - subnormal outputs, exact ties, 24 significant bits), `impulse` (unit impulses against weights
over the whole f16 range, subnormals and +-65504 included) and `select` (one +-2^e weight per output channel, every tap, against
activations over the whole f16 range, subnormals included) must equal the float64 convolution rounded ONCE to f16, to nearest even, BIT
FOR BIT (torch.equal); `wide` (four decades inside the normal range, 20 % zeros) is held per element to the derived bound
t32 + 2^-11 (|ref| + t32) + 2^-25, t32 = gamma_n(n) S.  BatchNorm partials: on shrunk fixed data every slab is an integer number of
quanta and the float64 host sum of a group's slab range EQUALS that group's sum y and sum y^2 of the ROUNDED f16 outputs (the data make
the unrounded sums differ); on wide data a derived bound.

Routes (taps, id), covered / not covered, and why:
  hconv_kernel<9,..,DEPTH 1> (taps 9)   9128016, 9064016 (element-wise staging, scalar stores), 9256032, 9128032, 9064032 (Npad <= 32 and
         Npad = 64), 9128064, 9064064, 9032032: covered, all eight tiles.
  hconv_kernel<9,..,DEPTH 3> (taps 27, arco_conv3d_fl_set(0))   rectangular 9128016, 9256032, 9128032, 9064032 (both forms), 9128064, 9064064,
         9032032 and flat 9628016, 9628032, 9564032 (both forms), 9628064, 9564064, 9532032: covered; volumes of one plane on one of each.
  hconv_kernel<1,..>   1256016 (also K = 19 / 20 element-wise), 1128032, 1032064, 1064064 (also the case that gets there only through
         stat_groups = 2), 1128128: covered; the grouped GEMM form with M / G no multiple of BM (m_lim) on 1128032 and 1064064.
  hconv_rw_kernel<1,1,8>   9408016: one plane; an odd D3 with S = 2; 1088 units on 1024 slots.  Covered.
  hconv_fc_kernel<A_T,C_T> as the cost model picks it   9261032, 9262032, 9263032, 9261064 at plane widths 7, 12, 24, 45, K 32 / 64 / 128,
         N 32 / 64 / 128, two BatchNorm groups, 300 tiles on 256 workgroups: covered.  The tile shapes the cost model picks at no shape
         of this file (and only a forced ARCO_HCONV_FC_CFG reaches) are NOT run here: tests/test_conv3d_fl_gpu.py ties each of them bit
         for bit to hconv_kernel, which this file anchors to float64.
  hconv1x1_narrow_out_kernel<1|2|4>   1808004, 1816004, 1832004, N = 1 .. 4; hconv1x1_narrow_in_kernel 1900000, K = 1 .. 4, N = 8, 16, 32:
         covered, each also as the data gradient of the other (the V-Net's out_conv), and one near miss per condition (M = 65535,
         ld_in % 8 != 0, the output 8 bytes off a 16-byte boundary) that must report hconv_kernel<1,256,16> / <1,128,32>.
  conv3d_image_kernel<3> in mma 4   27701016: one plane smaller than a tile, and two volumes in two groups, both with statistics: covered.
  One data-gradient case (mode 1 | 4 pack) per kernel template against float64 autograd.
  Out of scope: hwgrad_kernel and the casts (tests/test_wgrad_kernels_gpu.py, tests/test_side_kernels_gpu.py), the f16 pooling / resize / first-layer kernels.
The cases that need 256 workgroups, 65536 rows or more units than slots are as large as that takes and no larger (the largest, 270336
voxels of 16 channels, takes under a second with its float64 reference); EVERY case runs all four kinds.

Worst err / derived bound of the wide kind per family (CPU emulation, tests/test_hconv_kernels_cpu.py | MI355X, this file):
  family  kernels                                        err / derived bound
  h2d     hconv_kernel<9,..,1>                           0.95 | 0.98
  h3d     hconv_kernel<9,..,3>, rectangular and flat     0.95 | 0.97
  h1x1    hconv_kernel<1,..>                             0.98 | 1.00 (0.9992)
  rw      hconv_rw_kernel<1,1,8>                         0.96 | 0.97
  fc      hconv_fc_kernel                                0.93 | 0.96
  nout    hconv1x1_narrow_out_kernel<1|2|4>              0.99 | 1.00 (0.9971)
  nin     hconv1x1_narrow_in_kernel                      1.00 (0.9980) | 1.00 (0.9991)
  image   conv3d_image_kernel<3>, f16 epilogue           0.98 | 0.98
  (the emulation runs the small cases only, and the first 4096 rows of the streams; the MI355X all of them.)  The bound is tight by
  construction: its leading term is the half unit of the one f16 rounding, which some element always comes close to.
  A correct round-to-nearest store never exceeds 2^-11 |v|; a truncating one reaches 1.9 of the bound (planted in the CPU file).
  BatchNorm partials, wide kind: at most 0.40 (sums) and 0.45 (sums of squares) of their bound; what binds there is the exact kind.
Every exact case (fixed, impulse, select, the integer slabs of the rounded outputs) held bit for bit on every route on the MI355X, the
subnormal weights and activations of the impulse and select kinds included: v_mfma_f32_16x16x32_f16 keeps f16 subnormal operands, and
no expectation had to be widened.  NO kernel had to be changed.  Host code only: the conv_h.hip launches now note their route, and a
call that hconv_dispatch rejects with ARCO_ERR_ARG (a pointer off its 16-byte boundary) puts the previous id back, as the header says
of every ARCO_ERR_ARG."""
import contextlib

import pytest
import torch

import hconv_kernel_refs as R
from conv_kernel_refs import ceil_to, select_passes, slab_sums, stat_totals
from hconv_kernel_refs import CASES, DGRAD, equal_h, held
from loss_kernel_refs import SENTINEL, worst
from side_kernel_refs import GUARD
from test_side_kernels_gpu import DEV, dev, filled, put

pytestmark = pytest.mark.gpu


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


def names(cases):
    return [c["name"] for c in cases]


def having(kind):
    cs = [c for c in CASES if kind in c["kinds"]]
    return pytest.mark.parametrize("c", cs, ids=names(cs))


@contextlib.contextmanager
def switches(L, c):
    """arco_conv3d_fl_set as the case needs it, restored afterwards (process state; nothing is read from the environment)"""
    prev = L.query("arco_conv3d_fl_set", c["fl"]) if c["fl"] is not None else None
    try:
        yield
    finally:
        if prev is not None:
            L.query("arco_conv3d_fl_set", prev)


def fenced(n, dtype, shift=0):
    """GUARD + shift sentinels, n elements, GUARD sentinels -> (the buffer, the view of the n elements); the view starts on a 16-byte
    boundary (8 f16 / fp32 elements of guard) plus `shift` elements"""
    buf = torch.full((GUARD + shift + int(n) + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD + shift:]


def unfence(buf, shift, rows, ld, ncol):
    """the [rows, ncol] result on the CPU, after checking that the guards in front of and behind the buffer and every pad column still
    hold the sentinel"""
    torch.cuda.synchronize()
    full = buf.cpu()
    lo = GUARD + shift
    assert bool((full[:lo] == SENTINEL).all()), "the guard in front of the buffer was written"
    assert bool((full[lo + rows * ld:] == SENTINEL).all()), "the guard behind the buffer was written"
    body = full[lo:lo + rows * ld].view(rows, ld)
    assert bool((body[:, ncol:] == SENTINEL).all()), "a pad column of ld_out > N was written"
    return body[:, :ncol].contiguous()


def pack(L, w, cout, cin, taps, mode):
    """arco_pack_conv_weight of a torch-layout weight [cout, cin, taps]: mode 4 the f16 pack [taps][ceil16 N][ceil32 K], mode 0 the fp32
    pack (their layouts are held exactly by test_conv_kernels_gpu.py::test_pack_conv_weight)"""
    n, k = (cout, cin) if mode & 1 == 0 else (cin, cout)
    if mode & 4:
        wp = filled(taps * ceil_to(n, 16) * ceil_to(k, 32), torch.float16)
    else:
        wp = filled(taps * ceil_to(n, 16) * ceil_to(k, 16))
    L.call("arco_pack_conv_weight", L.ptr(dev(w)), cout, cin, taps, mode, L.ptr(wp))
    return wp


def run(L, c, d, dgrad=False, groups=0, route=None):
    """one launch of arco_conv3d_fwd(..., mma = 4) -> the f16 output rows [M, N] on the CPU (and the stat slabs and their count)"""
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    f16 = 0 if c["fam"] == "image" else 4                                                          # the one-channel volume: fp32 in, fp32 pack
    wp = pack(L, R.forward_weight(d), K, N, T, 1 | f16) if dgrad else pack(L, d["w"], N, K, T, f16)
    _, x = put(d["x"].half() if f16 else d["x"], c["ld_in"], c["in_off"])
    obuf, o = fenced(M * c["ld_out"], torch.float16, c["out_shift"])
    b = dev(d["bias"])
    s1 = s2 = b1 = b2 = None
    nmb, asked = 0, groups
    groups = groups or (c["stats"] if c["grouped"] else 0)                                         # (the case that is one only WITH its groups)
    with switches(L, c):
        if groups:
            nmb = L.query("arco_conv_mblocks_mma", T, c["nv"] * c["d3"], c["h"], c["w"], K, N, c["ld_in"], groups, 4)
            assert nmb >= groups
            (b1, s1), (b2, s2) = fenced(N * nmb, torch.float32), fenced(N * nmb, torch.float32)
        L.call("arco_conv3d_fwd", L.ptr(x), c["ld_in"], K, L.ptr(wp), N, L.ptr(o), c["ld_out"], L.ptr(b), None, 0, L.ptr(s1), L.ptr(s2), T,
               c["nv"], c["d3"], c["h"], c["w"], max(1, groups), 4)
        took = L.query("arco_conv_last_route")
    got = unfence(obuf, c["out_shift"], M, c["ld_out"], N)
    assert took == (c["route"] if route is None else route), (c["name"], took)
    if groups:
        s1, s2 = unfence(b1, 0, N, nmb, nmb), unfence(b2, 0, N, nmb, nmb)
    return (got, s1, s2, nmb) if asked else got


def report(name, got, c, d):
    r = held(name, got, c, d)
    assert r <= 1.0, (name, r)


# ---- the routes, one kind of input per test ------------------------------------------------------------------------------------------
@having("fixed")
def test_fixed_point_is_rounded_once(L, c):
    d = R.data(c, "fixed")
    assert equal_h(run(L, c, d), d["ref"])
    print(f"{c['name']} route {c['route']}: fixed exact")


@having("impulse")
def test_impulses_return_the_weights(L, c):
    d = R.data(c, "impulse")
    assert equal_h(run(L, c, d), d["ref"])
    print(f"{c['name']} route {c['route']}: impulse exact")


@having("select")
def test_selection_weights_return_the_shifted_input(L, c):
    for p in range(select_passes(c)):
        d = R.data(c, "select", p)
        assert equal_h(run(L, c, d), d["ref"]), p
    print(f"{c['name']} route {c['route']}: select exact, {select_passes(c)} passes")


@having("wide")
def test_wide_range_is_bounded_per_element(L, c):
    d = R.data(c, "wide")
    report(f"{c['name']} [{c['fam']}] route {c['route']}", run(L, c, d), c, d)


STATS = [c for c in CASES if c["stats"]]


@pytest.mark.parametrize("c", STATS, ids=names(STATS))
def test_batchnorm_partials(L, c):
    """slabs [N][nmb], nmb from arco_conv_mblocks_mma(..., 4): group g owns the slab range [g nmb / G, (g + 1) nmb / G) and the volumes
    [g nv / G, (g + 1) nv / G); the statistics are those of the ROUNDED f16 outputs"""
    G = c["stats"]
    d = R.data(c, "stats")
    got, s1, s2, nmb = run(L, c, d, groups=G)
    assert equal_h(got, d["ref"])
    assert R.stats_exact(c, s1, s2, nmb, G, R.expected_h(d["ref"])), "a group's slabs do not sum to its volumes' totals of the rounded outputs"
    d = R.data(c, "wide")
    got, s1, s2, nmb = run(L, c, d, groups=G)
    report(f"{c['name']} [{c['fam']}] with statistics", got, c, d)
    t1, t2 = stat_totals(c, d["ref"], G)
    tol1, tol2 = R.stats_tol(c, d, G)
    ra, rb = worst(slab_sums(s1, nmb, G), t1, tol1), worst(slab_sums(s2, nmb, G), t2, tol2)
    print(f"{c['name']} partials: sum err / bound {ra:.4f}, sumsq err / bound {rb:.4f}")
    assert ra <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("c", DGRAD, ids=names(DGRAD))
def test_data_gradient_on_the_mode_5_pack(L, c):
    for kind in ("fixed", "wide"):
        d = R.data(c, kind, 0, True)
        got = run(L, c, d, dgrad=True)
        ref = R.dgrad_autograd(c, d)
        if kind == "fixed":
            assert equal_h(got, ref)
        else:
            report(f"{c['name']} [{c['fam']}] route {c['route']}", got, c, dict(d, ref=ref))


def test_a_rejected_call_notes_no_route(L):
    """after a launch: ARCO_ERR_ARG (a packed-weight or input pointer off its 16-byte boundary) leaves arco_conv_last_route as it was,
    ARCO_ERR_UNSUPPORTED (a residual; 3x3x3 with K % 8 != 0) leaves 0 - and neither writes the output"""
    c = R.by_name("h2-64x32")
    d = R.data(c, "fixed")
    run(L, c, d)
    assert L.query("arco_conv_last_route") == c["route"]
    wp = pack(L, d["w"], c["n"], c["k"], 9, 4)
    _, x = put(d["x"].half(), c["ld_in"] + 8, 8)
    obuf, o = fenced(c["M"] * c["ld_out"], torch.float16)
    lib = L.load()

    def fwd(xv, wv, ld_in, K, res, taps):
        return lib.arco_conv3d_fwd(L.ptr(xv), ld_in, K, L.ptr(wv), c["n"], L.ptr(o), c["ld_out"], None, L.ptr(res), c["n"], None, None, taps,
                                   c["nv"], 1, c["h"], c["w"], 1, 4, L.stream())

    assert fwd(x, wp[4:], c["ld_in"] + 8, c["k"], None, 9) == R.ERR_ARG and L.query("arco_conv_last_route") == c["route"]
    assert fwd(x[4:], wp, c["ld_in"] + 8, c["k"], None, 9) == R.ERR_ARG and L.query("arco_conv_last_route") == c["route"]
    assert fwd(x, wp, c["ld_in"] + 8, c["k"], o, 9) == R.ERR_UNSUPPORTED and L.query("arco_conv_last_route") == 0
    run(L, c, d)
    assert fwd(x, wp, c["ld_in"] + 8, 20, None, 27) == R.ERR_UNSUPPORTED and L.query("arco_conv_last_route") == 0
    torch.cuda.synchronize()
    assert bool((obuf.cpu() == SENTINEL).all())
