"""Every forward-convolution route of csrc/igemm.hip, conv_sp.hip, gemm_sp.hip and conv3d_fl.hip called DIRECTLY (arco_amd._lib:
arco_conv_fwd for 2-D in mma 0, arco_conv3d_fwd otherwise), one route per test, against a plain float64 F.conv2d / F.conv3d of the same
fp32 input values (tests/conv_kernel_refs.py) - not through ops.py and not against another HIP route.  Every test asserts the kernel
that ran through arco_conv_last_route (ids: include/arco_hip.h).  Every output buffer is prefilled with a sentinel: the pad columns of
ld_out > N and GUARD elements behind the buffer must keep it; operands are also passed as channel slices (ld_in > K at a column
offset, ld_res > N).

Kinds of input (conv_kernel_refs.py): `fixed` (integers times a power of two inside the 2^24 budget, 9-bit values on both operands:
planes 0 and 1 of the split), `impulse` (unit impulses against full 24-bit weights: weight plane 2) and `select` (one +-2^e weight per
output channel, every tap, against full 24-bit activations: activation plane 2) must equal the float64 convolution BIT FOR BIT
(torch.equal); `wide` (six decades, 20 % zeros) is held per element to the derived bound gamma(n) S + u |ref| (+ the dropped terms of
mma 3) and to the project's measured 3e-6 S.  BatchNorm partials: on shrunk fixed data every slab is an integer number of quanta and the
float64 host sum of a group's slab range EQUALS that group's sum y and sum y^2; on wide data a derived bound.

Worst ratios per family, err / derived bound and err / (3e-6 S) (CPU emulation, tests/test_conv_kernels_cpu.py | MI355X, this file):
  family  kernels                                      err / derived bound    err / (3e-6 S)
  1x1     narrow-out streams (nout)                    0.54 | 0.60            0.10 | 0.10
  1x1     narrow-in stream (nin)                       0.70 | 0.70            0.07 | 0.07
  1x1     fp32 MFMA (mfma0)                            0.11 | 0.20            0.17 | 0.23
  1x1     split-bf16 incl. gemm_sp_kernel (mfma3)      0.05 | 0.05            0.30 | 0.19
  3x3     image kernels                                0.09 | 0.22            0.13 | 0.19
  3x3     fp32 MFMA incl. the halo kernels (mfma0)     0.02 | 0.07            0.15 | 0.40
  3x3     split-bf16 incl. conv_sp.hip (mfma3)         0.02 | 0.05            0.36 | 0.40
  3x3x3   conv3d_image_kernel<3>                       0.04 | 0.17            0.05 | 0.19
  3x3x3   fp32 MFMA (mfma0)                            0.01 | 0.03            0.30 | 0.54
  3x3x3   split-bf16 incl. conv3d_fl.hip, rw16 (mfma3) 0.006 | 0.009          0.40 | 0.53
  (the emulation runs the small cases only, the MI355X all of them.)  arco_gemm_splitk 0.03 / 0.14, arco_gemm_batched 0.05,
  arco_conv1x1_upres_fwd 0.04, and 0.14 of 3e-6 S + blend_tol (the project's 3e-6 S figure with the resize's own tolerance of
  side_kernel_refs.py added, as that error is no part of the GEMM's) (MI355X).  BatchNorm partials, wide kind: at most 0.001 of their bound (it allows every output its
  own bound and gamma(M / G) for the sums: rigorous, far from tight); what binds there is the exact kind.
  Every exact case (fixed, impulse, select, the integer slabs) held bit for bit on every route on the MI355X: no kernel had to be changed.

Routes covered: the four conv1x1_narrow_out_kernel<Q> and conv1x1_narrow_in_kernel; gemm_sp_kernel<false> (arco_gemm_sp_set(1, 1)) and
<true> (arco_conv1x1_upres_fwd); igemm_kernel<1,..> 256x16, 128x32, 32x64, 64x64, 64x224, 128x128 in mma 0 and 3 (and the scalar-load
form, K = 19); conv3d_image_kernel<1>, <3>, conv3x3_image_kernel (K = 3, 4), the four conv3x3_halo_kernel; every dispatch_spatial<1>,
dispatch_spatial<3> and dispatch_flat3 tile in both modes; launch_sp<4|2|1, 4|2> and <4,1>, launch_rw<4,1,8> (16->16, 16->4, 4->16,
32->16), launch_rw<2,2,8>; conv3d_rw16_kernel; conv3d_fc_kernel<1|2|4,2>, <2,4> and conv3d_fl_kernel<4,4> as fl_cost picks them at the
plane widths 56, 28, 14, 7; arco_pack_conv_weight / arco_pack_many (exact on integer views), arco_gemm_splitk, arco_gemm_batched; one
mode-1-pack data-gradient case per family against float64 autograd.  Edges per family: planes smaller than a tile and no multiple of it,
N = 19 / 4 / 2, K = 20 / 48, one image and one single-plane volume (NV D3 = 1: conv3d_image_kernel<3>, conv3d_rw16_kernel,
conv3d_fc_kernel, one dispatch_spatial<3> and one flat tile), and more tiles than workgroups with a ragged last round on every
persistent kernel.
Not covered, and why: launch_sp<2,1> and <1,1> (dispatch_rows<1> is never called: unreachable); gemm_sp_kernel at N = 64 (its padding
rule refuses Npad < 208 at any tile threshold: the case asserts igemm_kernel<1,32,64>); the tile shapes of conv3d_fl.hip that fl_cost
picks at no plane width of this file and only a forced ARCO_CONV3D_FL_CFG reaches (tests/test_conv3d_fl_gpu.py runs each of them).  The
largest 3x3x3 tiles (50176 .. 65536 voxels) run the fixed and the wide kind only; their smaller siblings run all four.
Out of scope: the weight-gradient kernels, the BatchNorm / GroupNorm family (held to float64 kernel by kernel in
tests/test_norm_kernels_gpu.py), conv_h.hip (mma 4: held to float64 route by route in tests/test_hconv_kernels_gpu.py), the
opt-in mma 1 / 2 (held bit for bit to a float64 convolution of the rounded operands in tests/test_mma12_kernels_gpu.py) and
arco_conv3d_fwd_pro (tests/test_block_fuse_gpu.py ties it bit for bit to the two-pass route that this file anchors)."""
import contextlib
import struct

import numpy as np
import pytest
import torch

import conv_kernel_refs as R
import side_kernel_refs as SR
from conv_kernel_refs import CASES, DGRAD, equal_bits, held
from loss_kernel_refs import SENTINEL, worst
from side_kernel_refs import GUARD, body, cols
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
    """the A/B switches a case needs, restored afterwards (they are process state; nothing is read from the environment)"""
    prev_fl = L.query("arco_conv3d_fl_set", 0) if c["fl0"] else None
    if c["gsp"]:
        L.query("arco_gemm_sp_set", 1, 1)
    try:
        yield
    finally:
        if c["gsp"]:
            L.query("arco_gemm_sp_set", 1, 2048)
        if prev_fl is not None:
            L.query("arco_conv3d_fl_set", prev_fl)


def pack(L, w, cout, cin, taps, mode):
    """arco_pack_conv_weight of a torch-layout weight [cout, cin, taps] (its layouts are held exactly by test_pack_conv_weight)"""
    n, k = (cout, cin) if mode & 1 == 0 else (cin, cout)
    npad = R.ceil_to(n, 16)
    size = taps * npad * (R.ceil_to(k, 32) * 3 // 2 if mode & 2 else R.ceil_to(k, 16))
    wp = torch.empty(size, dtype=torch.float32, device=DEV)
    L.call("arco_pack_conv_weight", L.ptr(dev(w)), cout, cin, taps, mode, L.ptr(wp))
    return wp


def run(L, c, d, dgrad=False, groups=0):
    """one launch of the case's entry point -> (output rows [M, N] on the CPU, stat slabs or None, slab count)"""
    M, K, N, T, mma = c["M"], c["k"], c["n"], c["taps"], c["mma"]
    split = 2 if mma == 3 else 0
    wp = pack(L, R.forward_weight(d), K, N, T, 1 | split) if dgrad else pack(L, d["w"], N, K, T, split)
    _, x = put(d["x"], c["ld_in"], c["in_off"])
    ob = filled(M * c["ld_out"])
    r = None if d["res"] is None else put(d["res"], c["ld_res"])[1]
    b = dev(d["bias"])
    s1 = s2 = None
    nmb = 0
    with switches(L, c):
        if groups:
            nmb = L.query("arco_conv_mblocks_mma", T, c["nv"] * c["d3"], c["h"], c["w"], K, N, c["ld_in"], groups, mma)
            assert nmb >= groups
            s1, s2 = filled(N * nmb), filled(N * nmb)
        if mma == 0 and T != 27 and c["d3"] == 1 and groups <= 1:
            L.call("arco_conv_fwd", L.ptr(x), c["ld_in"], K, L.ptr(wp), N, L.ptr(ob), c["ld_out"], L.ptr(b), L.ptr(r), c["ld_res"], L.ptr(s1),
                   L.ptr(s2), T, c["nv"], c["h"], c["w"])
        else:
            L.call("arco_conv3d_fwd", L.ptr(x), c["ld_in"], K, L.ptr(wp), N, L.ptr(ob), c["ld_out"], L.ptr(b), L.ptr(r), c["ld_res"], L.ptr(s1),
                   L.ptr(s2), T, c["nv"], c["d3"], c["h"], c["w"], max(1, groups), mma)
        route = L.query("arco_conv_last_route")
    got, ok = cols(ob, M, c["ld_out"], 0, N)
    assert ok, "a pad column of ld_out > N was written"
    assert route == c["route"], (c["name"], route)
    if groups:
        return got, body(s1, N * nmb, (N, nmb)), body(s2, N * nmb, (N, nmb)), nmb
    return got


def report(name, got, c, d):
    r1, r2 = held(name, got, c, d)
    assert r1 <= 1.0 and r2 <= 1.0, (name, r1, r2)


# ---- the routes, one kind of input per test ------------------------------------------------------------------------------------------
@having("fixed")
def test_fixed_point_is_exact(L, c):
    d = R.data(c, "fixed")
    assert equal_bits(run(L, c, d), d["ref"])
    print(f"{c['name']} route {c['route']}: fixed exact")


@having("impulse")
def test_impulses_return_the_weights(L, c):
    d = R.data(c, "impulse")
    assert equal_bits(run(L, c, d), d["ref"])
    print(f"{c['name']} route {c['route']}: impulse exact")


@having("select")
def test_selection_weights_return_the_shifted_input(L, c):
    for p in range(R.select_passes(c)):
        d = R.data(c, "select", p)
        assert equal_bits(run(L, c, d), d["ref"]), p
    print(f"{c['name']} route {c['route']}: select exact, {R.select_passes(c)} passes")


@having("wide")
def test_wide_range_is_bounded_per_element(L, c):
    d = R.data(c, "wide")
    report(f"{c['name']} [{R.FAMILY[c['taps']]} {c['fam']}] route {c['route']}", run(L, c, d), c, d)


STATS = [c for c in CASES if c["stats"]]


@pytest.mark.parametrize("c", STATS, ids=names(STATS))
def test_batchnorm_partials(L, c):
    """slabs [N][nmb], nmb from arco_conv_mblocks_mma: group g owns the slab range [g nmb / G, (g + 1) nmb / G) and the volumes
    [g nv / G, (g + 1) nv / G); the buffers hold nmb slabs per channel and the guard behind them keeps the sentinel"""
    G = c["stats"]
    d = R.data(c, "stats")
    got, s1, s2, nmb = run(L, c, d, groups=G)
    assert equal_bits(got, d["ref"])
    assert R.stats_exact(c, s1, s2, nmb, G, d["ref"]), "a group's slabs do not sum to its volumes' totals"
    d = R.data(c, "wide")
    got, s1, s2, nmb = run(L, c, d, groups=G)
    report(f"{c['name']} with statistics", got, c, d)
    t1, t2 = R.stat_totals(c, d["ref"], G)
    tol1, tol2 = R.stats_tol(c, d, G)
    ra, rb = worst(R.slab_sums(s1, nmb, G), t1, tol1), worst(R.slab_sums(s2, nmb, G), t2, tol2)
    print(f"{c['name']} partials: sum err / bound {ra:.4f}, sumsq err / bound {rb:.4f}")
    assert ra <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("c", DGRAD, ids=names(DGRAD))
def test_data_gradient_on_the_mode_1_pack(L, c):
    for kind in ("fixed", "wide"):
        d = R.data(c, kind, 0, True)
        got = run(L, c, d, dgrad=True)
        ref = R.dgrad_autograd(c, d)
        if kind == "fixed":
            assert equal_bits(got, ref)
        else:
            report(f"{c['name']} route {c['route']}", got, c, dict(d, ref=ref))


# ---- the weight packs: exact on integer views ------------------------------------------------------------------------------------------
def _pack_dims(n, k, mode):
    return R.ceil_to(n, 16), (R.ceil_to(k, 32) if mode & 6 else R.ceil_to(k, 16))


def _packed_view(buf, count, mode):
    """the first `count` packed ELEMENTS as integers (f16: one int16 each; split: three int16; plain: one int32)"""
    if mode & 4:
        return body(buf, count).view(torch.int16).numpy()
    if mode & 2:
        return body(buf, count * 3 // 2).view(torch.int16).numpy()
    return body(buf, count).view(torch.int32).numpy()


@pytest.mark.parametrize("mode", range(6))
@pytest.mark.parametrize("shape", [(19, 20, 1), (5, 3, 9), (40, 24, 9), (17, 33, 27)], ids=str)
def test_pack_conv_weight(L, shape, mode):
    cout, cin, taps = shape
    W = R._wide_values((cout, cin, taps), R.gen(cout, cin, taps), 3, 0.1)
    n, k = (cout, cin) if mode & 1 == 0 else (cin, cout)
    npad, kpad = _pack_dims(n, k, mode)
    count = taps * npad * kpad
    buf = filled(count, torch.float16) if mode & 4 else filled(count * 3 // 2 if mode & 2 else count)
    L.call("arco_pack_conv_weight", L.ptr(dev(W)), cout, cin, taps, mode, L.ptr(buf))
    want = R.pack_expected(R.pack_logical(W.numpy(), cout, cin, taps, mode), mode, npad, kpad)
    assert np.array_equal(_packed_view(buf, count, mode), want.reshape(-1))


def test_pack_many(L):
    """every form in one launch: modes 0 .. 5 on 3x3 / 3x3x3 weights (the tile path) and a 1x1 weight (element-wise), and the
    mode >> 3 gather forms 1, 2, 4 of the k2 s2 convolutions, plain, transposed, split and f16"""
    recs, keep = [], []

    def add(src, cout, cin, taps, mode, npad, kpad, logical):
        count = (1 if mode >> 3 else taps) * npad * kpad
        buf = filled(count, torch.float16) if mode & 4 else filled(count * 3 // 2 if mode & 2 else count)
        s = dev(src)
        keep.append((s, buf, count, mode, R.pack_expected(logical, mode, npad, kpad)))
        recs.append(struct.pack("<QQiiiiiiq", s.data_ptr(), buf.data_ptr(), cout, cin, taps, mode, npad, kpad, 0))

    for (cout, cin, taps) in ((40, 24, 9), (17, 33, 27), (19, 20, 1)):
        W = R._wide_values((cout, cin, taps), R.gen(7, cout, taps), 3, 0.1)
        for mode in range(6):
            n, k = (cout, cin) if mode & 1 == 0 else (cin, cout)
            add(W, cout, cin, taps, mode, *_pack_dims(n, k, mode), R.pack_logical(W.numpy(), cout, cin, taps, mode))
    co, ci = 16, 6                                                       # nn.Conv3d(ci, co, 2, 2): W2 [co][8 ci]; nn.ConvTranspose3d: W2 [8 co][ci]
    Wd, Wu, bias = (R._wide_values(s, R.gen(8, i), 3, 0.1) for i, s in enumerate(((co, ci, 8), (ci, co, 8), (co,))))
    for gm, src, n2, k2, g in ((1, Wd, co, 8 * ci, ci), (2, Wu, 8 * co, ci, co)):
        for mode in (0, 1, 2, 3, 4, 5):
            n, k = (n2, k2) if mode & 1 == 0 else (k2, n2)
            npad, kpad = (n, k) if mode & 6 == 0 else (n, R.ceil_to(k, 32))
            add(src, n2, k2, g, (gm << 3) | mode, npad, kpad, R.pack_gather_logical(src.numpy(), n2, k2, g, gm, mode))
    add(bias, 1, 8 * co, co, 4 << 3, 1, 8 * co, R.pack_gather_logical(bias.numpy(), 1, 8 * co, co, 4, 0))
    assert len(recs[0]) == L.query("arco_pack_desc_bytes")
    desc = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(DEV)
    L.call("arco_pack_many", L.ptr(desc), len(recs), sum(k[2] for k in keep))
    for i, (_, buf, count, mode, want) in enumerate(keep):
        assert np.array_equal(_packed_view(buf, count, mode), want.reshape(-1)), (i, mode)


# ---- split-K, batched and the fused-upsample GEMM ----------------------------------------------------------------------------------------
GEMM = R.C("gemm", 1, 0, 1, 1, 1, 37, 100, 19, 1128032, "mfma0")


def _gemm_data(kind, seed):
    c = dict(GEMM, name=f"gemm{seed}")
    g = R.gen(99, seed)
    M, K, N = c["M"], c["k"], c["n"]
    if kind == "fixed":
        x, w = R._ints((M, K), g, -255, 255).float() * R.QX, R._ints((N, K, 1), g, -255, 255).float() * R.QW
    else:
        x, w = R._wide_values((M, K), g, 3, 0.2), (R._wide_values((N, K, 1), g, 2, 0.0) / 10).float()
    return c, R.finish(c, dict(x=x, w=w, bias=None, res=None))


@pytest.mark.parametrize("splits", (1, 2, 3))
def test_gemm_splitk(L, splits):
    """K = 100 in 1, 2 and 3 slabs (3 does not divide the 7 chunks of 16); the slab sum writes whole rows of ld_out = 20 floats: only
    the guard behind the buffer keeps the sentinel.  Each slab is one more rounding: n + splits."""
    for kind in ("fixed", "wide"):
        c, d = _gemm_data(kind, splits)
        M, K, N = c["M"], c["k"], c["n"]
        wp = pack(L, d["w"], N, K, 1, 0)
        _, x = put(d["x"], K + 4, 4)
        ob, ws = filled(M * 20), torch.zeros(splits * M * 20, device=DEV)
        L.call("arco_gemm_splitk", L.ptr(x), K + 4, K, L.ptr(wp), N, L.ptr(ob), 20, M, splits, L.ptr(ws))
        assert L.query("arco_conv_last_route") == c["route"]
        got = body(ob, M * 20, (M, 20))[:, :N]
        if kind == "fixed":
            assert equal_bits(got, d["ref"])
        else:
            r = worst(got, d["ref"], R.tol_wide(c, d) + R.gamma(splits) * d["S"])
            print(f"gemm_splitk {splits}: worst err / bound {r:.4f}, err / (3e-6 S) {worst(got, d['ref'], R.MEASURED * d['S']):.3f}")
            assert r <= 1.0 and worst(got, d["ref"], R.MEASURED * d["S"]) <= 1.0


@pytest.mark.parametrize("splits", (1, 2))
def test_gemm_batched(L, splits):
    """three independent problems at operand strides that leave gaps; splits = 1 writes N of ld_out columns (the pad keeps the
    sentinel), splits = 2 whole rows"""
    B = 3
    for kind in ("fixed", "wide"):
        cs = [_gemm_data(kind, 10 + z) for z in range(B)]
        c = cs[0][0]
        M, K, N = c["M"], c["k"], c["n"]
        sx, sw, so = M * K + 8, 32 * 112 + 16, M * 20 + 12
        xb, wb = torch.zeros(B * sx, device=DEV), torch.zeros(B * sw, device=DEV)
        for z, (_, d) in enumerate(cs):
            xb[z * sx:z * sx + M * K] = dev(d["x"]).flatten()
            wb[z * sw:z * sw + 32 * 112] = pack(L, d["w"], N, K, 1, 0)
        ob = filled(B * so)
        ws = torch.zeros(B * splits * M * 20, device=DEV) if splits > 1 else None
        L.call("arco_gemm_batched", L.ptr(xb), K, K, L.ptr(wb), N, L.ptr(ob), 20, M, B, sx, sw, so, splits, L.ptr(ws))
        assert L.query("arco_conv_last_route") == c["route"]
        full = body(ob, B * so, (B, so))
        assert bool((full[:, M * 20:] == SENTINEL).all())                                          # the gaps between the problems
        for z, (cz, d) in enumerate(cs):
            rows = full[z, :M * 20].view(M, 20)
            got = rows[:, :N]
            assert splits > 1 or bool((rows[:, N:] == SENTINEL).all())
            if kind == "fixed":
                assert equal_bits(got, d["ref"]), z
            else:
                r = worst(got, d["ref"], R.tol_wide(cz, d) + R.gamma(splits) * d["S"])
                print(f"gemm_batched {splits} problem {z}: worst err / bound {r:.4f}")
                assert r <= 1.0 and worst(got, d["ref"], R.MEASURED * d["S"]) <= 1.0


UPRES = [("identity", (2, 3, 5), (2, 3, 5), 208, 32), ("x2", (3, 4, 5), (6, 8, 10), 208, 48), ("refused-n64", (3, 4, 5), (6, 8, 10), 64, 32)]


@pytest.mark.parametrize("name,lo,hi,N,K", UPRES, ids=[u[0] for u in UPRES])
def test_conv1x1_upres_fwd(L, name, lo, hi, N, K):
    """out = W . in + trilinear_align_corners(lo) on gemm_sp_kernel<true> (arco_gemm_sp_set(1, 1)).  identity: the blend of equal grids is
    the value itself, fixed-point data must come back exact.  x2: the GEMM's bound plus blend_tol (side_kernel_refs.py) of the resize.
    refused: N = 64 returns ARCO_ERR_UNSUPPORTED; the documented fallback (arco_trilinear_fwd, then arco_conv3d_fwd with the result as
    residual) is run instead and held to the same reference."""
    NV = 2
    M = NV * int(np.prod(hi))
    c = R.C(f"upres-{name}", 1, 3, NV, hi[0], hi[1], hi[2], K, N, 1514256, "mfma3", res=True)
    g = R.gen(55, N, K, *hi)
    kinds = ("fixed", "wide") if name == "identity" else ("wide",)
    for kind in kinds:
        if kind == "fixed":
            x, w = R._ints((M, K), g, -255, 255).float() * R.QX, R._ints((N, K, 1), g, -255, 255).float() * R.QW
            low = R._ints((NV, *lo, N), g, -2 ** 18, 2 ** 18).float() * R.QUANT
        else:
            x, w = R._wide_values((M, K), g, 3, 0.2), (R._wide_values((N, K, 1), g, 2, 0.0) / 7).float()
            low = R._wide_values((NV, *lo, N), g, 3, 0.2)
        up = SR.interp64(low, hi).view(M, N)
        d = R.finish(c, dict(x=x, w=w, bias=None, res=None))
        d["ref"], d["S"] = d["ref"] + up, d["S"] + up.abs()
        wp = pack(L, w, N, K, 1, 2)
        _, xv = put(x, K + 4, 4)
        _, lv = put(low.view(-1, N), N + 4)
        ob = filled(M * (N + 4))
        L.query("arco_gemm_sp_set", 1, 1)
        try:
            rc = L.load().arco_conv1x1_upres_fwd(L.ptr(xv), K + 4, K, L.ptr(wp), N, L.ptr(ob), N + 4, L.ptr(lv), N + 4, NV, *lo, *hi, L.stream())
            if name.startswith("refused"):
                assert rc == R.ERR_UNSUPPORTED and L.query("arco_conv_last_route") == 0             # no kernel taken, no stale id
                ub = filled(M * N)
                L.call("arco_trilinear_fwd", L.ptr(lv), N + 4, NV, *lo, N, *hi, L.ptr(ub), N)
                L.call("arco_conv3d_fwd", L.ptr(xv), K + 4, K, L.ptr(wp), N, L.ptr(ob), N + 4, None, L.ptr(ub), N, None, None, 1, NV, *hi, 1, 3)
                assert L.query("arco_conv_last_route") == 1032064
            else:
                assert rc == 0 and L.query("arco_conv_last_route") == 1514256
        finally:
            L.query("arco_gemm_sp_set", 1, 2048)
        got, ok = cols(ob, M, N + 4, 0, N)
        assert ok
        if kind == "fixed":
            assert equal_bits(got, d["ref"])
        else:
            tol = R.tol_wide(c, d) + SR.blend_tol(low, lo, hi).view(M, N) * (1 + R.U)
            r1, r2 = worst(got, d["ref"], tol), worst(got, d["ref"], R.MEASURED * d["S"] + SR.blend_tol(low, lo, hi).view(M, N))
            print(f"upres {name}: worst err / bound {r1:.4f}, err / (3e-6 S + the resize's blend_tol) {r2:.3f}")
            assert r1 <= 1.0 and r2 <= 1.0
