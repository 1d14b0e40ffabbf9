"""The reduced-operand modes of arco_conv3d_fwd on fp32 tensors - mma 1 (f16 operands) and mma 2 (bf16 operands): the MMA == 1 / MMA == 2
branches of igemm_kernel (csrc/igemm.hip), to_f16x4 / to_bf16x4 (csrc/split_bf16.h), the mode gate of launch_igemm - called DIRECTLY, one
route per test and mode, against a float64 convolution of the ROUNDED operands (tests/mma12_kernel_refs.py): both operands to nearest
even, exact products, fp32 accumulation, bias and residual unrounded in the fp32 epilogue.  Every test asserts the kernel that ran through
arco_conv_last_route; every output buffer is prefilled with a sentinel that the pad columns of ld_out > N and the GUARD elements behind
the buffer must keep; operands are also passed as channel slices (ld_in > K at a column offset, ld_res > N).

Kinds of input: `fixed` (integers inside the 2^24 budget, channels on rounding ties of the mode on x and on w), `impulse` (unit impulses
against 24-bit weights over the whole range of the mode, f16 subnormals and the neighbourhood of 65504 included) and `select` (one +-2^e
weight per output channel, every tap, against 24-bit activations of the same range) must equal the reference BIT FOR BIT (torch.equal) -
and those references differ from the unrounded ones on at least a quarter of the outputs (tests/test_mma12_kernels_cpu.py), so a tile
that fell back to the fp32 MFMA, truncated, rounded one operand only, took the other format or broke ties away from zero cannot pass;
`wide` (six decades, 20 % zeros) is held per element to gamma(taps K + 2) S_r + u |ref|; `overflow` (mma 1): 65520 and 1e6 become +inf
and the output is IEEE arithmetic on the rounded operands, NaN = inf * 0 included.  BatchNorm partials: the float64 host sum of each
group's slab range EQUALS that group's sum y and sum y^2 on integer data; on wide data a derived bound.

Worst ratios of the wide kind per family, err / derived bound and err / (3e-6 S_r) (CPU emulation of the small cases,
tests/test_mma12_kernels_cpu.py | MI355X, this file, all cases; the second ratio is recorded, not asserted):
  family              mode     err / derived bound    err / (3e-6 S_r)
  1x1                 mma 1    0.18 | 0.26            0.16 | 0.12
  1x1                 mma 2    0.23 | 0.24            0.15 | 0.14
  3x3x3 rectangular   mma 1    0.031 | 0.027          0.30 | 0.23
  3x3x3 rectangular   mma 2    0.028 | 0.026          0.27 | 0.23
  3x3x3 flat          mma 1    0.045 | 0.024          0.39 | 0.21
  3x3x3 flat          mma 2    0.031 | 0.025          0.29 | 0.22
  (the emulation runs the small cases only, the MI355X all of them.)  Data gradient (mma 2): 0.05 / 0.005 of the bound at taps 1 / 27;
  BatchNorm partials of the wide kind: at most 0.013 of their bound.
  Every exact kind - fixed, impulse, select on every tile in both modes, the integer slabs, the data gradients, the overflow kind (the
  MI355X rounds 65520 and 1e6 to +inf and propagates inf * 0 = NaN as IEEE does) and the ops.py patterns - held bit for bit on the
  MI355X, and every fallback shape came out on the unrounded fp32 arithmetic: no kernel and no line of ops.py had to be changed.

Routes covered, each in both modes: igemm_kernel<1,..> 256x16, 128x32, 32x64, 64x64, 64x224 (N = 448), 128x128, and 256x16 for the narrow
shape that mma 0 gives to conv1x1_narrow_out_kernel<4>; every dispatch_spatial<3> tile (128x16, 128x32, 64x32 by both of its conditions,
128x64, 64x64, 32x32) and every dispatch_flat3 tile at the plane widths 7 / 14 / 28; volumes of one plane; one mode-1-pack data-gradient
case per taps value in mma 2 against float64 autograd.  Fallbacks, pinned by the data (the result equals the UNROUNDED exact reference
bit for bit and differs from the rounded one): 3x3 per plane (D3 = 1: igemm_kernel DEPTH 1 and the halo kernel), K = 19 and
ld_in % 4 != 0 (the scalar-load form) at taps 1 and 27, the one-channel 3x3x3 volume (conv3d_image_kernel<3>).
The mode choice of ops.py (HEAD_MMA, CONV_MMA) is held at the end of the file on single-product data whose fp32, f16-rounded and
bf16-rounded results are three different bit patterns.  arco_conv3d_fwd_pro takes mma 3 only and is out of scope."""
import pytest
import torch

import conv_kernel_refs as R
import mma12_kernel_refs as Q
from conv_kernel_refs import equal_bits
from loss_kernel_refs import worst
from mma12_kernel_refs import CASES, DGRAD, FALLBACK, OVERFLOW, names
from side_kernel_refs import body, cols
from test_conv_kernels_gpu import pack
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


def having(kind, cases=CASES):
    cs = Q.having(kind, cases)
    return pytest.mark.parametrize("c", cs, ids=names(cs))


def run(L, c, d, dgrad=False, groups=0):
    """one launch of arco_conv3d_fwd in the case's mode on the plain fp32 pack (mode 0; mode 1 for the data gradient)
    -> output rows [M, N] on the CPU (and the stat slabs and their count with groups)"""
    M, K, N, T = c["M"], c["k"], c["n"], c["taps"]
    wp = pack(L, R.forward_weight(d), K, N, T, 1) if dgrad else pack(L, d["w"], N, K, T, 0)
    _, x = put(d["x"], c["ld_in"], c["in_off"])
    ob = filled(M * c["ld_out"])
    r = None if d["res"] is None else put(d["res"], c["ld_res"])[1]
    b = dev(d["bias"])
    s1 = s2 = None
    nmb = 0
    if groups:
        nmb = L.query("arco_conv_mblocks_mma", T, c["nv"] * c["d3"], c["h"], c["w"], K, N, c["ld_in"], groups, c["mma"])
        assert nmb >= groups
        s1, s2 = filled(N * nmb), filled(N * nmb)
    L.call("arco_conv3d_fwd", L.ptr(x), c["ld_in"], K, L.ptr(wp), N, L.ptr(ob), c["ld_out"], L.ptr(b), L.ptr(r), c["ld_res"], L.ptr(s1),
           L.ptr(s2), T, c["nv"], c["d3"], c["h"], c["w"], max(1, groups), c["mma"])
    route = L.query("arco_conv_last_route")
    got, ok = cols(ob, M, c["ld_out"], 0, N)
    assert ok, "a pad column of ld_out > N was written"
    assert route == c["route"], (c["name"], route)
    if groups:
        return got, body(s1, N * nmb, (N, nmb)), body(s2, N * nmb, (N, nmb)), nmb
    return got


def report(name, got, c, d):
    r1, _ = Q.held(name, got, c, d)
    assert r1 <= 1.0, (name, r1)


# ---- the routes, one kind of input per test --------------------------------------------------------------------------------------------
@having("fixed")
def test_fixed_point_is_exact(L, c):
    d = Q.data(c, "fixed")
    assert equal_bits(run(L, c, d), d["ref"])
    print(f"{c['name']} route {c['route']}: fixed exact")


@having("impulse")
def test_impulses_return_the_rounded_weights(L, c):
    d = Q.data(c, "impulse")
    assert equal_bits(run(L, c, d), d["ref"])
    print(f"{c['name']} route {c['route']}: impulse exact")


@having("select")
def test_selection_weights_return_the_rounded_shifted_input(L, c):
    for p in range(Q.select_passes(c)):
        d = Q.data(c, "select", p)
        assert equal_bits(run(L, c, d), d["ref"]), p
    print(f"{c['name']} route {c['route']}: select exact, {Q.select_passes(c)} passes")


@having("wide")
def test_wide_range_is_bounded_per_element(L, c):
    d = Q.data(c, "wide")
    report(f"{c['name']} [{Q.FAMILY[c['name']]}, mma {c['mma']}] route {c['route']}", run(L, c, d), c, d)


STATS = [c for c in CASES if c["stats"]]


@pytest.mark.parametrize("c", STATS, ids=names(STATS))
def test_batchnorm_partials(L, c):
    """slabs [N][nmb], nmb from arco_conv_mblocks_mma: group g owns the slab range [g nmb / G, (g + 1) nmb / G) and the volumes
    [g nv / G, (g + 1) nv / G); the buffers hold nmb slabs per channel and the guard behind them keeps the sentinel"""
    G = c["stats"]
    d = Q.data(c, "stats")
    got, s1, s2, nmb = run(L, c, d, groups=G)
    assert equal_bits(got, d["ref"])
    assert R.stats_exact(c, s1, s2, nmb, G, d["ref"]), "a group's slabs do not sum to its volumes' totals"
    d = Q.data(c, "wide")
    got, s1, s2, nmb = run(L, c, d, groups=G)
    report(f"{c['name']} with statistics", got, c, d)
    t1, t2 = R.stat_totals(c, d["ref"], G)
    tol1, tol2 = Q.stats_tol(c, d, G)
    ra, rb = worst(R.slab_sums(s1, nmb, G), t1, tol1), worst(R.slab_sums(s2, nmb, G), t2, tol2)
    print(f"{c['name']} partials: sum err / bound {ra:.4f}, sumsq err / bound {rb:.4f}")
    assert ra <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("c", DGRAD, ids=names(DGRAD))
def test_data_gradient_on_the_mode_1_pack(L, c):
    for kind in c["kinds"]:
        d = Q.data(c, kind)
        got = run(L, c, d, dgrad=True)
        ref = Q.dgrad_autograd(c, d)
        if kind == "fixed":
            assert equal_bits(got, ref)
        else:
            report(f"{c['name']} route {c['route']}", got, c, dict(d, ref=ref))


@pytest.mark.parametrize("c", FALLBACK, ids=names(FALLBACK))
def test_fallback_shapes_run_the_fp32_arithmetic(L, c):
    """these shapes must come out on the fp32 arithmetic whatever the mode: 3x3 per plane (D3 = 1), the scalar-load form (K = 19 or
    ld_in % 4 != 0) and the one-channel 3x3x3 volume.  The route id does not encode the mode, so the data decide: on the fixed kind of
    the mode (ties on the operands, everything exact in fp32) the result equals the UNROUNDED exact reference bit for bit and differs
    from the rounded one."""
    d = Q.data(c, "fixed")
    got = run(L, c, d)
    assert equal_bits(got, Q.unrounded(c, d)), "not the fp32 arithmetic"
    assert not equal_bits(got, d["ref"]) and Q.differs(got.double(), d["ref"]) >= 0.25


def test_f16_overflow_goes_to_infinity(L):
    """mma 1: an activation of 65520 (the tie above 65504) or 1e6 becomes +inf, as .half() and the f16-storage route round it - not
    65504.  Single-product outputs: +-inf where the row's selected weight meets it, NaN = inf * 0 in the row's other channels, every
    other row finite and exact."""
    c, d = OVERFLOW, Q.data(OVERFLOW, "overflow")
    got = run(L, c, d).double()
    print("overflow rows, kernel:", got[torch.isinf(Q.rne_f16(d["x"])).any(1)].tolist())
    assert torch.equal(torch.isnan(got), torch.isnan(d["ref"]))
    assert torch.allclose(got, d["ref"], rtol=0.0, atol=0.0, equal_nan=True)


# ---- the mode choice of ops.py ---------------------------------------------------------------------------------------------------------
def _ties(shape, g, scale):
    """odd 12-bit integers whose residue mod 16 is none of 1, 15: a tie of f16 (-> the even neighbour) that bf16 rounds elsewhere (to a
    multiple of 16), 7 and 9 beside the bf16 tie at 8: fp32, f16 and bf16 give three different values"""
    v = 2048 + 16 * R._ints(shape, g, 0, 127) + 3 + 2 * R._ints(shape, g, 0, 5)
    return (v * (2 * R._ints(shape, g, 0, 1) - 1)).float() * scale


def _ops_problem(taps, dims, ci, co, seed):
    """select-form data for ops.conv forward + backward, every result a single product: w one tie value per output channel (channel
    (7 n + 3) % ci - injective - and tap n % taps), x tie values everywhere, dy one tie value per output channel in a row of its own"""
    g = R.gen(81, taps, ci, co, seed)
    sp = dims[1:]
    c = R.C(f"ops-{taps}-{seed}", taps, 0, dims[0], sp[0] if len(sp) == 3 else 1, sp[-2], sp[-1], ci, co, 0, "mfma12")
    M = c["M"]
    x = _ties((M, ci), g, 2.0 ** -8)
    w = torch.zeros((co, ci, taps))
    dy = torch.zeros((M, co))
    inner = [m for m in range(M) if taps == 1 or (0 < m % c["w"] < c["w"] - 1 and 0 < m // c["w"] % c["h"] < c["h"] - 1
                                                  and (taps == 9 or 0 < m // (c["w"] * c["h"]) % c["d3"] < c["d3"] - 1))]
    for n in range(co):                                                       # (rows off the border: every tap of dy's row sees data)
        w[n, (7 * n + 3) % ci, n % taps] = _ties((1,), g, 2.0 ** -14)[0]
        dy[inner[(5 * n + 2) % len(inner)], n] = _ties((1,), g, 2.0 ** -10)[0]
    return c, x, w, dy


# (taps, (nv, spatial..), cin, cout, seed) of the problems below; the CPU file asserts their three-pattern condition without a GPU
OPS = {"head": (1, (1, 2, 5, 7), 32, 16, 1), "conv27-1": (27, (1, 3, 5, 7), 16, 16, 1), "conv27-2": (27, (1, 3, 5, 7), 16, 16, 2),
       "conv1-1": (1, (1, 2, 5, 7), 32, 16, 11), "conv1-2": (1, (1, 2, 5, 7), 32, 16, 12), "2d-9": (9, (2, 6, 7), 16, 16, 29),
       "2d-1": (1, (2, 6, 7), 16, 16, 21)}


def _problem(key):
    taps, dims, ci, co, seed = OPS[key]
    c, x, w, dy = _ops_problem(taps, dims, ci, co, seed)
    return dims, c, x, w, dy, _patterns(c, x, w, dy)


def _patterns(c, x, w, dy):
    """{format: (y, dx, dw)} in float64 with x, w and dy all in that format (0: as they are, 1: f16, 2: bf16)"""
    out = {}
    for fmt, r in ((0, Q.ident), (1, Q.rne_f16), (2, Q.rne_bf16)):
        xv, wv = r(x).double().requires_grad_(True), r(w).double().requires_grad_(True)
        y = R.conv64(xv, wv, c)
        gx, gw = torch.autograd.grad(y, (xv, wv), r(dy).double())
        out[fmt] = (y.detach(), gx, gw)
    for i in range(3):                                                        # three different bit patterns, each representable
        a, b, e = out[0][i], out[1][i], out[2][i]
        nz = a != 0
        assert int(nz.sum()) >= 16 and all(R.representable(t) for t in (a, b, e))
        assert bool((a[nz] != b[nz]).all()) and float((a[nz] != e[nz]).double().mean()) > 0.9 and float((b[nz] != e[nz]).double().mean()) > 0.9
    return out


def _ops_run(c, x, w, dy, dims):
    from arco_amd import ops
    sp = tuple(dims[1:])
    ci, co, T = c["k"], c["n"], c["taps"]
    k = round(T ** (1.0 / len(sp)))

    def to_map(rows, ch):
        return ops.to_channels_last(rows.view(dims[0], *sp, ch).movedim(-1, 1).contiguous().to(DEV))

    def to_rows(t):
        return t.detach().movedim(1, -1).reshape(-1, t.shape[1]).cpu()

    xi = to_map(x, ci).clone().requires_grad_(True)
    wi = w.view(co, ci, *([k] * len(sp))).to(DEV).clone().requires_grad_(True)
    y = ops.conv(xi, wi, None)
    y.backward(to_map(dy, co))
    torch.cuda.synchronize()
    return to_rows(y), to_rows(xi.grad), wi.grad.detach().reshape(co, ci, T).cpu()


class _switch:
    """ops.HEAD_MMA / ops.CONV_MMA set for a block and put back, the weight packs of the other mode forgotten both ways"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from arco_amd import ops
        self.prev = {k: getattr(ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(ops, k, v)
        ops.bump_weight_epoch()

    def __exit__(self, *exc):
        from arco_amd import ops
        for k, v in self.prev.items():
            setattr(ops, k, v)
        ops.bump_weight_epoch()


def test_head_mma_rounds_the_1x1x1_gemms_of_an_fp32_map():
    """HEAD_MMA = 1 (train_arco_3d --act_dtype f16, --head_mma auto): the forward is the f16 pattern, the data gradient the bf16 pattern
    (dy AND w rounded), the weight gradient the fp32 pattern"""
    dims, c, x, w, dy, pat = _problem("head")
    with _switch(HEAD_MMA=1):
        y, dx, dw = _ops_run(c, x, w, dy, dims)
    assert equal_bits(y, pat[1][0]), "forward: not the f16 pattern"
    assert equal_bits(dx, pat[2][1]), "data gradient: not the bf16 pattern"
    assert equal_bits(dw, pat[0][2]), "weight gradient: not the fp32 pattern"
    with _switch(HEAD_MMA=0):                                                 # and without the switch: fp32 throughout
        y, dx, dw = _ops_run(c, x, w, dy, dims)
    assert equal_bits(y, pat[0][0]) and equal_bits(dx, pat[0][1]) and equal_bits(dw, pat[0][2])


@pytest.mark.parametrize("mode", (1, 2))
def test_conv_mma_rounds_the_3x3x3_convolutions(mode):
    """CONV_MMA = 1 / 2 on a volume (D3 > 1): the forward is the f16 / bf16 pattern, the data gradient bf16, and the weight gradient
    the bf16 route (wgrad_halo2_kernel<.., 2>: both dy and x rounded, as the T4 cases of tests/wgrad_kernel_refs.py define it)"""
    dims, c, x, w, dy, pat = _problem(f"conv27-{mode}")
    with _switch(CONV_MMA=mode, HEAD_MMA=0):
        y, dx, dw = _ops_run(c, x, w, dy, dims)
    assert equal_bits(y, pat[mode][0]), "forward: not the pattern of the mode"
    assert equal_bits(dx, pat[2][1]), "data gradient: not the bf16 pattern"
    assert equal_bits(dw, pat[2][2]), "weight gradient: not the bf16 pattern"


@pytest.mark.parametrize("mode", (1, 2))
def test_conv_mma_rounds_the_1x1x1_convolutions_of_a_volume(mode):
    dims, c, x, w, dy, pat = _problem(f"conv1-{mode}")
    with _switch(CONV_MMA=mode, HEAD_MMA=0):
        y, dx, dw = _ops_run(c, x, w, dy, dims)
    assert equal_bits(y, pat[mode][0]) and equal_bits(dx, pat[2][1]) and equal_bits(dw, pat[0][2])


@pytest.mark.parametrize("taps", (9, 1))
def test_conv_mma_leaves_2d_maps_on_fp32(taps):
    """CONV_MMA = 1 limits the modes to volumes (ops.conv_raw: taps in (1, 27) and d3 > 1): a 2-D 3x3 and a 2-D 1x1 are the fp32
    pattern, forward and both gradients"""
    dims, c, x, w, dy, pat = _problem(f"2d-{taps}")
    with _switch(CONV_MMA=1, HEAD_MMA=0):
        y, dx, dw = _ops_run(c, x, w, dy, dims)
    assert equal_bits(y, pat[0][0]) and equal_bits(dx, pat[0][1]) and equal_bits(dw, pat[0][2])
