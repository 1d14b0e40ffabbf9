"""CPU companion of tests/test_unet_ops_edges_gpu.py: the bounds that file holds the HIP kernels to are checked here WITHOUT a GPU.
The kernels' arithmetic - fp32 coordinates, weights and sums, one rounding to f16 per stored value - is emulated with torch on the
CPU for the same cases and inputs and must stay inside the same per-element bounds against the same float64 references
(err / tol <= 1).  A bound that only a correct kernel's ordinary rounding could break would show here first.  The inputs of the tie
cases must really tie."""
import pytest
import torch
import torch.nn.functional as F

import test_unet_ops_edges_gpu as E


def _round(t, mode):
    return t.half().float() if mode == "h" else t


def _ac_src(n_out, n_in):
    """ac_src of csrc/interp.h in fp32: src = scale * index, i0 = (int)src clamped, i1 = i0 + 1 clamped, l1 = src - i0."""
    one = torch.ones((), dtype=torch.float32)
    scale = (one * (n_in - 1)) / (one * (n_out - 1)) if n_out > 1 else torch.zeros((), dtype=torch.float32)
    src = scale * torch.arange(n_out, dtype=torch.float32)
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, src - i0.float()


def emulate_resize(x, ho, wo, mode):
    """bilinear_fwd_kernel<T, V>: hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11) in fp32.  The kernel forms it with bl_blend1,
    fma(ly, fma(lx, v11, hx * v10), hy * fma(lx, v01, hx * v00)), for both storage types; here every operation rounds."""
    y0, y1, ly = _ac_src(ho, x.shape[2])
    x0, x1, lx = _ac_src(wo, x.shape[3])
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    hy, hx = 1.0 - ly, 1.0 - lx
    v = lambda yy, xx: x[:, :, yy][:, :, :, xx]
    return _round(hy * (hx * v(y0, x0) + lx * v(y0, x1)) + ly * (hx * v(y1, x0) + lx * v(y1, x1)), mode)


def _adjoint_weights(n_out, n_in):
    """[n_out, n_in] fp32: what output index o contributes to input index i (the kernels add (1 - l) for i0 == i and l for i1 == i)."""
    i0, i1, l = _ac_src(n_out, n_in)
    wgt = torch.zeros((n_out, n_in), dtype=torch.float32)
    o = torch.arange(n_out)
    wgt.index_put_((o, i0), 1.0 - l, accumulate=True)
    wgt.index_put_((o, i1), l, accumulate=True)
    return wgt


def emulate_resize_adjoint(dy, hi, wi, mode):
    """bilinear_bwd_kernel<T, V>: dx[yi, xi] = sum wy * wx * dy[yo, xo] in fp32 (here: rows, then columns)."""
    wy, wx = _adjoint_weights(dy.shape[2], hi), _adjoint_weights(dy.shape[3], wi)
    return _round(torch.einsum("pi,ncpj->ncij", wy, torch.einsum("qj,ncpq->ncpj", wx, dy)), mode)


RESIZE_PARAMS = [(s, c) for s in E.RESIZE_SHAPES for c in E.RESIZE_CH] + [((16, 16, 32, 32), 8), ((130, 128, 260, 256), 8)]


@pytest.mark.parametrize("shape,c", RESIZE_PARAMS)
@pytest.mark.parametrize("mode", E.MODES)
def test_resize_bounds_hold_for_the_emulated_kernels(mode, shape, c):
    hi, wi, ho, wo = shape
    case = E.resize_case(hi, wi, ho, wo, c)
    ef = E.worst(emulate_resize(case["x"], ho, wo, mode), case["y"],
                 E.stored_tol(case["y"], E.resize_fwd_term(hi, wi, ho, wo, case["xmax"]), mode))
    eb = E.worst(emulate_resize_adjoint(case["dy"], hi, wi, mode), case["dx"],
                 E.stored_tol(case["dx"], E.resize_adj_term(hi, wi, ho, wo, case["gmax"]), mode))
    print(f"emulated resize {mode} {hi}x{wi} -> {ho}x{wo} c={c}: forward err/tol {ef:.3f}  adjoint err/tol {eb:.3f}")
    assert ef <= 1.0 and eb <= 1.0, (ef, eb)


def _emulate_first_layer(case, mode):
    x, w, b = case["x"], case["w"].clone().requires_grad_(True), case["b"].clone().requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)                # fp32 products and sums
    y.backward(case["dy"])
    return _round(y.detach(), mode), w.grad, b.grad


@pytest.mark.parametrize("hw", E.FIRST_HW)
@pytest.mark.parametrize("k,n", [(k, 16) for k in E.FIRST_K] + E.NARROW_KN)
@pytest.mark.parametrize("mode", E.MODES)
def test_first_layer_bounds_hold_for_the_emulated_kernels(mode, k, n, hw):
    case = E.first_case(k, n, 2, *hw)
    y, dw, db = _emulate_first_layer(case, mode)
    ey = E.worst(y, case["y"], E.stored_tol(case["y"], case["term"], mode))
    ew, eb = E.maxrel(dw, case["dw"]), E.maxrel(db, case["db"])
    print(f"emulated first layer {mode} K={k} N={n} {hw}: output err/tol {ey:.3f}  dW {ew:.2e}  db {eb:.2e}")
    assert ey <= 1.0 and ew < E.GRAD_RULE and eb < E.GRAD_RULE, (ey, ew, eb)


@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("mode", E.MODES)
def test_first_layer_statistic_bounds_hold_for_the_emulated_kernels(mode, k, groups):
    """Per-group sums of z and z^2 in fp32 over the fp32 convolution's (rounded) outputs, the running statistics updated group after
    group, against float64 BatchNorm of the float64 convolution (f16: rounded): covers outputs that round the other way in fp32; then
    the activation in fp32 against float64 BatchNorm of the same z."""
    nb, h, w, slope = 2 * groups, 17, 15, 0.01
    m = nb // groups * h * w
    case = E.first_case(k, 16, nb, h, w)
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand(16, generator=g).add(0.5), torch.randn(16, generator=g).mul(0.2)
    z, _, _ = _emulate_first_layer(case, mode)
    rm, rv, acts = torch.zeros(16, dtype=torch.float64), torch.ones(16, dtype=torch.float64), []
    for zg in z.chunk(groups, 0):
        s, q = zg.sum((0, 2, 3)).double(), (zg * zg).sum((0, 2, 3)).double()
        mean, var = s / m, q / m - (s / m) ** 2
        rm, rv = 0.9 * rm + 0.1 * mean, 0.9 * rv + 0.1 * var * m / (m - 1)
        mu, istd = mean.float().view(1, -1, 1, 1), (var + 1e-5).rsqrt().float().view(1, -1, 1, 1)
        y = (zg - mu) * istd * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        acts.append(_round(torch.where(y >= 0, y, y * slope), mode))
    ztol = E.stored_tol(case["y"], case["term"], mode)
    z_ref = case["y"].half().double() if mode == "h" else case["y"]
    _, rm_ref, rv_ref, stats = E.bn_ref(z_ref, gamma, beta, groups, slope)
    tm, tv = E.stat_tols(stats, m, (rm_ref, rv_ref), **({} if mode == "h" else dict(dz=ztol, z=z_ref, groups=groups)))
    em, ev = E.worst(rm, rm_ref, tm), E.worst(rv, rv_ref, tv)
    z64 = z.double()
    a_ref, _, _, _ = E.bn_ref(z64, gamma, beta, groups, slope)
    ea = E.worst(torch.cat(acts), a_ref, E.stored_tol(a_ref, E.bn_act_term(z64, gamma, beta, groups, m, slope), mode))
    print(f"emulated first-layer BN {mode} K={k} groups={groups}: running mean {em:.3f}  running var {ev:.3f}  activation {ea:.3f}")
    assert em <= 1.0 and ev <= 1.0 and ea <= 1.0, (em, ev, ea)


@pytest.mark.parametrize("shape", E.POOL_SHAPES + E.POOL_SHAPES_F32)
def test_tie_inputs_tie(shape):
    case = E.pool_case(*shape)
    x = case["x"]
    share = E.tie_share(x)
    print(f"tie share {shape}: {share:.3f}")
    assert share > 0.2
    assert torch.equal(x, x.half().float())                                        # f16-representable
    win = x[0, :4, 0:2, 0:2].reshape(4, 4)                                         # the forced windows of channels 0 ... 3
    assert bool((win[0] == win[0, 0]).all()) and bool((win[1] == 0).all())
    assert bool(torch.signbit(win[1]).any()) and not bool(torch.signbit(win[1]).all())     # -0.0 and +0.0 in one window
    # torch routes a tie to the first maximum in row-major window order, -0.0 == +0.0 included: the routed gradient of the forced
    # windows sits on element 0 (equal values), 0 (zeros), 0 (equal negatives) and 1 (-0.0 before +0.0 over negatives)
    ones = torch.ones_like(case["dy_int"])
    _, route = E.pool_ref(x, ones)
    first = route[0, :4, 0:2, 0:2].reshape(4, 4).argmax(1).tolist()
    assert first == [0, 0, 0, 1], first
    # integer / 8 gradients: exact in f16, and so is their sum with another such value
    assert torch.equal(case["dy_int"], case["dy_int"].half().float())
