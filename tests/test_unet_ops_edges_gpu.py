"""The U-Net operators AROUND the convolutions - nn.MaxPool2d(2) (+ the skip gradient), the align_corners bilinear resize (+ the
in-place concat) and the first layer (3x3 convolution of the fp32 image, <= 4 channels -> 16) - in both storage modes (fp32 and f16
activation storage: csrc/elementwise.hip, the image kernels of csrc/igemm.hip and csrc/wgrad.hip), each against plain PyTorch on the CPU
in float64 on the same input values, at the edges the other operator tests do not reach: tied maxima, operands that are channel
slices of a wider buffer, sides of 1 / identity / downsampling resizes with a random gradient, every channel count and ragged tiles
of the first layer, per-group BatchNorm statistics, and grids large enough for the second trip of the grid-stride loops.

Tolerances are derived, per ELEMENT (never a tensor maximum), u = 2^-24 (fp32), one stored f16 value adds 2^-11 |ref| + 2^-25:
  * pooling: maxima and routed gradients are exact; the sum with the skip gradient is one fp32 rounding (+ one f16 rounding);
  * resize forward: (16 + 4 S) u max|x|, S the largest side - 16 for the four-term lerp, 4 S for coordinates computed as
    scale * index in fp32 (relative error u = up to S u of a pixel; a weight error d moves the result by d (|v0| + |v1|));
    adjoint: the same times n = (2 ceil(Ho / Hi) + 1) (2 ceil(Wo / Wi) + 1), the bound on contributions per input pixel;
  * first layer: (2 (9 K + 1) + 2) u (conv(|x|, |w|) + |b|) per output; weight / bias gradients 2e-5 of the tensor's maximum
    (the rule of tests/test_half2d_gpu.py); BatchNorm batch statistics M u mean|term| with M = NB H W values per group.
tests/test_unet_ops_edges_cpu.py emulates the fp32 arithmetic (+ the one f16 rounding) on the CPU and holds it to the same bounds, so
the bounds are checked on a machine without a GPU.  The helpers up to the first test are shared with that file."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32, U16, SUB16 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
GRID_CAP = 4096 * 256          # ew_grid: at most 4096 workgroups of 256 threads

MODES = ("f", "h")             # fp32 tensors | f16 activation storage


def dtype_of(mode):
    return torch.float16 if mode == "h" else torch.float32


# ---- tolerances ------------------------------------------------------------------------------------------------------------------
def stored_tol(ref, fp32_term, mode):
    """Per-element bound of a stored result: the fp32 term alone (fp32 tensors), + one rounding to f16 (normal and subnormal range)."""
    tol = torch.as_tensor(fp32_term, dtype=torch.float64) + torch.zeros_like(ref)
    if mode == "h":
        tol = tol + U16 * ref.abs() + SUB16
    return tol


def worst(got, ref, tol):
    """max over the elements of |got - ref| / tol."""
    return float(((got.detach().double().cpu() - ref).abs() / tol).max())


def resize_fwd_term(hi, wi, ho, wo, xmax):
    return (16 + 4 * max(hi, wi, ho, wo)) * U32 * xmax


def resize_adj_term(hi, wi, ho, wo, gmax):
    n = (2 * math.ceil(ho / hi) + 1) * (2 * math.ceil(wo / wi) + 1)
    return n * (16 + 4 * max(hi, wi, ho, wo)) * U32 * gmax


def first_layer_term(x64, w64, b64):
    k = int(w64.shape[1])
    mag = F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=1)
    return (2 * (9 * k + 1) + 2) * U32 * mag


def maxrel(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()) / max(1e-30, float(ref.abs().max()))


GRAD_RULE = 2e-5               # first-layer weight / bias gradients: of the tensor's maximum


# ---- inputs and float64 references (computed once, shared, never modified) -----------------------------------------------------------
def nhwc(t):
    """A channels-last copy with explicit strides (also for sides of 1)."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


TIE_VALUES = (-1.5, -0.25, 0.0, 0.0, 0.0, 0.5, 2.0)
POOL_SHAPES = [(1, 8, 2, 2), (3, 8, 6, 10), (2, 24, 4, 6)]                 # (NB, C, H, W), both modes
POOL_SHAPES_F32 = [(2, 4, 4, 6), (2, 12, 6, 4)]                             # channel counts only the fp32 kernels take


def tie_input(seed, nb, c, h, w):
    """f16-representable values drawn from a small set with repeats; window (0, 0) of image 0 holds four equal values (channels 0, 4,
    ...), a mix of -0.0 and +0.0 (channels 1, 5, ...), equal negative values (2, 6, ...) and a maximum that is a tie of -0.0 and
    +0.0 over negative values (3, 7, ...)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(TIE_VALUES, dtype=torch.float32)[torch.randint(0, len(TIE_VALUES), (nb, c, h, w), generator=g)]
    forced = torch.tensor([[[0.5, 0.5], [0.5, 0.5]], [[-0.0, 0.0], [0.0, -0.0]], [[-1.5, -1.5], [-1.5, -1.5]],
                           [[-0.25, -0.0], [0.0, -1.5]]], dtype=torch.float32)
    for ch in range(c):
        x[0, ch, 0:2, 0:2] = forced[ch % 4]
    return x


def tie_share(x):
    """Share of the 2 x 2 windows whose maximum is attained more than once."""
    win = x.unfold(2, 2, 2).unfold(3, 2, 2).reshape(*x.shape[:2], x.shape[2] // 2, x.shape[3] // 2, 4)
    return float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).double().mean())


def pool_ref(x, dy):
    """F.max_pool2d(x, 2) and its autograd gradient (to the first maximum in row-major window order) in float64."""
    xr = x.double().contiguous().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    y.backward(dy.double().contiguous())
    return y.detach(), xr.grad


@functools.lru_cache(maxsize=None)
def pool_case(nb, c, h, w):
    g = torch.Generator().manual_seed(1000 * c + 10 * h + w)
    x = tie_input(7 * c + h, nb, c, h, w)
    dy_int = torch.randint(-64, 64, (nb, c, h // 2, w // 2), generator=g).float() / 8           # exact in f16
    dy = torch.randn((nb, c, h // 2, w // 2), generator=g).half().float()                       # f16-representable
    dskip = torch.randn((nb, c, h, w), generator=g).half().float()
    y, dx_int = pool_ref(x, dy_int)
    _, dx = pool_ref(x, dy)
    return dict(x=x, dy_int=dy_int, dy=dy, dskip=dskip, y=y, dx_int=dx_int, dx_skip=dx + dskip.double())


def skip_sum_tol(ref, mode):
    """routed gradient + skip gradient: one fp32 rounding of the sum, then (f16) one rounding of the stored value."""
    return stored_tol(ref, U32 * ref.abs() + 1e-300, mode)


RESIZE_SHAPES = [(1, 1, 4, 4), (3, 5, 1, 1), (2, 2, 4, 4), (5, 7, 13, 9), (9, 6, 4, 3), (7, 7, 7, 7), (1, 6, 5, 12), (6, 1, 3, 1),
                 (20, 12, 41, 21)]              # (Hi, Wi, Ho, Wo)
RESIZE_CH = (8, 24)


def resize_ref(x, dy, ho, wo):
    xr = x.double().contiguous().requires_grad_(True)
    y = F.interpolate(xr, size=(ho, wo), mode="bilinear", align_corners=True)
    y.backward(dy.double().contiguous())
    return y.detach(), xr.grad


@functools.lru_cache(maxsize=None)
def resize_case(hi, wi, ho, wo, c, nb=2):
    g = torch.Generator().manual_seed(hi * 1000 + wi * 100 + ho * 10 + wo + c)
    x = torch.randn((nb, c, hi, wi), generator=g).half().float()
    dy = torch.randn((nb, c, ho, wo), generator=g).half().float()
    y, dx = resize_ref(x, dy, ho, wo)
    return dict(x=x, dy=dy, y=y, dx=dx, xmax=float(x.abs().max()), gmax=float(dy.abs().max()))


FIRST_K = (1, 2, 3, 4)
FIRST_HW = [(16, 16), (17, 15), (40, 24)]       # exactly one 16 x 16 tile | one pixel over and under the tile side | ragged
NARROW_KN = [(2, 8), (4, 4), (1, 8)]            # (K, N) with N < 16


def conv_ref(x, w, b, dy):
    xr = x.double().contiguous()
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv2d(xr, wr, br, padding=1)
    y.backward(dy.double().contiguous())
    return y.detach(), wr.grad, br.grad


@functools.lru_cache(maxsize=None)
def first_case(k, n, nb, h, w):
    """The fp32 image (NOT rounded to f16: the first layer reads it as it is), fp32 weights, an f16-representable gradient."""
    g = torch.Generator().manual_seed(k * 100000 + n * 1000 + nb * 100 + h + w)
    x = torch.rand((nb, k, h, w), generator=g)
    wt = torch.randn((n, k, 3, 3), generator=g) / 3
    b = torch.randn((n,), generator=g)
    dy = torch.randn((nb, n, h, w), generator=g).half().float()
    y, dw, db = conv_ref(x, wt, b, dy)
    return dict(x=x, w=wt, b=b, dy=dy, y=y, dw=dw, db=db, term=first_layer_term(x.double(), wt.double(), b.double()))


def bn_ref(z, gamma, beta, groups, slope, momentum=0.1, eps=1e-5):
    """Train-mode BatchNorm + LeakyReLU in float64, applied GROUP AFTER GROUP (ops.bn_groups: running statistics updated in that
    order, starting from (0, 1)).  Returns the activation, the running statistics and per group (mean, biased variance, mean|z|,
    mean z^2)."""
    co = int(z.shape[1])
    rm, rv = torch.zeros(co, dtype=torch.float64), torch.ones(co, dtype=torch.float64)
    outs, stats = [], []
    for zg in z.chunk(groups, 0):
        stats.append((zg.mean((0, 2, 3)), zg.var((0, 2, 3), unbiased=False), zg.abs().mean((0, 2, 3)), (zg * zg).mean((0, 2, 3))))
        outs.append(F.leaky_relu(F.batch_norm(zg, rm, rv, gamma.double(), beta.double(), True, momentum, eps), slope))
    return torch.cat(outs), rm, rv, stats


def stat_tols(stats, m, running, dz=None, z=None, groups=1):
    """Bounds of the running mean / variance after one call, per channel: the batch statistics' M u mean|term| (terms z for the mean,
    z^2 for the variance; the largest over the groups - the running statistics are a combination of the groups' with weights that
    sum to less than 1) + 4 u |running| for the fp32 update (1 - momentum) * running + momentum * batch (two products, a sum).  dz: per-element bound of the z that was summed against the reference's z (fp32 tensors: the stored z is
    not the reference's) - its mean adds to the mean's bound, the mean of 2 |z| dz to the variance's."""
    tm = torch.stack([m * U32 * s[2] for s in stats]).max(0).values + 4 * U32 * running[0].abs()
    tv = torch.stack([m * U32 * s[3] for s in stats]).max(0).values + 4 * U32 * running[1].abs()
    if dz is not None:
        tm = tm + torch.stack([d.mean((0, 2, 3)) for d in dz.chunk(groups, 0)]).max(0).values
        tv = tv + torch.stack([(2 * zz.abs() * d).mean((0, 2, 3)) for zz, d in zip(z.chunk(groups, 0), dz.chunk(groups, 0))]).max(0).values
    return tm, tv


def bn_act_term(z, gamma, beta, groups, m, slope, eps=1e-5):
    """fp32 term of a = lrelu((z - mean) * istd * gamma + beta) for the SAME z, per element.  The kernel's mean and variance carry
    dm <= M u mean|z| and dv <= M u mean z^2 + 2 |mean| dm (variance as E z^2 - mean^2); y - beta = (z - mean) * istd * gamma is
    three fp32 operations (3 u relative), istd = rsqrt(var + eps) carries dv / (2 (var + eps)) + 4 u relative, the mean's error
    enters as |gamma| istd dm; the sum with beta and the LeakyReLU's product round once each (2 u |y|)."""
    out = []
    for zg in z.chunk(groups, 0):
        mean, var = zg.mean((0, 2, 3), keepdim=True), zg.var((0, 2, 3), unbiased=False, keepdim=True)
        dm = m * U32 * zg.abs().mean((0, 2, 3), keepdim=True)
        dv = m * U32 * (zg * zg).mean((0, 2, 3), keepdim=True) + 2 * mean.abs() * dm
        istd = (var + eps).rsqrt()
        ga, be = gamma.double().view(1, -1, 1, 1), beta.double().view(1, -1, 1, 1)
        ymb = (zg - mean) * istd * ga
        out.append(ga.abs() * istd * dm + ymb.abs() * (7 * U32 + dv / (2 * (var + eps))) + 2 * U32 * (ymb + be).abs())
    return torch.cat(out)


def large_sides():
    """(rows, columns) whose product exceeds the grid cap by a few percent: with one lane group of channels (8 in f16, 4 in fp32)
    and one image, a map of this size is one work item per pixel."""
    cols = 1024
    rows = GRID_CAP // cols + 16
    return rows, cols


# ---- GPU plumbing ------------------------------------------------------------------------------------------------------------------
def dev(t, mode):
    return nhwc(t.to(DEV).to(dtype_of(mode)))


def wide(t, mode, sentinel):
    """t as the LEADING channel block of a channels-last buffer twice as wide (row stride 2 C), the trailing block = sentinel."""
    nb, c, h, w = t.shape
    buf = torch.full((nb, h, w, 2 * c), sentinel, dtype=dtype_of(mode), device=DEV).permute(0, 3, 1, 2)
    buf[:, :c].copy_(t)
    return buf


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def exact(got, ref):
    return torch.equal(got.detach().double().cpu(), ref)


# ---- 1. max-pool ties ----------------------------------------------------------------------------------------------------------------
def _pool_params():
    return [(m, s) for m in MODES for s in POOL_SHAPES] + [("f", s) for s in POOL_SHAPES_F32]


def _run_pool(ops, mode, case, strided):
    """maxpool2 forward / backward (integer / 8 gradients) and maxpool2_skip backward (random gradients) on `case`; strided: x and the
    skip gradient are the leading channel blocks of buffers twice as wide.  Returns what the kernels wrote and the guard blocks."""
    c = case["x"].shape[1]
    guards = []

    def operand(t, sentinel):
        if not strided:
            return dev(t, mode)
        buf = wide(t, mode, sentinel)
        guards.append((buf[:, c:], buf[:, c:].clone()))
        return buf[:, :c]

    x = operand(case["x"], 777.0).detach().requires_grad_(True)
    y = ops.maxpool2(x)
    assert y.dtype == dtype_of(mode)
    y.backward(dev(case["dy_int"], mode))
    x2 = operand(case["x"], 555.0).detach().requires_grad_(True)
    y2, skip = ops.maxpool2_skip(x2)
    torch.autograd.backward([y2, skip], [dev(case["dy"], mode), operand(case["dskip"], -333.0)])
    assert x.grad.dtype == dtype_of(mode) and x2.grad.dtype == dtype_of(mode)
    return y, x.grad, y2, x2.grad, guards


def _check_pool(mode, case, y, dx, y2, dx2, tag):
    assert exact(y, case["y"]) and exact(y2, case["y"]), tag               # the maximum, exactly
    assert exact(dx, case["dx_int"]), tag                                   # routed to the first maximum in row-major window order
    e = worst(dx2, case["dx_skip"], skip_sum_tol(case["dx_skip"], mode))
    print(f"{tag}: routed + skip gradient err/tol {e:.3f}")
    assert e <= 1.0, (tag, e)


@pytest.mark.parametrize("mode,shape", _pool_params())
def test_maxpool_ties_route_to_the_first_maximum(mode, shape):
    from arco_amd import ops
    case = pool_case(*shape)
    share = tie_share(case["x"])
    print(f"maxpool ties {mode} {shape}: tie share {share:.3f}")
    assert share > 0.2
    y, dx, y2, dx2, _ = _run_pool(ops, mode, case, strided=False)
    _check_pool(mode, case, y, dx, y2, dx2, f"maxpool ties {mode} {shape}")


# ---- 2. pooling on strided operands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape", _pool_params())
def test_maxpool_on_channel_slices_of_a_wider_buffer(mode, shape):
    from arco_amd import ops
    case = pool_case(*shape)
    y, dx, y2, dx2, guards = _run_pool(ops, mode, case, strided=True)
    _check_pool(mode, case, y, dx, y2, dx2, f"maxpool ld=2C {mode} {shape}")
    assert len(guards) == 3
    for now, before in guards:
        assert same_bits(now, before)              # the trailing channels of the buffers are untouched


@pytest.mark.parametrize("mode", MODES)
def test_pooled_stage_output_and_gradient_route(mode, monkeypatch):
    """conv_bn_act(pool=True, cat_room=co): fp32 - the fused arco_bn_act_pool_fwd; f16 - apply, then arco_maxpool2_fwd_h on the
    activation inside the concat buffer (ld = 2 co).  ReLU (slope 0), so the stored activation holds exact zeros and its windows tie.
    The gradient that enters the BatchNorm backward is da + (dpool routed by torch on the STORED activation): integers / 8, exact."""
    from arco_amd import ops
    g = torch.Generator().manual_seed(21)
    nb, ci, co, h, w = 2, 16, 16, 12, 20
    x = torch.randn((nb, ci, h, w), generator=g).half().float()
    wt = (torch.randn((co, ci, 3, 3), generator=g) / 12).half().float().to(DEV).requires_grad_(True)
    b = torch.zeros(co, device=DEV, requires_grad=True)
    gamma = torch.rand(co, generator=g).add(0.5).to(DEV).requires_grad_(True)
    beta = torch.randn(co, generator=g).mul(0.2).to(DEV).requires_grad_(True)
    da = torch.randint(-64, 64, (nb, co, h, w), generator=g).float() / 8
    dp = torch.randint(-64, 64, (nb, co, h // 2, w // 2), generator=g).float() / 8
    rm, rv = torch.zeros(co, device=DEV), torch.ones(co, device=DEV)
    seen = []
    inner = ops._bn_backward
    monkeypatch.setattr(ops, "_bn_backward", lambda d, *a, **k: (seen.append(d.detach().clone()), inner(d, *a, **k))[1])
    xg = dev(x, mode).requires_grad_(True)
    a, pooled = ops.conv_bn_act(xg, wt, b, gamma, beta, rm, rv, slope=0.0, p=0.0, cat_room=co, pool=True)
    buf = a._arco_cat_buf
    assert a.dtype == pooled.dtype == dtype_of(mode) and buf.shape[1] == 2 * co and buf.data_ptr() == a.data_ptr()
    a64 = a.detach().double().cpu()
    share = tie_share(a64)
    print(f"pooled stage {mode}: tie share of the stored activation {share:.3f}")
    assert share > 0.02                            # all-negative windows (1 / 16 of them) tie at zero
    assert exact(pooled, F.max_pool2d(a64, 2))
    torch.autograd.backward([a, pooled], [dev(da, mode), dev(dp, mode)])
    assert len(seen) == 1
    _, routed = pool_ref(a64, dp)
    assert exact(seen[0], da.double() + routed)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape", [(m, s) for m in MODES for s in ((1, 8, 3, 4), (1, 8, 4, 5))] +
                         [("h", (1, 4, 4, 4)), ("h", (2, 12, 2, 6))])
def test_maxpool_refuses_odd_sides_and_partial_lane_groups(mode, shape):
    """Argument checks of the entry points (they return before any launch): an odd side in both modes, a channel count that is not a
    multiple of 8 in f16."""
    from arco_amd import ops
    x = dev(torch.zeros(shape), mode)
    with pytest.raises(RuntimeError, match="arco_maxpool2_fwd"):
        ops.maxpool2(x)


# ---- 4. resize ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RESIZE_CH)
@pytest.mark.parametrize("shape", RESIZE_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_resize_forward_and_adjoint(mode, shape, c):
    from arco_amd import ops
    hi, wi, ho, wo = shape
    case = resize_case(hi, wi, ho, wo, c)
    x = dev(case["x"], mode).requires_grad_(True)
    y = ops.bilinear(x, (ho, wo))
    assert y.dtype == dtype_of(mode) and tuple(y.shape) == (2, c, ho, wo)
    y.backward(dev(case["dy"], mode))
    ef = worst(y, case["y"], stored_tol(case["y"], resize_fwd_term(hi, wi, ho, wo, case["xmax"]), mode))
    eb = worst(x.grad, case["dx"], stored_tol(case["dx"], resize_adj_term(hi, wi, ho, wo, case["gmax"]), mode))
    print(f"resize {mode} {hi}x{wi} -> {ho}x{wo} c={c}: forward err/tol {ef:.3f}  adjoint err/tol {eb:.3f}")
    assert ef <= 1.0 and eb <= 1.0, (ef, eb)


@pytest.mark.parametrize("c,h,w", [(8, 5, 3), (24, 2, 6)])
@pytest.mark.parametrize("mode", MODES)
def test_upcat_writes_only_its_half_of_the_buffer(mode, c, h, w):
    """cat([skip, bilinear_x2(x)]) in place behind the skip: the concat buffer is images 1, 2 of a 4-image tensor, so one sentinel
    image lies right before it and one right behind it."""
    from arco_amd import ops
    case = resize_case(h, w, 2 * h, 2 * w, c)
    g = torch.Generator().manual_seed(c + h)
    skip_v = torch.randn((2, c, 2 * h, 2 * w), generator=g).half().float()
    dcat = torch.randn((2, 2 * c, 2 * h, 2 * w), generator=g).half().float()
    big = torch.full((4, 2 * h, 2 * w, 2 * c), 4242.0, dtype=dtype_of(mode), device=DEV).permute(0, 3, 1, 2)
    buf = big[1:3]
    buf[:, :c].copy_(skip_v)
    before = big.clone()
    skip = buf[:, :c].detach().requires_grad_(True)
    skip._arco_cat_buf = buf
    x = dev(case["x"], mode).requires_grad_(True)
    cat = ops.upcat(x, skip)
    assert cat.dtype == dtype_of(mode) and cat.data_ptr() == buf.data_ptr()           # in place
    cat.backward(dev(dcat, mode))
    assert same_bits(big[0], before[0]) and same_bits(big[3], before[3])               # the guards
    assert same_bits(big[1:3, :c], before[1:3, :c])                                    # the skip half
    _, dx = resize_ref(case["x"], dcat[:, c:], 2 * h, 2 * w)
    ef = worst(cat[:, c:], case["y"], stored_tol(case["y"], resize_fwd_term(h, w, 2 * h, 2 * w, case["xmax"]), mode))
    eb = worst(x.grad, dx, stored_tol(dx, resize_adj_term(h, w, 2 * h, 2 * w, float(dcat.abs().max())), mode))
    print(f"upcat {mode} c={c} {h}x{w}: forward err/tol {ef:.3f}  adjoint err/tol {eb:.3f}")
    assert ef <= 1.0 and eb <= 1.0, (ef, eb)
    assert exact(skip.grad, dcat[:, :c].double())                                      # the skip's gradient is a slice


# ---- 5. first layer ---------------------------------------------------------------------------------------------------------------------
def _first_layer(ops, mode, case):
    x = nhwc(case["x"].to(DEV))
    wt, b = case["w"].to(DEV).requires_grad_(True), case["b"].to(DEV).requires_grad_(True)
    with ops.open_half(mode == "h"):
        y = ops.conv(x, wt, b)
    assert y.dtype == dtype_of(mode)
    y.backward(dev(case["dy"], mode))
    return y.detach(), wt.grad, b.grad


def _check_first_layer(mode, case, y, dw, db, tag):
    ey = worst(y, case["y"], stored_tol(case["y"], case["term"], mode))
    ew, eb = maxrel(dw, case["dw"]), maxrel(db, case["db"])
    print(f"{tag}: output err/tol {ey:.3f}  dW {ew:.2e}  db {eb:.2e}  (rule {GRAD_RULE:.0e})")
    assert ey <= 1.0, (tag, ey)
    assert ew < GRAD_RULE and eb < GRAD_RULE, (tag, ew, eb)


@pytest.mark.parametrize("hw", FIRST_HW)
@pytest.mark.parametrize("k", FIRST_K)
@pytest.mark.parametrize("mode", MODES)
def test_first_layer_every_channel_count_and_ragged_tiles(mode, k, hw):
    from arco_amd import ops
    case = first_case(k, 16, 2, *hw)
    _check_first_layer(mode, case, *_first_layer(ops, mode, case), f"first layer {mode} K={k} {hw[0]}x{hw[1]}")


@pytest.mark.parametrize("k,n", NARROW_KN)
def test_first_layer_below_16_outputs(k, n):
    """The f16 first layer exists for 16 output channels: its weight-gradient kernel reads 16 channels of the gradient.  A forward
    with fewer is refused in ops, with a message that says so, before anything is launched - it is never followed by a backward
    that raises.  The fp32 route accepts the same layer and its gradients meet the rule."""
    from arco_amd import ops
    case = first_case(k, n, 2, 17, 15)
    x = nhwc(case["x"].to(DEV))
    wt, b = case["w"].to(DEV).requires_grad_(True), case["b"].to(DEV).requires_grad_(True)
    with ops.open_half(True), pytest.raises(RuntimeError, match="16 channels"):
        ops.conv(x, wt, b)
    gamma, beta = torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    with ops.open_half(True), pytest.raises(RuntimeError, match="16 channels"):
        ops.conv_bn_act(x, wt, b, gamma, beta, torch.zeros(n, device=DEV), torch.ones(n, device=DEV))
    _check_first_layer("f", case, *_first_layer(ops, "f", case), f"first layer f K={k} N={n} 17x15")


@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("mode", MODES)
def test_first_layer_batchnorm_statistics_per_group(mode, k, groups):
    """conv_bn_act on the first layer at 17 x 15 (two ragged tiles per image), one statistic slab set per group.  The running
    statistics after one call against float64 BatchNorm applied group after group to the float64 convolution (f16: rounded to f16
    first - statistics of the rounded outputs).  The activation against the same BatchNorm of the z the convolution kernel STORES
    (ops.conv on the same operands; itself held to float64 here): a z that rounds the other way in fp32 than in float64 is the
    convolution's one allowed rounding, not an error of the normalisation."""
    from arco_amd import ops
    nb, h, w, slope = 2 * groups, 17, 15, 0.01
    m = nb // groups * h * w
    case = first_case(k, 16, nb, h, w)
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand(16, generator=g).add(0.5), torch.randn(16, generator=g).mul(0.2)
    x, wt, b = nhwc(case["x"].to(DEV)), case["w"].to(DEV), case["b"].to(DEV)
    rm, rv = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    with ops.open_half(mode == "h"), ops.bn_groups(groups):
        a = ops.conv_bn_act(x, wt, b, gamma.to(DEV), beta.to(DEV), rm, rv, slope=slope, p=0.0, num_batches_tracked=nbt)
    with ops.open_half(mode == "h"):
        z = ops.conv(x, wt, b)
    assert a.dtype == z.dtype == dtype_of(mode) and int(nbt) == groups
    ztol = stored_tol(case["y"], case["term"], mode)
    ez = worst(z, case["y"], ztol)
    z_ref = case["y"].half().double() if mode == "h" else case["y"]
    _, rm_ref, rv_ref, stats = bn_ref(z_ref, gamma, beta, groups, slope)
    tm, tv = stat_tols(stats, m, (rm_ref, rv_ref), **({} if mode == "h" else dict(dz=ztol, z=z_ref, groups=groups)))
    em, ev = worst(rm, rm_ref, tm), worst(rv, rv_ref, tv)
    z64 = z.double().cpu()
    a_ref, _, _, _ = bn_ref(z64, gamma, beta, groups, slope)
    ea = worst(a, a_ref, stored_tol(a_ref, bn_act_term(z64, gamma, beta, groups, m, slope), mode))
    print(f"first-layer BN {mode} K={k} groups={groups}: z err/tol {ez:.3f}  running mean {em:.3f}  running var {ev:.3f}  activation {ea:.3f}")
    assert ez <= 1.0 and em <= 1.0 and ev <= 1.0 and ea <= 1.0, (ez, em, ev, ea)


# ---- 6. large grids: the second trip of the grid-stride loops ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_large_grid_maxpool(mode):
    """One lane group of channels, one image, 2080 x 2048: 1040 x 1024 windows = work items, more than 4096 x 256.  Forward,
    backward and backward + skip; the reference is float32 on the CPU (maxima and routes are exact in any precision)."""
    from arco_amd import ops
    c = 8 if mode == "h" else 4
    ho, wo = large_sides()
    items = ho * wo * (c // (8 if mode == "h" else 4))
    print(f"large grid maxpool {mode}: {items} items, cap {GRID_CAP} ({items / GRID_CAP:.3f} x)")
    assert items > GRID_CAP
    g = torch.Generator().manual_seed(5)
    x = torch.tensor(TIE_VALUES)[torch.randint(0, len(TIE_VALUES), (1, c, 2 * ho, 2 * wo), generator=g)]
    dy = torch.randint(-64, 64, (1, c, ho, wo), generator=g).float() / 8
    dskip = torch.randint(-64, 64, (1, c, 2 * ho, 2 * wo), generator=g).float() / 8       # sums exact in f16 and fp32
    xr = x.clone().requires_grad_(True)
    y_ref = F.max_pool2d(xr, 2)
    y_ref.backward(dy)
    xg = dev(x, mode).requires_grad_(True)
    y = ops.maxpool2(xg)
    y.backward(dev(dy, mode))
    assert torch.equal(y.detach().float().cpu(), y_ref.detach())
    assert torch.equal(xg.grad.float().cpu(), xr.grad)
    x2 = dev(x, mode).requires_grad_(True)
    y2, skip = ops.maxpool2_skip(x2)
    torch.autograd.backward([y2, skip], [dev(dy, mode), dev(dskip, mode)])
    assert torch.equal(y2.detach().float().cpu(), y_ref.detach())
    assert torch.equal(x2.grad.float().cpu(), xr.grad + dskip)


@functools.lru_cache(maxsize=None)
def _large_resize_case(c, up):
    ho, wo = large_sides()
    hi, wi = ho // 2, wo // 2
    if not up:
        hi, wi, ho, wo = ho, wo, hi, wi
    g = torch.Generator().manual_seed(31 + c + up)
    x = torch.randn((1, c, hi, wi), generator=g).half().float()
    dy = torch.randn((1, c, ho, wo), generator=g).half().float()
    y, dx = resize_ref(x, dy, ho, wo)
    return dict(x=x, dy=dy, y=y, dx=dx, xmax=float(x.abs().max()), gmax=float(dy.abs().max()), shape=(hi, wi, ho, wo))


@pytest.mark.parametrize("mode", MODES)
def test_large_grid_resize_forward(mode):
    """520 x 512 -> 1040 x 1024, one lane group of channels: one work item per OUTPUT pixel."""
    from arco_amd import ops
    c = 8 if mode == "h" else 4
    case = _large_resize_case(c, True)
    hi, wi, ho, wo = case["shape"]
    items = ho * wo
    print(f"large grid resize forward {mode}: {items} items, cap {GRID_CAP} ({items / GRID_CAP:.3f} x)")
    assert items > GRID_CAP
    with torch.no_grad():
        y = ops.bilinear(dev(case["x"], mode), (ho, wo))
    e = worst(y, case["y"], stored_tol(case["y"], resize_fwd_term(hi, wi, ho, wo, case["xmax"]), mode))
    print(f"  forward err/tol {e:.3f}")
    assert e <= 1.0, e


@pytest.mark.parametrize("mode", MODES)
def test_large_grid_resize_adjoint(mode):
    """1040 x 1024 -> 520 x 512: the adjoint has one work item per INPUT pixel."""
    from arco_amd import ops
    c = 8 if mode == "h" else 4
    case = _large_resize_case(c, False)
    hi, wi, ho, wo = case["shape"]
    items = hi * wi
    print(f"large grid resize adjoint {mode}: {items} items, cap {GRID_CAP} ({items / GRID_CAP:.3f} x)")
    assert items > GRID_CAP
    x = dev(case["x"], mode).requires_grad_(True)
    ops.bilinear(x, (ho, wo)).backward(dev(case["dy"], mode))
    e = worst(x.grad, case["dx"], stored_tol(case["dx"], resize_adj_term(hi, wi, ho, wo, case["gmax"]), mode))
    print(f"  adjoint err/tol {e:.3f}")
    assert e <= 1.0, e
