"""f16 ACTIVATION STORAGE of the 2-D path (train_arco_2d --act_dtype f16; csrc/conv_h.hip's 2-D dispatch, the _Float16 kernels of csrc/elementwise.hip, the *_h
entry points) against the fp32 kernels of the same operators AND float64 PyTorch on the CPU, on the SAME f16-representable inputs -
the convention of tests/test_half_gpu.py: products of f16 values are exact in fp32 and accumulation is fp32 in both, so what differs
is one rounding of each stored result (2^-11 relative): stored results are held to 1e-3 of the tensor's maximum, fp32 weight / bias
gradients (exact products, another summation order) to 2e-5.  Reference operators: nn.Conv2d / BatchNorm2d / LeakyReLU / Dropout /
MaxPool2d / Upsample(bilinear, align_corners) of unetWithArgs.py:31-85.
The per-element float64 anchor of the 3x3 / 1x1 forward and data-gradient kernels, route by route, lives in tests/test_hconv_kernels_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rand_act(rs, shape, scale=1.0):
    x = torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).to(DEV)
    return _cl(x.half())            # f16-representable values, channels-last


def _maxrel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / max(1e-12, float(b.double().abs().max()))


def _l2rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(1e-20, float(b.double().norm()))


def _torch_conv_ref(x, w, b, dy):
    """Plain PyTorch on the CPU, float64, same operands: (y, dx, dw, db) of nn.Conv2d(3, padding=1)."""
    import torch.nn.functional as F
    xr = x.detach().cpu().double().contiguous().requires_grad_(True)
    wr = w.detach().cpu().double().requires_grad_(True)
    br = b.detach().cpu().double().requires_grad_(True)
    y = F.conv2d(xr, wr, br, padding=1)
    y.backward(dy.detach().cpu().double().contiguous())
    return y.detach(), xr.grad, wr.grad, br.grad


# (ci, co, NB, H, W): every 3x3 of UNet(1, 4) at 256 x 256 (ConvBlock stages, the concatenated inputs of the UpBlocks, out_conv
# 16 -> 4), out_conv at 19 classes, one Cityscapes-shaped map, one map whose sides are not multiples of the tile
CONV_SHAPES = [(16, 16, 2, 256, 256), (32, 16, 2, 256, 256), (16, 4, 2, 256, 256),
               (16, 32, 2, 128, 128), (32, 32, 2, 128, 128), (64, 32, 2, 128, 128),
               (32, 64, 2, 64, 64), (64, 64, 2, 64, 64), (128, 64, 2, 64, 64),
               (64, 128, 2, 32, 32), (128, 128, 2, 32, 32), (256, 128, 2, 32, 32),
               (128, 256, 2, 16, 16), (256, 256, 2, 16, 16), (512, 256, 2, 16, 16),
               (16, 19, 2, 64, 128), (16, 16, 1, 512, 1024), (32, 32, 2, 40, 24), (64, 64, 3, 24, 40)]


@pytest.mark.parametrize("ci,co,nb,H,W", CONV_SHAPES)
def test_conv3x3_f16_storage_forward_backward(ci, co, nb, H, W):
    from arco_amd import ops
    rs = np.random.RandomState(ci + co + W)
    x16 = _rand_act(rs, (nb, ci, H, W))
    w = torch.from_numpy((rs.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(np.float32)).to(DEV)
    w = w.half().float().requires_grad_(True)              # f16-representable weights: the f16 pack is then exact
    b = torch.from_numpy(rs.standard_normal(co).astype(np.float32)).to(DEV).requires_grad_(True)
    dy16 = _rand_act(rs, (nb, co, H, W))
    outs = {}
    for mode in ("h", "f"):
        x = (x16 if mode == "h" else x16.float()).clone().requires_grad_(True)
        w.grad = b.grad = None
        y = ops.conv(x, w, b)
        assert y.dtype == (torch.float16 if mode == "h" else torch.float32)
        y.backward(dy16 if mode == "h" else dy16.float())
        assert x.grad.dtype == x.dtype and w.grad.dtype == torch.float32
        outs[mode] = (y.detach().float(), x.grad.float(), w.grad.clone(), b.grad.clone())
    ref = _torch_conv_ref(x16, w, b, dy16)
    for k, (name, tol) in enumerate((("y", 1e-3), ("dx", 1e-3), ("dw", 2e-5), ("db", 2e-5))):
        e_f, e_t = _maxrel(outs["h"][k], outs["f"][k]), _maxrel(outs["h"][k], ref[k])
        print(f"conv3x3 {ci}->{co} {nb}x{H}x{W} {name}: vs fp32 kernel {e_f:.3e}  vs float64 torch {e_t:.3e}")
        assert e_f < tol, (name, e_f)
        assert e_t < tol, (name, e_t)


@pytest.mark.parametrize("in_chns,H,W", [(1, 64, 48), (3, 64, 48), (3, 40, 24), (1, 256, 256)])
def test_first_layer_reads_the_fp32_image_and_opens_the_f16_region(in_chns, H, W):
    """unetWithArgs.py:101 in_conv: the fp32 image (1 / 3 channels) -> 16 channels stored as f16, and its weight gradient from the f16
    gradient and the fp32 image.  The image is NOT rounded: the fp32 kernel on the same image is the reference."""
    from arco_amd import ops
    rs = np.random.RandomState(5 + in_chns)
    x = _cl(torch.from_numpy(rs.uniform(size=(2, in_chns, H, W)).astype(np.float32)).to(DEV))
    w = torch.from_numpy((rs.standard_normal((16, in_chns, 3, 3)) / 3).astype(np.float32)).to(DEV).requires_grad_(True)
    b = torch.from_numpy(rs.standard_normal(16).astype(np.float32)).to(DEV).requires_grad_(True)
    dy16 = _rand_act(rs, (2, 16, H, W))
    outs = {}
    for half in (True, False):
        w.grad = b.grad = None
        with ops.open_half(half):
            y = ops.conv(x, w, b)
        assert y.dtype == (torch.float16 if half else torch.float32)
        y.backward(dy16 if half else dy16.float())
        outs[half] = (y.detach().float(), w.grad.clone(), b.grad.clone())
    assert not ops.use_half(x, 9, in_chns)           # the switch does not outlive the `with`
    ref = _torch_conv_ref(x, w, b, dy16)
    for k, rk, tol in ((0, 0, 1e-3), (1, 2, 2e-5), (2, 3, 2e-5)):
        e_f, e_t = _maxrel(outs[True][k], outs[False][k]), _maxrel(outs[True][k], ref[rk])
        print(f"first layer in_chns={in_chns} {H}x{W} [{k}]: vs fp32 kernel {e_f:.3e}  vs float64 torch {e_t:.3e}")
        assert e_f < tol and e_t < tol, (k, e_f, e_t)


def _distinct_in_windows(rs, nb, c, H, W):
    """f16-representable values without ties inside any 2 x 2 window: a per-position offset in {0, 8, 16, 24} + small noise."""
    base = torch.from_numpy(rs.standard_normal((nb, c, H, W)).astype(np.float32))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    slot = ((yy % 2) * 2 + (xx % 2)).float()
    perm = torch.from_numpy(rs.permutation(4).astype(np.float32))
    x = base.clamp(-3, 3) + 8.0 * perm[slot.long()]
    return _cl(x.to(DEV).half())


@pytest.mark.parametrize("c,H,W", [(16, 64, 48), (32, 32, 32), (256, 4, 6)])
def test_maxpool2_f16_equals_the_fp32_kernels_exactly(c, H, W):
    """nn.MaxPool2d(2) forward, backward and backward + skip gradient: a maximum and a routed value need no rounding.  The gradients
    are small integers / 8, so the sum with the skip gradient is exact in f16 as well."""
    from arco_amd import ops
    rs = np.random.RandomState(c + H)
    x16 = _distinct_in_windows(rs, 2, c, H, W)
    dy16 = _cl(torch.from_numpy(rs.randint(-64, 64, (2, c, H // 2, W // 2)).astype(np.float32) / 8).to(DEV).half())
    ds16 = _cl(torch.from_numpy(rs.randint(-64, 64, (2, c, H, W)).astype(np.float32) / 8).to(DEV).half())
    res = {}
    for mode in ("h", "f"):
        cast = (lambda t: t) if mode == "h" else (lambda t: t.float())
        x = cast(x16).clone().requires_grad_(True)
        y = ops.maxpool2(x)
        assert y.dtype == x.dtype
        y.backward(cast(dy16))
        x2 = cast(x16).clone().requires_grad_(True)
        y2, skip = ops.maxpool2_skip(x2)
        torch.autograd.backward([y2, skip], [cast(dy16), cast(ds16)])
        assert x.grad.dtype == x.dtype and x2.grad.dtype == x.dtype
        res[mode] = (y.detach().float(), x.grad.float(), y2.detach().float(), x2.grad.float())
    for k in range(4):
        assert torch.equal(res["h"][k], res["f"][k]), k
    ref = torch.nn.functional.max_pool2d(x16.float().cpu(), 2)
    assert torch.equal(res["h"][0].cpu(), ref)


@pytest.mark.parametrize("c,h,w", [(16, 32, 24), (128, 8, 8), (32, 20, 12)])
def test_upsample_behind_the_skip_f16(c, h, w):
    """cat([skip, bilinear_x2(x)]) written in place behind the skip (ops.upcat) and the plain resize (ops.bilinear), forward and
    backward: interpolated in fp32, rounded once on store."""
    import torch.nn.functional as F
    from arco_amd import ops
    rs = np.random.RandomState(c + h)
    x16 = _rand_act(rs, (2, c, h, w))
    skip16 = _rand_act(rs, (2, c, 2 * h, 2 * w))
    dcat16 = _rand_act(rs, (2, 2 * c, 2 * h, 2 * w))
    res = {}
    for mode in ("h", "f"):
        dt = torch.float16 if mode == "h" else torch.float32
        x = x16.to(dt).clone().requires_grad_(True)
        buf = ops.new_act_nd(2, 2 * c, (2 * h, 2 * w), DEV, dt)
        buf[:, :c].copy_(skip16)
        skip = buf[:, :c].detach().requires_grad_(True)
        skip._arco_cat_buf = buf
        cat = ops.upcat(x, skip)
        assert cat.dtype == dt and cat.data_ptr() == buf.data_ptr()         # in place: no concat copy
        cat.backward(dcat16.to(dt))
        xb = x16.to(dt).clone().requires_grad_(True)
        up = ops.bilinear(xb, (2 * h + 1, 2 * w - 3))                          # a size that is not x2
        up.backward(torch.ones_like(up))
        res[mode] = (cat.detach().float(), x.grad.float(), skip.grad.float(), up.detach().float(), xb.grad.float())
    xr = x16.cpu().double().requires_grad_(True)
    upr = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=True)
    catr = torch.cat([skip16.cpu().double(), upr], 1)
    catr.backward(dcat16.cpu().double())
    assert torch.equal(res["h"][2], res["f"][2])                 # the skip's gradient is a slice
    for k, name in ((0, "cat"), (1, "dx"), (3, "resize"), (4, "resize dx")):
        e = _maxrel(res["h"][k], res["f"][k])
        print(f"upcat c={c} {h}x{w} {name}: vs fp32 kernel {e:.3e}")
        assert e < 1e-3, (name, e)
    assert _maxrel(res["h"][0], catr.detach()) < 1e-3 and _maxrel(res["h"][1], xr.grad) < 1e-3


@pytest.mark.parametrize("p,pool", [(0.0, False), (0.3, False), (0.0, True)])
def test_conv_bn_lrelu_dropout_stage_f16_storage(p, pool):
    """conv3x3 -> train-mode BatchNorm (statistics of the ROUNDED outputs, from the conv epilogue) -> LeakyReLU -> Dropout(p)
    (unetWithArgs.py:36-44), forward and backward, with room for the decoder's concat and the pooled second output of the encoder
    blocks; dropout masks are the ones the fp32 pass draws for the same seed."""
    from arco_amd import ops
    rs = np.random.RandomState(11)
    ci, co = 32, 32
    x16 = _rand_act(rs, (2, ci, 32, 48))
    w = torch.from_numpy((rs.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(np.float32)).to(DEV).half().float().requires_grad_(True)
    b = torch.zeros(co, device=DEV, requires_grad=True)
    gamma = torch.from_numpy(rs.uniform(0.5, 1.5, co).astype(np.float32)).to(DEV).requires_grad_(True)
    beta = torch.from_numpy(rs.standard_normal(co).astype(np.float32) * 0.2).to(DEV).requires_grad_(True)
    da16 = _rand_act(rs, (2, co, 32, 48))
    dp16 = _rand_act(rs, (2, co, 16, 24))
    outs = {}
    for mode in ("h", "f"):
        dt = torch.float16 if mode == "h" else torch.float32
        rm, rv = torch.zeros(co, device=DEV), torch.ones(co, device=DEV)
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        x = x16.to(dt).clone().requires_grad_(True)
        for t in (w, b, gamma, beta):
            t.grad = None
        ops.reseed_dropout(77)          # both arms draw their dropout mask from the same seed
        a = ops.conv_bn_act(x, w, b, gamma, beta, rm, rv, slope=0.01, p=p, num_batches_tracked=nbt, cat_room=co if pool else 0,
                            pool=pool)
        if pool:
            a, pooled = a
            assert pooled.dtype == dt and a._arco_cat_buf.dtype == dt
            torch.autograd.backward([a, pooled], [da16.to(dt), dp16.to(dt)])
        else:
            a.backward(da16.to(dt))
        assert a.dtype == dt
        outs[mode] = [a.detach().float(), x.grad.float(), w.grad.clone(), gamma.grad.clone(), beta.grad.clone(), rm.clone(), rv.clone()]
        if pool:
            outs[mode].append(pooled.detach().float())
    if p > 0:
        zh, zf = outs["h"][0] == 0, outs["f"][0] == 0
        assert 0.25 < float(zf.float().mean()) < 0.35
        assert float((zh != zf).float().mean()) < 1e-4          # the same mask (an activation that rounds to exactly 0 aside)
    # as tests/test_half_gpu.py::test_conv_bn_relu_stage_f16_storage: the activation element-wise; the gradients in the L2 norm
    # (a rounding can move a pre-activation across the LeakyReLU kink; the few flipped elements change slope 0.01 <-> 1)
    e = _maxrel(outs["h"][0], outs["f"][0])
    print(f"stage p={p} pool={pool}: activation {e:.3e}")
    assert e < 3e-3
    # pool=True: the pooled output's gradient is routed to the window's maximum of the STORED activation.  Two activations of a window
    # that differ by less than an f16 ulp (2^-11 relative: ~1e-3 of the windows for values of order 1) round to a tie, the route moves
    # to another pixel and that element carries its whole gradient: 2 dp^2 of a window's 4 da^2 + dp^2, i.e. a relative L2 distance of
    # sqrt(1e-3 * 2 / 5) = 2e-2 in expectation - inherent to any f16 storage of the activation; held to 3e-2
    bound = 3e-2 if pool else 1e-2
    for k in range(1, 5):
        e = _l2rel(outs["h"][k], outs["f"][k])
        print(f"  gradient {k}: L2 {e:.3e}")
        assert e < bound, k
    for k in (5, 6):
        assert _maxrel(outs["h"][k], outs["f"][k]) < 1e-3, k
    if pool:
        assert _maxrel(outs["h"][7], outs["f"][7]) < 3e-3


# ---- the whole U-Net ---------------------------------------------------------------------------------------------------------------
def _unet_reference(net, x, tgt, rnd):
    """UNet(1, 4).forward (unetWithArgs.py:88-158, dropout off, train-mode BatchNorm) restated with torch operators in float64 on the
    CPU; `rnd` is applied to BOTH operands of every convolution - the activations it reads and its weights (identity: the exact network;
    f16 rounding: the scale arm - a convolution on f16 matrix-core operands with exact accumulation, which is what the reduced-operand
    mode of the V-Net test does on fp32 tensors: igemm.hip's MMA = 1 rounds the A and the B fragment in registers).  Biases, BatchNorm,
    pooling and the upsample are exact, and so is the whole backward pass (the V-Net test's arm also rounds its gradient operands, to
    bf16: this arm is the stricter one)."""
    import torch.nn.functional as F
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.named_parameters()}

    def block(h, pre):
        for i in (0, 4):
            h = F.conv2d(rnd(h), rnd(P[f"{pre}.conv_conv.{i}.weight"]), P[f"{pre}.conv_conv.{i}.bias"], padding=1)
            h = F.batch_norm(h, None, None, P[f"{pre}.conv_conv.{i + 1}.weight"], P[f"{pre}.conv_conv.{i + 1}.bias"], True, 0.1, 1e-5)
            h = F.leaky_relu(h, 0.01)
        return h

    h = x.detach().cpu().double()
    xs = [block(h, "encoder.in_conv")]
    for i in range(1, 5):
        xs.append(block(F.max_pool2d(xs[-1], 2), f"encoder.down{i}.maxpool_conv.1"))
    fm = [xs[4]]
    h = xs[4]
    for i, skip in zip(range(1, 5), (xs[3], xs[2], xs[1], xs[0])):
        h = F.conv2d(rnd(h), rnd(P[f"decoder.up{i}.conv1x1.weight"]), P[f"decoder.up{i}.conv1x1.bias"])
        h = F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=True)
        h = block(torch.cat([skip, h], 1), f"decoder.up{i}.conv")
        fm.append(h)
    out = F.conv2d(rnd(h), rnd(P["decoder.out_conv.weight"]), P["decoder.out_conv.bias"], padding=1)
    loss = ((out - tgt.cpu().double()) ** 2).mean() + sum((f ** 2).mean() for f in fm) * 0.1
    loss.backward()
    return out.detach(), [f.detach() for f in fm], {k: v.grad for k, v in P.items() if v.grad is not None}


class _RoundF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.half().double()

    @staticmethod
    def backward(ctx, g):
        return g                    # only the forward's convolution operands are rounded


def test_unet_f16_storage_tracks_fp32_forward_and_gradients():
    """tests/test_half_gpu.py::test_vnet_f16_storage_tracks_fp32_forward_and_gradients restated for UNet(1, 4): 2 images of
    128 x 128, dropout off, the same weights, three arms - fp32 tensors (split-bf16 kernels), f16 storage, and for SCALE a float64
    restatement on the CPU that rounds the operands of every convolution (activations and weights) to f16 against the same restatement
    without rounding (the 2-D kernels have no reduced-operand mode on fp32 tensors; _unet_reference says what the arm models).  Logits
    and feature maps: relative L2 < 2e-2; parameter gradients: within 1.5 x the scale arm's distance + 2e-2 (activations that cross the
    LeakyReLU kink) - the V-Net test's bounds.

    MEASURED (MI355X, profiles/f16_2d_notes.md section 3): logits 2.0e-3 (scale arm 1.7e-3), feature maps 2.4e-3 ... 7.1e-3 (scale arm
    2.0e-3 ... 5.7e-3).  Gradients of 64 parameters: f16 storage 2.6e-4 ... 0.18, 0.73 ... 1.50 x the scale arm's over the encoder; all
    64 hold the rule, the tightest by 0.017 (decoder.up4.conv1x1.bias, 0.010 against 0.028); the parameter farthest from its
    scale arm is encoder.down3 conv_conv.1.weight, 0.169 against 1.5 x 0.113 + 2e-2 = 0.189.  The distance does not depend on the loss scale (2^10 ... 2^22: the same to three digits): it is
    the forward roundings moving pre-activations across the LeakyReLU kink and max-pool routes, not the f16 backward."""
    from arco_amd import ops
    from arco_amd.networks.unetWithArgs import UNet
    torch.manual_seed(3)
    net = UNet(1, 4).to(DEV).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.uniform(size=(2, 1, 128, 128)).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy(rs.standard_normal((2, 4, 128, 128)).astype(np.float32)).to(DEV)
    res = {}
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    try:
        for half in (False, True):
            ops.ACT_HALF = half
            ops.bump_weight_epoch()
            net.load_state_dict(sd)
            net.zero_grad()
            seen = []
            hook = net.encoder.down2.maxpool_conv[1].register_forward_hook(lambda m, i, o: seen.append((o[0] if isinstance(o, tuple) else o).dtype))
            out, x4, fm = net(x)
            hook.remove()
            assert seen == [torch.float16 if half else torch.float32]          # the activations inside the network
            assert out.dtype == torch.float32 and x4.dtype == torch.float32 and all(f.dtype == torch.float32 for f in fm)
            loss = ((out - tgt) ** 2).mean() + sum((f ** 2).mean() for f in fm) * 0.1
            loss.backward()
            scale = ops.LOSS_SCALE if half else 1.0
            res[half] = (out.detach().clone(), [f.detach().clone() for f in fm],
                         {n: p.grad.detach().clone() / scale for n, p in net.named_parameters() if p.grad is not None})
    finally:
        ops.ACT_HALF = False
        ops.bump_weight_epoch()
    net.load_state_dict(sd)
    exact = _unet_reference(net, x, tgt, lambda t: t)
    rounded = _unet_reference(net, x, tgt, _RoundF16.apply)
    e2, o2, f2 = _l2rel(res[True][0], res[False][0]), _l2rel(rounded[0], exact[0]), _l2rel(res[False][0], exact[0])
    print(f"logits: f16 storage vs fp32 kernels L2 {e2:.3e} | scale arm (float64, f16-rounded conv operands) {o2:.3e} | fp32 kernels vs float64 {f2:.3e}")
    assert e2 < 2e-2, e2
    for i, (a, b) in enumerate(zip(res[True][1], res[False][1])):
        e = _l2rel(a, b)
        print(f"feature map {i}: L2 {e:.3e} | scale arm {_l2rel(rounded[1][i], exact[1][i]):.3e}")
        assert e < 2e-2, (i, e)
    assert set(res[True][2]) == set(res[False][2])
    worst, bad = 0.0, []
    for n, g in res[False][2].items():
        gh = res[True][2][n]
        if float(g.abs().max()) < 1e-9:           # conv biases under train-mode BN: exact zeros in every mode
            assert float(gh.abs().max()) < 1e-6, n
            continue
        e = float((gh - g).norm()) / float(g.norm())
        eo = float((rounded[2][n] - exact[2][n]).norm()) / float(exact[2][n].norm())
        worst = max(worst, e)
        print(f"grad {n}: f16 storage {e:.3e} | scale arm {eo:.3e}")
        if not e < 1.5 * eo + 2e-2:
            bad.append((n, e, eo))
    print("worst relative L2 gradient error", worst)
    assert not bad, bad             # (every parameter is measured before the rule is asserted)


def test_eval_route_ignores_act_dtype():
    """model.eval() logits with ops.ACT_HALF set are bit-identical to those without: evaluation stays on the fp32 route."""
    from arco_amd import ops
    from arco_amd.networks.unetWithArgs import UNet
    torch.manual_seed(4)
    net = UNet(1, 4).to(DEV).eval()
    x = torch.rand(2, 1, 64, 64, device=DEV)
    try:
        with torch.no_grad():
            ops.ACT_HALF = False
            a, a4, afm = net(x)
            ops.ACT_HALF = True
            b, b4, bfm = net(x)
    finally:
        ops.ACT_HALF = False
    assert b.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a4, b4)
    assert all(f.dtype == torch.float32 and torch.equal(f, g) for f, g in zip(bfm, afm))


def test_pack_plan_carries_f16_packs_for_conv2d():
    """PackPlan(half=[True]) over a U-Net: every 3x3 / 1x1 Conv2d with >= 8 input channels is served its f16 pack from the plan;
    the first layer keeps the fp32 pack its kernel reads."""
    from arco_amd import ops
    from arco_amd.networks.unetWithArgs import UNet
    torch.manual_seed(5)
    net = UNet(1, 4).to(DEV).train()
    plan = ops.PackPlan([net], with_dgrad=True, half=[True])
    plan.refresh()
    w = net.encoder.down1.maxpool_conv[1].conv_conv[0].weight
    wp = ops.pack_weight(w, 9, 0, half=True)
    assert wp.dtype == torch.float16 and wp.data_ptr() == w._arco_plan[0][3].data_ptr()
    fresh = ops._pack_now(w.detach().contiguous(), 32, 16, 9, 0, False, half=True)
    assert torch.equal(wp, fresh)
    w0 = net.encoder.in_conv.conv_conv[0].weight
    assert ops.pack_weight(w0, 9, 0).dtype == torch.float32 and w0._arco_plan[0][3] is None
