"""F16 INFERENCE (`ops.eval_half()`, eval_surface's act_dtype="f16"): the scope, the accuracy of the U-Net route against the fp32 route,
the V-Net route against today's process-wide switch, and the four evaluation entry points - each held to a result assembled by hand
from the stored f16 logits through the functions that exist already.  What must not move is asserted next to it: defaults,
act_dtype="f32", forwards before and after the scope, the switches of `ops`."""
import numpy as np
import pytest
import torch

import fixture_inputs as fx

gpu = pytest.mark.gpu
DEV = "cuda:0"
C2, PATCH2, VOL2 = 4, (64, 64), (5, 40, 36)
C3, PATCH3, SXY, SZ = 2, (32, 32, 16), 8, 4
VOLS3 = [(40, 36, 20), (24, 24, 12)]              # ragged last windows on every axis; smaller than the patch (padded)


def _switches():
    from arco_amd import ops
    return (ops.ACT_HALF, ops.EVAL_HALF, ops.LOGITS_CAST, ops._OPEN_HALF_2D, ops.FM_CAST, ops.CONV_MMA, ops.HEAD_MMA, ops.BN_GROUPS,
            ops.LOSS_SCALE, ops.WGRAD_SIDE, ops.POOL_FUSE, ops.BLOCK_FUSE)


def _l2rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(1e-20, float(b.double().cpu().norm()))


@pytest.fixture(scope="module")
def unet():
    """UNet(1, 4).eval() with seeded weights, affine parameters (1 + 0.1 N, 0.1 N) and running statistics (0.2 N, U(0.5, 1.5)), and
    its input: 2 x 1 x 64 x 64."""
    from arco_amd.networks.unetWithArgs import UNet
    net = UNet(1, C2).to(DEV)
    net.load_state_dict(fx.randomize_running_stats(fx.unet_state(41, 1, C2), 42), strict=True)
    x = torch.from_numpy(np.random.RandomState(43).uniform(size=(2, 1, 64, 64)).astype(np.float32)).to(DEV)
    return net.eval(), x


@pytest.fixture(scope="module")
def vnet():
    from arco_amd.networks.vnetWithArgs import VNet
    net = VNet(n_channels=1, n_classes=C3, normalization='batchnorm').to(DEV)
    net.load_state_dict(fx.randomize_running_stats(fx.vnet_state(51, 1, C3, 16), 52), strict=True)
    return net.eval()


# ---- the scope ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_scope_opens_the_f16_route_and_leaves_everything_else_where_it_was(unet):
    from arco_amd import ops
    net, x = unet
    before = _switches()
    with torch.no_grad():
        base, base4, base_fm = net(x)                                  # (taken before this test enters the scope)
        assert base.dtype == torch.float32
        seen = []
        hook = net.encoder.down2.maxpool_conv[1].register_forward_hook(lambda m, i, o: seen.append((o[0] if isinstance(o, tuple) else o).dtype))
        with ops.eval_half():
            out, x4, fm = net(x)
        assert seen == [torch.float16]                                 # the activations inside the network
        assert out.dtype == torch.float32 and x4.dtype == torch.float32 and all(f.dtype == torch.float32 for f in fm)
        assert not net.training and _switches() == before
        with ops.eval_half(logits="stored"):
            s_out, s4, s_fm = net(x)
        assert s_out.dtype == torch.float16 and tuple(s_out.shape) == tuple(out.shape)
        assert torch.equal(s_out.float(), out)                         # the cast is all that differs
        assert torch.equal(s4, x4) and all(f.dtype == torch.float32 and torch.equal(f, g) for f, g in zip(s_fm, fm))
        net(x)
        assert seen == [torch.float16, torch.float16, torch.float32]   # after the scope: the fp32 route again
        hook.remove()
        assert not torch.equal(out, base)                              # (another route: the accuracy test says how far)

        def same_as_base():
            o, o4, ofm = net(x)
            return (o.dtype == torch.float32 and torch.equal(o, base) and torch.equal(o4, base4)
                    and all(torch.equal(f, g) for f, g in zip(ofm, base_fm)))
        assert same_as_base()
        try:
            for flag in (True, False):
                ops.ACT_HALF = flag
                assert same_as_base()                                  # the process-wide switch alone does not move an eval forward
        finally:
            ops.ACT_HALF = before[0]
    assert _switches() == before
    with pytest.raises(ValueError, match="logits"):
        ops.eval_half(logits="f16")


@gpu
def test_a_body_that_raises_leaves_every_switch_as_it_was(unet):
    from arco_amd import ops
    net, x = unet
    before = _switches()
    with pytest.raises(KeyError):
        with ops.eval_half(logits="stored"):
            assert _switches() != before
            raise KeyError("body")
    assert _switches() == before

    def boom(m, i, o):
        raise ZeroDivisionError("inside the network")
    hook = net.encoder.down2.maxpool_conv[1].register_forward_hook(boom)      # fires inside the Encoder's open_half region
    try:
        with pytest.raises(ZeroDivisionError), torch.no_grad(), ops.eval_half():
            net(x)
    finally:
        hook.remove()
    assert _switches() == before
    with torch.no_grad():
        assert net(x)[0].dtype == torch.float32


# ---- accuracy, U-Net ------------------------------------------------------------------------------------------------------------------
def _unet_eval_reference(net, x, rnd):
    """UNet(1, 4)'s evaluation-mode forward (unetWithArgs.py:88-158: BatchNorm with the running statistics, dropout inactive) restated
    with torch operators in float64 on the CPU.  `rnd` is applied to everything the f16 route STORES: every pre-activation a
    convolution writes, every activation, the 1x1 convolution's output, the upsampled map, the logits - and to the weights of the
    convolutions that read the f16 pack (all but the first layer, which reads the fp32 image with fp32 weights).  A maximum and a
    concatenation of rounded values need no rounding.  rnd = identity: the exact network."""
    import torch.nn.functional as F
    P = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}

    def block(h, pre, first=False):
        for i in (0, 4):
            w = P[f"{pre}.conv_conv.{i}.weight"]
            z = rnd(F.conv2d(h, w if (first and i == 0) else rnd(w), P[f"{pre}.conv_conv.{i}.bias"], padding=1))
            bn = f"{pre}.conv_conv.{i + 1}"
            y = F.batch_norm(z, P[bn + ".running_mean"], P[bn + ".running_var"], P[bn + ".weight"], P[bn + ".bias"], False, 0.0, 1e-5)
            h = rnd(F.leaky_relu(y, 0.01))
        return h

    xs = [block(x.detach().cpu().double(), "encoder.in_conv", first=True)]
    for i in range(1, 5):
        xs.append(block(F.max_pool2d(xs[-1], 2), f"encoder.down{i}.maxpool_conv.1"))
    h = xs[4]
    fm = [h]
    for i, skip in zip(range(1, 5), (xs[3], xs[2], xs[1], xs[0])):
        h = rnd(F.conv2d(h, rnd(P[f"decoder.up{i}.conv1x1.weight"]), P[f"decoder.up{i}.conv1x1.bias"]))
        h = rnd(F.interpolate(h, scale_factor=2, mode="bilinear", align_corners=True))
        h = block(torch.cat([skip, h], 1), f"decoder.up{i}.conv")
        fm.append(h)
    out = rnd(F.conv2d(h, rnd(P["decoder.out_conv.weight"]), P["decoder.out_conv.bias"], padding=1))
    return out, fm


@gpu
def test_unet_f16_inference_tracks_the_fp32_route(unet):
    """The f16 route against the fp32 route of the same net (seeded non-trivial running statistics and affine parameters), relative L2
    of the logits and of each of the five feature maps.  Yardstick: _unet_eval_reference rounding every stored value to f16 against the
    same restatement without rounding.  Rule (tests/test_half2d_gpu.py::test_unet_f16_storage_tracks_fp32_forward_and_gradients, whose
    1.5 and floor are taken over unchanged): distance(f16 route, fp32 route) <= 1.5 x distance(rounded, exact) + 2e-2.

    MEASURED (MI355X, profiles/eval2d_gpu_notes.md), f16 route vs fp32 route | rounded vs exact restatement: logits 4.26e-4 | 4.29e-4;
    feature maps 3.88e-4 | 3.87e-4, 3.74e-4 | 3.70e-4, 4.39e-4 | 4.43e-4, 4.07e-4 | 4.06e-4, 4.71e-4 | 4.72e-4 (the fp32 route sits
    2.6e-7 ... 4.7e-7 from the exact restatement).  The restatement predicts the route to a percent of the distance, so the rule holds
    with room to spare: its floor of 2e-2 is 40 times what is measured.  The rule is kept as the merged test states it, not tightened
    to these figures.  Every figure is printed before the rule is asserted."""
    from arco_amd import ops
    net, x = unet
    with torch.no_grad():
        f32 = net(x)
        with ops.eval_half():
            f16 = net(x)
    exact = _unet_eval_reference(net, x, lambda t: t)
    rounded = _unet_eval_reference(net, x, lambda t: t.half().double())
    names = ["logits"] + [f"feature map {i}" for i in range(5)]
    got = [(f16[0], f32[0])] + list(zip(f16[2], f32[2]))
    ref = [(rounded[0], exact[0])] + list(zip(rounded[1], exact[1]))
    rows = []
    for name, (a, b), (r, e) in zip(names, got, ref):
        assert tuple(a.shape) == tuple(r.shape)
        rows.append((name, _l2rel(a, b), _l2rel(r, e), _l2rel(b, e)))
        print(f"{name}: f16 route vs fp32 route L2 {rows[-1][1]:.3e} | rounded vs exact restatement {rows[-1][2]:.3e} | "
              f"fp32 route vs exact restatement {rows[-1][3]:.3e}")
    for name, d, d_ref, _ in rows:
        assert d <= 1.5 * d_ref + 2e-2, (name, d, d_ref)
        assert d > 0 and d_ref > 0, name


# ---- accuracy, V-Net ------------------------------------------------------------------------------------------------------------------
@gpu
def test_vnet_scope_is_todays_f16_route_without_the_global(vnet):
    from arco_amd import ops
    from arco_amd.networks.vnetWithArgs import VNet
    x = torch.from_numpy(np.random.RandomState(53).uniform(size=(1, 1, 32, 32, 16)).astype(np.float32)).to(DEV)
    before = _switches()
    with torch.no_grad():
        base = vnet(x)[0]
        try:
            ops.ACT_HALF = True
            seen = []
            hook = vnet.block_two.register_forward_hook(lambda m, i, o: seen.append(o.dtype))
            manual = vnet(x)[0]
        finally:
            ops.ACT_HALF = before[0]
        with ops.eval_half():
            scoped, _, fm = vnet(x)
        hook.remove()
        assert seen == [torch.float16, torch.float16]
        assert scoped.dtype == torch.float32 and all(f.dtype == torch.float32 for f in fm)
        assert torch.equal(scoped, manual) and not torch.equal(scoped, base)
        with ops.eval_half(logits="stored"):
            stored = vnet(x)[0]
        assert stored.dtype == torch.float16 and torch.equal(stored.float(), manual)
        assert torch.equal(vnet(x)[0], base) and _switches() == before
        torch.manual_seed(0)
        gn = VNet(n_channels=1, n_classes=C3, normalization='groupnorm').to(DEV).eval()
        with pytest.raises(RuntimeError, match="batchnorm"), ops.eval_half():
            gn(x)
        assert gn(x)[0].dtype == torch.float32 and _switches() == before


# ---- 2-D entry points -----------------------------------------------------------------------------------------------------------------
def _volume2d():
    rs = np.random.RandomState(61)
    img = rs.uniform(size=VOL2).astype(np.float32)
    lab = np.stack([fx.blob_labels(rs, 1, VOL2[1:], C2)[0] for _ in range(VOL2[0])]).astype(np.int64)
    return img, lab


def _by_hand_2d(net, img, order):
    """The label map of the stored f16 logits: the slices to the patch as predict_volume(zoom="gpu") takes them there, one forward inside
    the scope, the logits cast to fp32, the existing argmax_zoom_back."""
    from arco_amd import ops
    from arco_amd.utils import zoom_gpu
    vol = torch.from_numpy(img).to(DEV)
    zoomed = zoom_gpu.zoom_nearest(vol, PATCH2) if order == 0 else zoom_gpu.zoom_cubic(vol, PATCH2)
    with torch.no_grad(), ops.eval_half(logits="stored"):
        logits = net(zoomed.unsqueeze(1))[0]
    assert logits.dtype == torch.float16
    return zoom_gpu.argmax_zoom_back(logits.float(), VOL2[1:])


@gpu
@pytest.mark.parametrize("order", [0, 3])
def test_2d_entry_points_f16(unet, order):
    from arco_amd import eval_surface, test_2D
    from arco_amd.utils import surface_gpu
    net, _ = unet
    img, lab = _volume2d()
    before = _switches()
    hand = _by_hand_2d(net, img, order)
    assert len(torch.unique(hand)) > 1
    pred = eval_surface.predict_volume(img, net, PATCH2, zoom="gpu", order=order, act_dtype="f16")
    assert pred.is_cuda and pred.dtype == torch.int64 and torch.equal(pred, hand) and _switches() == before
    host = eval_surface.predict_volume(img, net, PATCH2, zoom="host", order=order, act_dtype="f16")
    assert isinstance(host, np.ndarray) and host.dtype == np.int64 and np.array_equal(host, hand.cpu().numpy()) and _switches() == before
    assert np.array_equal(eval_surface.predict_volume(img, net, PATCH2, order=order, act_dtype="f16"), host)       # zoom defaults to "host"
    assert np.array_equal(eval_surface.predict_volume(img, net, PATCH2, batch=2, zoom="gpu", order=order, act_dtype="f16").cpu().numpy(),
                          eval_surface.predict_volume(img, net, PATCH2, batch=2, zoom="host", order=order, act_dtype="f16"))
    # the four numbers of every class: the hand-made map scored through the device functions that exist
    lab_d = torch.from_numpy(lab).to(DEV)
    cnt = test_2D.overlap_counts(hand, lab_d, C2).cpu().numpy()
    scored = surface_gpu.surface_metrics(hand, lab_d, range(1, C2))
    want = []
    for c in range(1, C2):
        dice, jc = test_2D._dice_jc(int(cnt[c, 0]), int(cnt[c, 1]), int(cnt[c, 2]))
        want.append((dice, jc) + (tuple(scored[c - 1]) if cnt[c, 0] > 0 and cnt[c, 1] > 0 else (0.0, 0.0)))
    got = eval_surface.test_single_volume(img, lab, net, C2, PATCH2, surface="gpu", zoom="gpu", order=order, act_dtype="f16")
    assert got == want and any(m[2] > 0 for m in got) and _switches() == before
    assert eval_surface.test_single_volume(img, lab, net, C2, PATCH2, surface="gpu", zoom="host", order=order, act_dtype="f16") == want
    # the pass-through route (surface="host", everything else at its default) takes the keyword too
    ph = eval_surface.test_single_volume(img, lab, net, C2, PATCH2, order=order, act_dtype="f16")
    assert len(ph) == C2 - 1 and [m[:2] for m in ph] == [m[:2] for m in want] and _switches() == before
    for m, w in zip(ph, want):
        assert m[2] == w[2] and abs(m[3] - w[3]) <= 1e-9 * max(1.0, abs(w[3]))        # hd95 equal, asd to one float64 sum (eval_surface's note)
    assert not net.training


@gpu
@pytest.mark.parametrize("order", [0, 3])
def test_2d_entry_points_f32_is_the_call_without_the_keyword(unet, order):
    from arco_amd import eval_surface
    net, _ = unet
    img, lab = _volume2d()
    before = _switches()
    for kw in ({}, {"zoom": "host"}, {"zoom": "gpu"}):
        a = eval_surface.predict_volume(img, net, PATCH2, order=order, **kw)
        b = eval_surface.predict_volume(img, net, PATCH2, order=order, act_dtype="f32", **kw)
        assert type(a) is type(b) and (torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b))
    for kw in ({}, {"surface": "gpu"}, {"surface": "gpu", "zoom": "gpu"}, {"surface": "gpu", "zoom": "gpu", "nms": 1, "cc": "gpu"}):
        assert (eval_surface.test_single_volume(img, lab, net, C2, PATCH2, order=order, **kw)
                == eval_surface.test_single_volume(img, lab, net, C2, PATCH2, order=order, act_dtype="f32", **kw))
    assert _switches() == before


# ---- 3-D entry points -----------------------------------------------------------------------------------------------------------------
@gpu
def test_3d_entry_points(vnet):
    from arco_amd import eval_surface, ops, test_2D
    from arco_amd.utils import cc_gpu, surface_gpu
    before = _switches()
    cases, preds = [], []
    for i, shp in enumerate(VOLS3):
        image = fx.eval3d_volume(71 + i, shp)
        today = eval_surface.predict_case(vnet, image, SXY, SZ, PATCH3, C3)
        assert torch.equal(eval_surface.predict_case(vnet, image, SXY, SZ, PATCH3, C3, act_dtype="f32"), today)
        try:
            ops.ACT_HALF = True
            manual = eval_surface.predict_case(vnet, image, SXY, SZ, PATCH3, C3)
        finally:
            ops.ACT_HALF = before[0]
        got = eval_surface.predict_case(vnet, image, SXY, SZ, PATCH3, C3, act_dtype="f16")
        assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == shp
        assert torch.equal(got, manual) and _switches() == before
        assert bool(got.any()) and not bool(got.all())
        cases.append((image, fx.blob_labels(np.random.RandomState(81 + i), 1, shp, C3)[0]))     # one box of class 1 per volume
        preds.append(got)
    assert any(s < p for s, p in zip(VOLS3[1], PATCH3))
    kw = dict(patch_size=PATCH3, stride_xy=SXY, stride_z=SZ)
    total = np.zeros(4)
    for (image, label), pred in zip(cases, preds):                       # the f16 label maps scored by hand
        p = cc_gpu.largest_cc(pred).to(torch.int64)
        g = torch.from_numpy((label != 0).astype(np.int64)).to(DEV)
        n_pred, n_gt, n_both = test_2D.overlap_counts(p, g, 2)[1].cpu().tolist()
        assert n_pred > 0
        total += np.asarray((2.0 * n_both / float(n_pred + n_gt), float(n_both) / float(n_pred + n_gt - n_both)) + tuple(surface_gpu.pair_metrics(p, g)))
    want = total / len(cases)
    got = eval_surface.test_all_case(vnet, cases, C3, surface="gpu", cc="gpu", nms=1, act_dtype="f16", **kw)
    assert got.shape == (4,) and np.array_equal(got[:3], want[:3]) and got[2] > 0
    np.testing.assert_allclose(got[3], want[3], rtol=1e-12, atol=0)
    assert _switches() == before
    host = eval_surface.test_all_case(vnet, cases, C3, surface="gpu", cc="host", nms=1, act_dtype="f16", **kw)          # test_single_case in the scope
    assert np.array_equal(host[:3], want[:3]) and _switches() == before
    passthrough = eval_surface.test_all_case(vnet, cases, C3, nms=1, act_dtype="f16", **kw)                              # surface="host", all defaults
    assert np.array_equal(passthrough[:3], want[:3]) and _switches() == before
    np.testing.assert_array_equal(eval_surface.test_all_case(vnet, cases, C3, surface="gpu", cc="gpu", nms=1, act_dtype="f32", **kw),
                                  eval_surface.test_all_case(vnet, cases, C3, surface="gpu", cc="gpu", nms=1, **kw))
    assert _switches() == before and not vnet.training


# ---- argument checking (no GPU, no library) -------------------------------------------------------------------------------------------
def test_a_bad_act_dtype_is_a_value_error_before_any_work(monkeypatch):
    from arco_amd import eval_surface

    def never(*a, **k):
        raise AssertionError("reached the library / the network")
    for name in ("call", "load", "query"):
        monkeypatch.setattr(eval_surface._L, name, never)

    class Net:
        training = False
        eval = train = __call__ = never
    img2, lab2 = np.zeros(VOL2, dtype=np.float32), np.zeros(VOL2, dtype=np.int64)
    img3 = np.zeros(VOLS3[1], dtype=np.float32)
    before = _switches()
    for zoom in ("host", "gpu"):
        with pytest.raises(ValueError, match="act_dtype"):
            eval_surface.predict_volume(img2, Net(), PATCH2, zoom=zoom, act_dtype="bf16")
    for kw in ({}, {"surface": "gpu", "zoom": "gpu"}):
        with pytest.raises(ValueError, match="act_dtype"):
            eval_surface.test_single_volume(img2, lab2, Net(), C2, PATCH2, act_dtype="bf16", **kw)
    with pytest.raises(ValueError, match="act_dtype"):
        eval_surface.predict_case(Net(), img3, SXY, SZ, PATCH3, C3, act_dtype="bf16")
    for kw in ({}, {"surface": "gpu", "cc": "gpu"}):
        with pytest.raises(ValueError, match="act_dtype"):
            eval_surface.test_all_case(Net(), [(img3, img3)], C3, patch_size=PATCH3, stride_xy=SXY, stride_z=SZ, act_dtype="bf16", **kw)
    for bad in (None, "F16", 16, "half"):
        with pytest.raises(ValueError, match="act_dtype"):
            eval_surface.check_act_dtype(bad)
    assert eval_surface.check_act_dtype("f32") == "f32" and eval_surface.check_act_dtype("f16") == "f16"
    assert _switches() == before
