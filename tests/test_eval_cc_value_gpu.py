"""The by-value `nms` post-processing of eval_surface on the device (cc="gpu": cc_gpu.largest_cc_by_value / largest_per_class on the label
map that is there already) against the host route (cc="host": cc_host.getLargestCC_by_value / keep_largest_per_class), with
surface="gpu" on both: dice, jc and hd95 equal (==), asd to rtol 1e-12 - the masks are identical, only the order of one float64 sum may
differ (the bar of tests/test_eval_cc_gpu.py).
  3-D  test_all_case(nms=1, nms_mode="value" | "per_class" | "foreground") on a three-class VNet: the "padded" fixture volume and a
       ragged one
  2-D  test_single_volume(nms=1) on the four-class U-Net and volume of EVAL2D_CASES["a"], both zoom routes, and surface="host"
The predictions of these random networks are speckled, so each mode removes voxels and the modes differ; that is asserted."""
import numpy as np
import pytest
import torch

import fixture_inputs as fx

pytestmark = pytest.mark.gpu

RAGGED = (20, 22, 18)                                  # against the 16^3 patch: clamped last windows on every axis
MODES = ("value", "per_class", "foreground")


@pytest.fixture(scope="module")
def setup3d():
    """(net, C, kw, [(image, prediction of test_single_case), ...]): the padded volume and a ragged one, predicted once."""
    from arco_amd import test_util
    from arco_amd.networks.vnetWithArgs import VNet
    shape, patch, sxy, sz, C, nf, seed = fx.EVAL3D_CASES["padded"]
    assert C == 3 and shape == (12, 16, 10) and patch == (16, 16, 16)
    net = VNet(n_channels=1, n_classes=C, n_filters=nf, normalization='batchnorm', has_dropout=False).cuda()
    net.load_state_dict(fx.randomize_running_stats(fx.vnet_state(seed, 1, C, nf), seed + 1), strict=True)
    kw = dict(patch_size=patch, stride_xy=6, stride_z=4)
    vols = []
    for i, shp in enumerate((shape, RAGGED)):
        image = fx.eval3d_volume(seed + 2 + i, shp)
        pred, _ = test_util.test_single_case(net, image, kw["stride_xy"], kw["stride_z"], patch, num_classes=C)
        assert pred.shape == shp and set(np.unique(pred)) == {0, 1, 2}
        vols.append((image, pred))
    return net, C, kw, vols


@pytest.fixture(scope="module")
def setup2d():
    from arco_amd.networks.unetWithArgs import UNet
    shape, C, seed = fx.EVAL2D_CASES["a"]
    assert shape == (3, 40, 36) and C == 4
    image, label = fx.eval2d_volume(seed, shape, C)
    net = UNet(in_chns=1, class_num=C).cuda()
    net.load_state_dict(fx.randomize_running_stats(fx.unet_state(seed, 1, C), seed + 1))
    net.eval()
    return net, C, image, label


def _same(got, exp):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape and got.shape[-1] == 4
    assert np.array_equal(got[..., :3], exp[..., :3]), (got, exp)
    np.testing.assert_allclose(got[..., 3], exp[..., 3], rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode", MODES)
def test_all_case_cc_gpu_equals_cc_host(setup3d, mode):
    from arco_amd import eval_surface
    net, C, kw, vols = setup3d
    cases = [(image, np.roll(pred, 2, axis=0)) for image, pred in vols] + [(vols[1][0], vols[1][1])]
    host = eval_surface.test_all_case(net, cases, C, nms=1, nms_mode=mode, surface="gpu", cc="host", **kw)
    assert host[0] > 0 and host[2] > 0 and host[3] > 0                                 # the comparison is not of zeros
    _same(eval_surface.test_all_case(net, cases, C, nms=1, nms_mode=mode, surface="gpu", cc="gpu", **kw), host)
    np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, nms=1, nms_mode=mode, surface="gpu", **kw), host)  # default "host"
    # the host surface route scores the same masks: hd95 equal, asd to the order of one float64 sum
    _same(eval_surface.test_all_case(net, cases, C, nms=1, nms_mode=mode, cc="host", **kw), host)


def test_modes_differ_and_remove_voxels(setup3d):
    """Each mode is held to more than the identity, and "value" to more than "foreground": on these predictions the largest component
    of one value is not the largest foreground component, and the per-class map is a proper subset of the prediction."""
    from arco_amd import eval_surface
    from arco_amd.test_util import getLargestCC
    from arco_amd.utils.cc_host import getLargestCC_by_value, keep_largest_per_class
    from arco_amd.utils import cc_gpu
    net, C, kw, vols = setup3d
    removed = differ = 0
    for image, pred in vols:
        per_class, value, fg = keep_largest_per_class(pred), getLargestCC_by_value(pred), getLargestCC(pred)
        pd = torch.from_numpy(pred).cuda()
        assert np.array_equal(cc_gpu.largest_per_class(pd, C).cpu().numpy(), per_class)
        assert np.array_equal(cc_gpu.largest_cc_by_value(pd, C).cpu().numpy(), value)
        assert ((per_class == pred) | (per_class == 0)).all() and not (value & ~fg).any()      # subsets of the prediction / the foreground
        removed += int((per_class != pred).any())
        differ += int(not np.array_equal(value, fg))
    assert removed > 0 and differ > 0
    cases = [(image, np.roll(pred, 2, axis=0)) for image, pred in vols]
    by_mode = {m: eval_surface.test_all_case(net, cases, C, nms=1, nms_mode=m, surface="gpu", cc="gpu", **kw) for m in MODES}
    plain = eval_surface.test_all_case(net, cases, C, nms=0, surface="gpu", cc="gpu", **kw)
    assert not np.array_equal(by_mode["value"], by_mode["foreground"]) and not np.array_equal(by_mode["per_class"], plain)
    assert not np.array_equal(by_mode["per_class"], by_mode["value"])


def test_defaults_are_unchanged_3d(setup3d):
    from arco_amd import eval_surface
    net, C, kw, vols = setup3d
    cases = [(image, np.roll(pred, 2, axis=0)) for image, pred in vols]
    for route in (dict(surface="gpu", cc="gpu"), dict(surface="gpu"), dict()):
        for nms in (0, 1):
            today = eval_surface.test_all_case(net, cases, C, nms=nms, **route, **kw)
            np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, nms=nms, nms_mode="foreground", **route, **kw), today)
        plain = eval_surface.test_all_case(net, cases, C, nms=0, **route, **kw)
        for mode in MODES + ("not read without nms",):
            np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, nms=0, nms_mode=mode, **route, **kw), plain)


def test_single_volume_nms(setup2d):
    from arco_amd import eval_surface, test_2D
    from arco_amd.utils.cc_host import keep_largest_per_class
    net, C, image, label = setup2d
    pred = test_2D.predict_volume(image, net)
    kept = keep_largest_per_class(pred)
    assert len(np.unique(pred[pred != 0])) >= 3 and (kept != pred).any() and kept.any()           # the post-processing removes voxels
    gpu = eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom="gpu", nms=1, cc="gpu")
    assert len(gpu) == C - 1 and any(m[2] > 0 for m in gpu)
    for zoom in ("gpu", "host"):
        _same(gpu, eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom=zoom, nms=1, cc="host"))
        _same(gpu, eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom=zoom, nms=1))
    _same(gpu, eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom="host", nms=1, cc="gpu"))
    host = eval_surface.test_single_volume(image, label, net, C, surface="host", nms=1, cc="host")
    _same(gpu, host)
    assert host == eval_surface.test_single_volume(image, label, net, C, nms=1)                   # the defaults are the host routes
    # ... and it is the metric list of the post-processed map
    exp = [test_2D.calculate_metric_percase(kept == c, label == c) for c in range(1, C)]
    assert host == exp
    plain = eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom="gpu")
    assert plain != gpu and len(plain) == len(gpu)                                               # nms=1 scores another map


def test_defaults_are_unchanged_2d(setup2d):
    from arco_amd import eval_surface, test_2D
    net, C, image, label = setup2d
    host = test_2D.test_single_volume(image, label, net, C)
    assert eval_surface.test_single_volume(image, label, net, C) == host
    assert eval_surface.test_single_volume(image, label, net, C, nms=0) == host
    assert eval_surface.test_single_volume(image, label, net, C, nms=0, cc="host") == host
    for zoom in ("gpu", "host"):
        today = eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom=zoom)
        for cc in ("host", "gpu"):
            assert eval_surface.test_single_volume(image, label, net, C, surface="gpu", zoom=zoom, nms=0, cc=cc) == today


def test_rejections_before_any_gpu_work():
    from arco_amd import eval_surface
    image = np.zeros((2, 8, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="nms_mode"):
        eval_surface.test_all_case(None, [(image, image)], 3, nms=1, nms_mode="largest", surface="gpu", cc="gpu")
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_single_volume(image, image, None, 4, nms=1, cc="gpu", surface="host")
