"""The evaluation entry points of arco_amd/eval_surface.py with surface="gpu" (hd95 / asd from arco_amd/utils/surface_gpu.py) against the
host route, which is arco_amd.test_2D / arco_amd.test_util themselves: the same dice / jc, the same hd95 (==) and asd to rtol 1e-12
(the order of one float64 sum).  The networks and volumes are those of tests/test_eval_gpu.py."""
import numpy as np
import pytest
import torch

import fixture_inputs as fx

pytestmark = pytest.mark.gpu


def _same(got, exp):
    assert got[0] == exp[0] and got[1] == exp[1] and got[2] == exp[2], (got, exp)
    np.testing.assert_allclose(got[3], exp[3], rtol=1e-12, atol=0)


def test_single_volume_surface_gpu_equals_host():
    from arco_amd import eval_surface, test_2D
    from arco_amd.networks.unetWithArgs import UNet
    C = 4
    sd = fx.unet_state(21, 1, C)
    rs = np.random.RandomState(4)          # with this seed every class has voxels in the prediction and in the label (asserted below)
    for k in list(sd):
        if k.endswith("running_mean"):
            sd[k] = torch.from_numpy(rs.normal(scale=0.1, size=tuple(sd[k].shape)).astype(np.float32))
        if k.endswith("running_var"):
            sd[k] = torch.from_numpy(rs.uniform(0.5, 1.5, size=tuple(sd[k].shape)).astype(np.float32))
    net = UNet(1, C).cuda()
    net.load_state_dict(sd, strict=True)
    img = rs.uniform(size=(5, 48, 80)).astype(np.float32)
    lab = np.stack([fx.blob_labels(rs, 1, (48, 80), C)[0] for _ in range(5)]).astype(np.int64)
    patch = (64, 64)
    host = test_2D.test_single_volume(img, lab, net, C, patch)
    assert eval_surface.test_single_volume(img, lab, net, C, patch) == host
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="host") == host
    gpu = eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu")
    assert len(gpu) == len(host) == C - 1
    for g, h in zip(gpu, host):
        _same(g, h)
    pred = test_2D.predict_volume(img, net, patch)
    scored = [c for c in range(1, C) if (pred == c).any() and (lab == c).any()]
    assert scored and all(host[c - 1][2] > 0 for c in scored)            # the comparison is not of zeros
    # the per-pair function, numpy and device tensors
    c = scored[-1]
    exp = test_2D.calculate_metric_percase(pred == c, lab == c)
    assert eval_surface.calculate_metric_percase_2d(pred == c, lab == c) == exp
    _same(eval_surface.calculate_metric_percase_2d(pred == c, lab == c, surface="gpu"), exp)
    _same(eval_surface.calculate_metric_percase_2d(torch.from_numpy(pred == c).cuda(), torch.from_numpy(lab == c).cuda(), surface="gpu"), exp)
    # the reference's empty-set conventions hold on the GPU route too
    assert eval_surface.calculate_metric_percase_2d(np.zeros((4, 4)), np.ones((4, 4)), surface="gpu") == (0.0, 0.0, 0.0, 0.0)
    assert eval_surface.calculate_metric_percase_2d(np.ones((4, 4)), np.zeros((4, 4)), surface="gpu") == (1.0, 1.0, 0.0, 0.0)


def test_all_case_3d_surface_gpu_equals_host():
    from arco_amd import eval_surface, test_util
    from arco_amd.networks.vnetWithArgs import VNet
    from arco_amd.utils import metrics
    shape, patch, sxy, sz, C, nf, seed = fx.EVAL3D_CASES["ragged"]
    net = VNet(n_channels=1, n_classes=C, n_filters=nf, normalization='batchnorm', has_dropout=False).cuda()
    net.load_state_dict(fx.randomize_running_stats(fx.vnet_state(seed, 1, C, nf), seed + 1), strict=True)
    image = fx.eval3d_volume(seed + 2, shape)
    pred, _ = test_util.test_single_case(net, image, sxy, sz, patch, num_classes=C)
    other = np.roll(pred, 2, axis=0)
    assert pred.any() and other.any()
    host = test_util.calculate_metric_percase(pred, other)
    assert host[2] > 0 and host[3] > 0
    _same(eval_surface.calculate_metric_percase_3d(pred, other, surface="gpu"), host)
    _same(metrics.calculate_metric_percase(pred, other, surface="gpu"), metrics.calculate_metric_percase(pred, other))
    cases = [(image, other), (image, pred)]
    kw = dict(patch_size=patch, stride_xy=sxy, stride_z=sz)
    avg_host = test_util.test_all_case(net, cases, C, **kw)
    avg_gpu = eval_surface.test_all_case(net, cases, C, surface="gpu", **kw)
    assert avg_gpu.shape == (4,) and np.array_equal(avg_gpu[:3], avg_host[:3]) and avg_host[2] > 0
    np.testing.assert_allclose(avg_gpu[3], avg_host[3], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, **kw), avg_host)   # the default is the host route
    np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, surface="host", **kw), avg_host)
