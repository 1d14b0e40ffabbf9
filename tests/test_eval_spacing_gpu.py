"""The evaluation entry points of arco_amd/eval_surface.py with metrics.binary's `voxelspacing` and `connectivity`: surface="gpu" (the
float64 record kernels, utils/surface_gpu.spaced_*) against surface="host" (metrics.binary with the same arguments on the label map of
the same predict functions) - dice / jc equal (==), hd95 / asd to rtol 1e-12 (per distance the two routes differ by at most
4 * 2^-52, tests/surface_sp_kernel_refs.py; then one float64 mean and one interpolated percentile) - and, with both keywords at their
defaults, exactly what each function returned before it had them.  The networks and volumes are those of tests/test_eval_zoom_gpu.py
and tests/test_eval_cc_gpu.py."""
import numpy as np
import pytest
import torch

import fixture_inputs as fx

pytestmark = pytest.mark.gpu

VS = (10.0, 1.25, 1.25)                      # ACDC: 1.25 x 1.25 mm in the slice, 10 mm between slices
C2 = 4


def _close(got, exp):
    """(dice, jc, hd95, asd): the overlap numbers equal, the surface numbers to rtol 1e-12."""
    assert got[0] == exp[0] and got[1] == exp[1], (got, exp)
    np.testing.assert_allclose(got[2:], exp[2:], rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def net2d():
    from arco_amd.networks.unetWithArgs import UNet
    sd = fx.unet_state(21, 1, C2)
    rs = np.random.RandomState(4)
    for k in list(sd):
        if k.endswith("running_mean"):
            sd[k] = torch.from_numpy(rs.normal(scale=0.1, size=tuple(sd[k].shape)).astype(np.float32))
        if k.endswith("running_var"):
            sd[k] = torch.from_numpy(rs.uniform(0.5, 1.5, size=tuple(sd[k].shape)).astype(np.float32))
    net = UNet(1, C2).cuda()
    net.load_state_dict(sd, strict=True)
    return net.eval()


@pytest.fixture(scope="module")
def setup3d():
    """(net, C, kw, image, prediction of test_single_case) on the ragged volume."""
    from arco_amd import test_util
    from arco_amd.networks.vnetWithArgs import VNet
    shape, patch, sxy, sz, C, nf, seed = fx.EVAL3D_CASES["ragged"]
    net = VNet(n_channels=1, n_classes=C, n_filters=nf, normalization='batchnorm', has_dropout=False).cuda()
    net.load_state_dict(fx.randomize_running_stats(fx.vnet_state(seed, 1, C, nf), seed + 1), strict=True)
    kw = dict(patch_size=patch, stride_xy=sxy, stride_z=sz)
    image = fx.eval3d_volume(seed + 2, shape)
    pred, _ = test_util.test_single_case(net, image, sxy, sz, patch, num_classes=C)
    assert pred.any() and not pred.all()
    return net, C, kw, image, pred


def test_single_volume_with_spacing(net2d):
    from arco_amd import eval_surface, test_2D
    from arco_amd.utils import metrics, surface_gpu
    shape, patch = (5, 28, 47), (48, 64)
    rs = np.random.RandomState(sum(shape))
    img = rs.uniform(size=shape).astype(np.float32)
    lab = np.stack([fx.blob_labels(rs, 1, shape[1:], C2)[0] for _ in range(shape[0])]).astype(np.int64)
    pred = test_2D.predict_volume(img, net2d, patch)
    scored = [c for c in range(1, C2) if (pred == c).any() and (lab == c).any()]
    assert scored
    for conn in (1, 2):
        host = eval_surface.test_single_volume(img, lab, net2d, C2, patch, surface="host", voxelspacing=VS, connectivity=conn)
        assert len(host) == C2 - 1
        unit = test_2D.test_single_volume(img, lab, net2d, C2, patch)
        for c in range(1, C2):                                           # the host route is metrics.binary with the two arguments
            assert host[c - 1][:2] == unit[c - 1][:2]
            if c in scored:
                assert host[c - 1][2] == metrics.binary.hd95(pred == c, lab == c, VS, conn)
                assert host[c - 1][3] == metrics.binary.asd(pred == c, lab == c, VS, conn)
                assert host[c - 1][2] != unit[c - 1][2]                  # the spacing is not ignored
            else:
                assert host[c - 1][2:] == (0.0, 0.0)
        for zoom in ("host", "gpu"):
            gpu = eval_surface.test_single_volume(img, lab, net2d, C2, patch, surface="gpu", zoom=zoom, voxelspacing=VS, connectivity=conn)
            assert len(gpu) == C2 - 1
            for g, h in zip(gpu, host):
                _close(g, h)
    # the per-pair function on one slice: a 2-D map has two spacings
    c = scored[-1]
    s = next(i for i in range(shape[0]) if (pred[i] == c).any() and (lab[i] == c).any())
    exp = eval_surface.calculate_metric_percase_2d(pred[s] == c, lab[s] == c, voxelspacing=(1.25, 2.5), connectivity=2)
    assert exp[2:] == (metrics.binary.hd95(pred[s] == c, lab[s] == c, (1.25, 2.5), 2), metrics.binary.asd(pred[s] == c, lab[s] == c, (1.25, 2.5), 2))
    assert exp[:2] == test_2D.calculate_metric_percase(pred[s] == c, lab[s] == c)[:2]
    _close(eval_surface.calculate_metric_percase_2d(pred[s] == c, lab[s] == c, surface="gpu", voxelspacing=(1.25, 2.5), connectivity=2), exp)
    _close(eval_surface.calculate_metric_percase_2d(torch.from_numpy(pred[s] == c).cuda(), torch.from_numpy(lab[s] == c).cuda(), surface="gpu",
                                                    voxelspacing=(1.25, 2.5), connectivity=2), exp)
    assert eval_surface.calculate_metric_percase_2d(np.zeros((4, 4)), np.ones((4, 4)), surface="gpu", voxelspacing=2.0) == (0.0, 0.0, 0.0, 0.0)
    assert eval_surface.calculate_metric_percase_2d(np.ones((4, 4)), np.zeros((4, 4)), surface="gpu", voxelspacing=2.0) == (1.0, 1.0, 0.0, 0.0)

    # both keywords at their defaults: today's paths
    assert eval_surface.test_single_volume(img, lab, net2d, C2, patch, voxelspacing=None, connectivity=1) == unit
    lab_d, pred_d = torch.from_numpy(lab).cuda(), torch.from_numpy(pred).cuda()
    cnt = test_2D.overlap_counts(pred_d, lab_d, C2).cpu().numpy()
    ints = surface_gpu.surface_metrics(pred_d, lab_d, range(1, C2))
    today = [test_2D._dice_jc(int(cnt[c, 0]), int(cnt[c, 1]), int(cnt[c, 2])) + (ints[c - 1] if c in scored else (0.0, 0.0))
             for c in range(1, C2)]
    for zoom in ("host", "gpu"):
        assert eval_surface.test_single_volume(img, lab, net2d, C2, patch, surface="gpu", zoom=zoom) == today
        assert eval_surface.test_single_volume(img, lab, net2d, C2, patch, surface="gpu", zoom=zoom, voxelspacing=None, connectivity=1) == today
    assert (eval_surface.calculate_metric_percase_2d(pred[s] == c, lab[s] == c, surface="gpu", voxelspacing=None, connectivity=1)
            == test_2D.calculate_metric_percase(pred[s] == c, lab[s] == c)[:2] + surface_gpu.pair_metrics(pred[s] == c, lab[s] == c))


def test_metric_percase_3d_with_spacing(setup3d):
    from arco_amd import eval_surface, test_util
    from arco_amd.utils import metrics, surface_gpu
    _, _, _, _, pred = setup3d
    other = np.roll(pred, 2, axis=0)
    for conn in (1, 3):
        host = eval_surface.calculate_metric_percase_3d(pred, other, surface="host", voxelspacing=VS, connectivity=conn)
        assert host == (metrics.binary.dc(pred, other), metrics.binary.jc(pred, other), metrics.binary.hd95(pred, other, VS, conn),
                        metrics.binary.asd(pred, other, VS, conn))
        assert host[2] > 0 and host[3] > 0
        _close(eval_surface.calculate_metric_percase_3d(pred, other, surface="gpu", voxelspacing=VS, connectivity=conn), host)
    assert host[2] != metrics.binary.hd95(pred, other)
    _close(eval_surface.calculate_metric_percase_3d(pred, other, surface="gpu", voxelspacing=0.5),
           eval_surface.calculate_metric_percase_3d(pred, other, voxelspacing=0.5))
    # defaults: today's paths
    today_host = test_util.calculate_metric_percase(pred, other)
    assert eval_surface.calculate_metric_percase_3d(pred, other, voxelspacing=None, connectivity=1) == today_host
    today_gpu = (metrics.binary.dc(pred, other), metrics.binary.jc(pred, other)) + surface_gpu.pair_metrics(pred, other)
    assert eval_surface.calculate_metric_percase_3d(pred, other, surface="gpu") == today_gpu
    assert eval_surface.calculate_metric_percase_3d(pred, other, surface="gpu", voxelspacing=None, connectivity=1) == today_gpu


def test_all_case_with_spacing(setup3d):
    from arco_amd import eval_surface, test_util
    net, C, kw, image, pred = setup3d
    cases = [(image, np.roll(pred, 2, axis=0)), (image, pred)]
    host = eval_surface.test_all_case(net, cases, C, nms=1, surface="host", voxelspacing=VS, **kw)
    assert host.shape == (4,) and host[0] > 0 and host[2] > 0 and host[3] > 0
    unit = test_util.test_all_case(net, cases, C, nms=1, **kw)
    assert np.array_equal(host[:2], unit[:2]) and host[2] != unit[2]     # the same masks, other distances
    for cc in ("gpu", "host"):
        got = eval_surface.test_all_case(net, cases, C, nms=1, surface="gpu", cc=cc, voxelspacing=VS, **kw)
        assert got.shape == (4,) and np.array_equal(got[:2], host[:2]), (cc, got, host)
        np.testing.assert_allclose(got[2:], host[2:], rtol=1e-12, atol=0)
    # defaults: today's paths
    np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, nms=1, voxelspacing=None, connectivity=1, **kw), unit)
    today = eval_surface.test_all_case(net, cases, C, nms=1, surface="gpu", cc="gpu", **kw)
    assert np.array_equal(today[:3], unit[:3])
    np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, nms=1, surface="gpu", cc="gpu", voxelspacing=None, connectivity=1,
                                                             **kw), today)
