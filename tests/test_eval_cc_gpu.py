"""eval_surface.test_all_case with cc="gpu" (the device-resident tail: predict_case -> cc_gpu.largest_cc -> overlap counts and surface
histograms on device tensors) against cc="host" (test_single_case -> getLargestCC on the host), both with surface="gpu": dice, jc and
hd95 equal (==), asd to rtol 1e-12 - the masks are identical, only the order of one float64 sum may differ.  The network and the
volumes are those of tests/test_eval_surface_gpu.py; one volume is ragged against the patch, one smaller than it (padded)."""
import numpy as np
import pytest
import torch

import fixture_inputs as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    """(net, kw, [(image, prediction of test_single_case), ...]): the ragged volume and a padded one, predicted once."""
    from arco_amd import test_util
    from arco_amd.networks.vnetWithArgs import VNet
    shape, patch, sxy, sz, C, nf, seed = fx.EVAL3D_CASES["ragged"]
    net = VNet(n_channels=1, n_classes=C, n_filters=nf, normalization='batchnorm', has_dropout=False).cuda()
    net.load_state_dict(fx.randomize_running_stats(fx.vnet_state(seed, 1, C, nf), seed + 1), strict=True)
    kw = dict(patch_size=patch, stride_xy=sxy, stride_z=sz)
    vols = []
    for i, shp in enumerate((shape, fx.EVAL3D_CASES["padded"][0])):
        image = fx.eval3d_volume(seed + 2 + i, shp)
        pred, _ = test_util.test_single_case(net, image, sxy, sz, patch, num_classes=C)
        assert pred.shape == shp and pred.any() and not pred.all()
        vols.append((image, pred))
    assert any(s < p for s, p in zip(vols[1][0].shape, patch))                         # the second one is padded
    return net, C, kw, vols


def _same(got, exp):
    assert got.shape == exp.shape == (4,)
    assert np.array_equal(got[:3], exp[:3]), (got, exp)
    np.testing.assert_allclose(got[3], exp[3], rtol=1e-12, atol=0)


def test_predict_case_is_the_label_map_of_test_single_case(setup):
    from arco_amd import eval_surface
    net, C, kw, vols = setup
    for image, pred in vols:
        got = eval_surface.predict_case(net, image, kw["stride_xy"], kw["stride_z"], kw["patch_size"], C)
        assert got.is_cuda and got.dtype == torch.int64 and got.is_contiguous() and tuple(got.shape) == image.shape
        assert np.array_equal(got.cpu().numpy(), pred)


@pytest.mark.parametrize("nms", [1, 0])
def test_all_case_cc_gpu_equals_cc_host(setup, nms):
    from arco_amd import eval_surface
    net, C, kw, vols = setup
    cases = [(image, np.roll(pred, 2, axis=0)) for image, pred in vols] + [(vols[0][0], vols[0][1])]
    host = eval_surface.test_all_case(net, cases, C, nms=nms, surface="gpu", cc="host", **kw)
    assert host[0] > 0 and host[2] > 0 and host[3] > 0                                 # the comparison is not of zeros
    _same(eval_surface.test_all_case(net, cases, C, nms=nms, surface="gpu", cc="gpu", **kw), host)
    np.testing.assert_array_equal(eval_surface.test_all_case(net, cases, C, nms=nms, surface="gpu", **kw), host)   # the default is "host"


def test_nms_changes_the_prediction(setup):
    """The largest component is a proper subset of the foreground in at least one volume, so cc="gpu" with nms=1 is held to more than
    the identity."""
    from arco_amd.test_util import getLargestCC
    from arco_amd.utils import cc_gpu
    _, _, _, vols = setup
    shrunk = 0
    for _, pred in vols:
        host = getLargestCC(pred)
        assert np.array_equal(cc_gpu.largest_cc(torch.from_numpy(pred).cuda()).cpu().numpy(), host)
        shrunk += int(host.sum() < (pred != 0).sum())
    assert shrunk > 0


class _Background(torch.nn.Module):
    """Logits that favour class 0 everywhere."""

    def forward(self, x):
        y = torch.zeros((x.shape[0], 2, *x.shape[2:]), dtype=torch.float32, device=x.device)
        y[:, 0] = 4.0
        return y


def test_all_background_prediction_scores_zero_on_both_routes(setup):
    from arco_amd import eval_surface
    _, _, kw, vols = setup
    net = _Background().cuda()
    cases = [(image, pred) for image, pred in vols]
    for cc in ("host", "gpu"):
        avg = eval_surface.test_all_case(net, cases, 2, nms=0, surface="gpu", cc=cc, **kw)
        assert avg.tolist() == [0.0, 0.0, 0.0, 0.0], cc
        with pytest.raises(AssertionError):                                            # getLargestCC's `assert n != 0`, on both routes
            eval_surface.test_all_case(net, cases, 2, nms=1, surface="gpu", cc=cc, **kw)
