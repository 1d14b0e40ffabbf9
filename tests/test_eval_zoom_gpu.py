"""2-D evaluation with the zoom round trip on the GPU (arco_amd/eval_surface.py, zoom="gpu") against the host route, which is
arco_amd.test_2D.predict_volume itself (scipy's zoom(order=0) twice per slice): the same label map (array_equal) and, through the same
kernels, the same four numbers of every class (==).  The network, its randomised running statistics and the blob labels are those of
tests/test_eval_surface_gpu.py; the two volumes are cases of tests/zoom_kernel_refs.py whose forward zoom zeroes a last row (and
column) of the image."""
import numpy as np
import pytest
import torch

import fixture_inputs as fx
import zoom_kernel_refs as R

pytestmark = pytest.mark.gpu

C = 4
VOLUMES = [((5, 28, 47), (48, 64)), ((3, 55, 58), (48, 48))]


@pytest.fixture(scope="module")
def net():
    from arco_amd.networks.unetWithArgs import UNet
    sd = fx.unet_state(21, 1, C)
    rs = np.random.RandomState(4)
    for k in list(sd):
        if k.endswith("running_mean"):
            sd[k] = torch.from_numpy(rs.normal(scale=0.1, size=tuple(sd[k].shape)).astype(np.float32))
        if k.endswith("running_var"):
            sd[k] = torch.from_numpy(rs.uniform(0.5, 1.5, size=tuple(sd[k].shape)).astype(np.float32))
    net = UNet(1, C).cuda()
    net.load_state_dict(sd, strict=True)
    return net


def _volume(shape):
    rs = np.random.RandomState(sum(shape))
    img = rs.uniform(size=shape).astype(np.float32)
    lab = np.stack([fx.blob_labels(rs, 1, shape[1:], C)[0] for _ in range(shape[0])]).astype(np.int64)
    return img, lab


@pytest.mark.parametrize("shape,patch", VOLUMES, ids=["5x28x47", "3x55x58"])
def test_zoom_gpu_equals_host(net, shape, patch):
    from arco_amd import eval_surface, test_2D
    assert (patch, shape[1:]) in R.CASES[:2]
    img, lab = _volume(shape)
    host_pred = test_2D.predict_volume(img, net, patch)
    for training in (False, True):                                     # the mode is restored, and an eval-mode net stays in eval mode
        net.train(training)
        pred = eval_surface.predict_volume(img, net, patch, zoom="gpu")
        assert net.training is training
        assert torch.is_tensor(pred) and pred.is_cuda and pred.dtype == torch.int64 and tuple(pred.shape) == shape
        assert np.array_equal(pred.cpu().numpy(), host_pred)
    net.eval()
    assert np.array_equal(eval_surface.predict_volume(img, net, patch, batch=2, zoom="gpu").cpu().numpy(),
                          test_2D.predict_volume(img, net, patch, batch=2))                        # several batches, the last one short
    # the defaults and zoom="host" are the host route: a numpy array, what test_2D returns
    for kw in ({}, {"zoom": "host"}):
        p = eval_surface.predict_volume(img, net, patch, **kw)
        assert isinstance(p, np.ndarray) and p.dtype == np.int64 and np.array_equal(p, host_pred)
    assert len(np.unique(host_pred)) > 1

    surf = eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu")
    both = eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu")
    assert len(both) == C - 1 and both == surf                         # the same label map through the same kernels: all four numbers, ==
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="host") == surf
    assert any(m[2] > 0 for m in both)                                 # the comparison is not of zeros
    host = test_2D.test_single_volume(img, lab, net, C, patch)
    assert eval_surface.test_single_volume(img, lab, net, C, patch) == host
    assert eval_surface.test_single_volume(img, lab, net, C, patch, zoom="host") == host
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="host", zoom="host") == host
    net.train()
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu") == surf and net.training
    net.eval()
