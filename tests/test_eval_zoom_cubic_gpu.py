"""2-D evaluation with the cubic-spline zoom of the slices (order=3, the route of the reference's test.py:116-135) on the GPU
(arco_amd/eval_surface.py, zoom="gpu") against the host route, which is scipy.ndimage.zoom(order=3) per slice in
eval_surface.predict_volume(zoom="host", order=3): the same label map (array_equal) and, through the same kernels, the same four numbers of
every class (==).  The network and the blob volumes are those of tests/test_eval_zoom_gpu.py.  Three volumes: one whose forward zoom
zeroes the last image row, one with slices of patch size (the skip rule: no zoom either way), one with ONE axis of patch size (zoomed
all the same, test.py:123).  On their slices the float64 restatement of tests/zoom_cubic_kernel_refs.py equals scipy on every output
(asserted here, on the CPU), so the device route, which is held to the restatement bit for bit, has the host route's network input."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

import zoom_cubic_kernel_refs as R
from test_eval_zoom_gpu import C, _volume, net  # noqa: F401  (the U-Net fixture and the volumes of the order-0 test)

pytestmark = pytest.mark.gpu

VOLUMES = [((5, 28, 47), (48, 64)), ((3, 48, 48), (48, 48)), ((4, 48, 40), (48, 64))]
IDS = ["5x28x47", "3x48x48_patch_size", "4x48x40_one_axis_kept"]


@pytest.mark.parametrize("shape,patch", VOLUMES, ids=IDS)
def test_order3_zoom_gpu_equals_host(net, shape, patch):
    from arco_amd import eval_surface, test_2D
    from arco_amd.utils import zoom_gpu
    img, lab = _volume(shape)
    as_is = shape[1:] == patch
    if not as_is:
        exp = np.stack([zoom(img[s], (patch[0] / shape[1], patch[1] / shape[2]), order=3) for s in range(shape[0])])
        assert np.array_equal(R.ref_zoom_cubic(img, patch), exp)                  # the restatement is scipy on these slices, exactly
        assert np.array_equal(zoom_gpu.zoom_cubic(torch.from_numpy(img).cuda(), patch).cpu().numpy(), exp)
        assert bool((exp[:, -1, :] == 0).all()) == (shape[1] == 28) and (exp[:, :-1, :] != 0).all()
    host_pred = eval_surface.predict_volume(img, net, patch, zoom="host", order=3)
    assert isinstance(host_pred, np.ndarray) and host_pred.dtype == np.int64 and host_pred.shape == shape
    for training in (False, True):                                     # the mode is restored, and an eval-mode net stays in eval mode
        net.train(training)
        pred = eval_surface.predict_volume(img, net, patch, zoom="gpu", order=3)
        assert net.training is training
        assert torch.is_tensor(pred) and pred.is_cuda and pred.dtype == torch.int64 and tuple(pred.shape) == shape
        assert np.array_equal(pred.cpu().numpy(), host_pred)
        assert np.array_equal(eval_surface.predict_volume(img, net, patch, zoom="host", order=3), host_pred) and net.training is training
    net.eval()
    assert np.array_equal(eval_surface.predict_volume(img, net, patch, batch=2, zoom="gpu", order=3).cpu().numpy(),
                          eval_surface.predict_volume(img, net, patch, batch=2, order=3))          # several batches, the last one short
    assert np.array_equal(eval_surface.predict_volume(img, net, patch, batch=2, order=3), host_pred)
    assert len(np.unique(host_pred)) > 1

    # order=0 and the default return what they return today; order 3 is another label map wherever a slice is zoomed at all
    pred0 = test_2D.predict_volume(img, net, patch)
    for kw in ({}, {"order": 0}):
        assert np.array_equal(eval_surface.predict_volume(img, net, patch, **kw), pred0)
        assert np.array_equal(eval_surface.predict_volume(img, net, patch, zoom="gpu", **kw).cpu().numpy(), pred0)
    if as_is:
        assert np.array_equal(host_pred, pred0)                        # neither order resamples a slice of patch size
    else:
        assert (host_pred != pred0).any()

    surf = eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="host", order=3)
    both = eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu", order=3)
    assert len(both) == C - 1 and both == surf                         # the same label map through the same kernels: all four numbers, ==
    assert any(m[2] > 0 for m in both)                                 # the comparison is not of zeros
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", order=3) == surf
    host = eval_surface.test_single_volume(img, lab, net, C, patch, order=3)          # surface="host": medpy's distances on the same map
    assert [m[:2] for m in host] == [m[:2] for m in surf] and [m[2] for m in host] == [m[2] for m in surf]
    today = test_2D.test_single_volume(img, lab, net, C, patch)
    assert eval_surface.test_single_volume(img, lab, net, C, patch) == today
    assert eval_surface.test_single_volume(img, lab, net, C, patch, order=0) == today
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu", order=0) == \
        eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu")
    if not as_is:
        assert both != eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu")
    net.train()
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu", order=3) == surf and net.training
    net.eval()


def test_order3_with_nms_on_the_device(net):
    """order=3 works with nms / cc="gpu" exactly as order 0 does: the device-resident case equals the host-zoom, host-cc case."""
    from arco_amd import eval_surface
    shape, patch = VOLUMES[0]
    img, lab = _volume(shape)
    ref = eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="host", nms=1, cc="host", order=3)
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu", nms=1, cc="gpu", order=3) == ref
    assert eval_surface.test_single_volume(img, lab, net, C, patch, surface="gpu", zoom="gpu", nms=1, cc="host", order=3) == ref


def test_order3_device_route_refuses_a_float64_volume(net):
    from arco_amd import eval_surface
    shape, patch = VOLUMES[0]
    img, _ = _volume(shape)
    with pytest.raises(ValueError, match="float32"):
        eval_surface.predict_volume(img.astype(np.float64), net, patch, zoom="gpu", order=3)
    assert eval_surface.predict_volume(img.astype(np.float64), net, patch, zoom="gpu").dtype == torch.int64      # order 0 takes it, as before
