"""The evaluation entry points with a choice of route for hd95 / asd: `surface="host"` (default: scipy on the host, exactly what
arco_amd.test_2D / arco_amd.test_util do - those calls are passed through untouched) or `surface="gpu"` (the HIP surface-distance
kernels, utils/surface_gpu.py: hd95 equal, asd to the order of one float64 sum; unit voxel spacing and connectivity 1, which is all
the reference asks medpy for).  Any other value is a ValueError, raised before any GPU work.

  2-D (test_2D.py:52-92)       calculate_metric_percase_2d, test_single_volume
  3-D (test_util.py:39-79,214) calculate_metric_percase_3d, test_all_case
Inference, the zoom round trip, the sliding window, the overlap counts and the empty-set conventions are those modules' own."""
import numpy as np
import torch

from . import test_2D as _t2d
from . import test_util as _t3d
from .utils import surface_gpu as _surface_gpu
from .utils.metrics import binary as _binary


def calculate_metric_percase_2d(pred, gt, surface="host"):
    """(dice, jc, hd95, asd) of two binary masks (numpy or torch) with test_2D.calculate_metric_percase's conventions."""
    if _surface_gpu.check_route(surface) == "host":
        return _t2d.calculate_metric_percase(pred, gt)
    p = (pred if torch.is_tensor(pred) else torch.from_numpy(np.asarray(pred) > 0)) > 0
    g = (gt if torch.is_tensor(gt) else torch.from_numpy(np.asarray(gt) > 0)) > 0
    n_pred, n_gt, n_both = int(p.sum()), int(g.sum()), int((p & g.to(p.device)).sum())
    dice, jc = _t2d._dice_jc(n_pred, n_gt, n_both)
    hd95 = asd = 0.0
    if n_pred > 0 and n_gt > 0:
        hd95, asd = _surface_gpu.pair_metrics(p, g)
    return dice, jc, hd95, asd


@torch.no_grad()
def test_single_volume(image, label, net, classes, patch_size=(256, 256), device="cuda:0", surface="host"):
    """test_2D.test_single_volume; with surface="gpu" the surface metrics of all classes come from one call on the label volumes that
    are on the device for the overlap counts already."""
    if _surface_gpu.check_route(surface) == "host":
        return _t2d.test_single_volume(image, label, net, classes, patch_size, device=device)
    prediction = _t2d.predict_volume(image, net, patch_size, device=device)
    pred_d, lab_d = torch.from_numpy(prediction).to(device), torch.from_numpy(np.asarray(label, dtype=np.int64)).to(device)
    cnt = _t2d.overlap_counts(pred_d, lab_d, classes).cpu().numpy()
    scored = _surface_gpu.surface_metrics(pred_d, lab_d, range(1, classes)) if classes > 1 else []
    metric_list = []
    for c in range(1, classes):
        dice, jc = _t2d._dice_jc(int(cnt[c, 0]), int(cnt[c, 1]), int(cnt[c, 2]))
        hd95 = asd = 0.0
        if cnt[c, 0] > 0 and cnt[c, 1] > 0:
            hd95, asd = scored[c - 1]
        metric_list.append((dice, jc, hd95, asd))
    return metric_list


def calculate_metric_percase_3d(pred, gt, surface="host"):
    """(dice, jc, hd95, asd) as test_util.calculate_metric_percase; with surface="gpu" both surface metrics from one histogram call."""
    if _surface_gpu.check_route(surface) == "host":
        return _t3d.calculate_metric_percase(pred, gt)
    return (_binary.dc(pred, gt), _binary.jc(pred, gt)) + _surface_gpu.pair_metrics(pred, gt)


def test_all_case(model, cases, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4, preproc_fn=None,
                  metric_detail=0, nms=0, device="cuda:0", surface="host"):
    """test_util.test_all_case: the mean (dice, jc, hd95, asd) over `cases` (an all-background prediction scores (0, 0, 0, 0))."""
    if _surface_gpu.check_route(surface) == "host":
        return _t3d.test_all_case(model, cases, num_classes, patch_size=patch_size, stride_xy=stride_xy, stride_z=stride_z,
                                  preproc_fn=preproc_fn, metric_detail=metric_detail, nms=nms, device=device)
    total, n = np.zeros(4), 0
    for ith, (image, label) in enumerate(cases):
        if preproc_fn is not None:
            image = preproc_fn(image)
        prediction, _ = _t3d.test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, device=device)
        if nms:
            prediction = _t3d.getLargestCC(prediction)
        single = (0, 0, 0, 0) if np.sum(prediction) == 0 else calculate_metric_percase_3d(prediction, np.asarray(label), surface)
        if metric_detail:
            print('%02d,\t%.5f, %.5f, %.5f, %.5f' % (ith, *single))
        total += np.asarray(single, dtype=np.float64)
        n += 1
    avg = total / max(n, 1)
    print('average metric is {}'.format(avg))
    return avg
