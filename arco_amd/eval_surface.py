"""The evaluation entry points with a choice of route for hd95 / asd: `surface="host"` (default: scipy on the host, exactly what
arco_amd.test_2D / arco_amd.test_util do - those calls are passed through untouched) or `surface="gpu"` (the HIP surface-distance
kernels, utils/surface_gpu.py: hd95 equal, asd to the order of one float64 sum; unit voxel spacing and connectivity 1, which is all
the reference asks medpy for).  Any other value is a ValueError, raised before any GPU work.

  2-D (test_2D.py:52-92)       calculate_metric_percase_2d, test_single_volume
  3-D (test_util.py:39-79,214) calculate_metric_percase_3d, test_all_case, predict_case
test_all_case also takes `cc="host"` (default: getLargestCC on the host for `nms`) or `cc="gpu"` (with surface="gpu" only: the label map
stays on the device from the arg-max through the largest component, utils/cc_gpu.py, to the four metrics).
predict_volume and test_single_volume take `zoom="host"` (default: test_2D.predict_volume, scipy's zoom(order=0) on the host twice per
slice) or `zoom="gpu"` (utils/zoom_gpu.py: the volume is uploaded once, resampled to the patch on the device, and the arg-max map is
resampled back by the kernel that takes the arg-max - the same label map, bit for bit, as a device tensor; in test_single_volume with
surface="gpu" only, where it goes on to the overlap counts and the surface kernels without leaving the device).
Both also take `order=0` (default: every path exactly as without the keyword) or `order=3`, the route of the reference's
test.py:116-135: a slice whose size differs from the patch goes to the patch by the cubic-spline zoom (scipy.ndimage.zoom(order=3) on
zoom="host"; zoom_gpu.zoom_cubic, its float64 prefilter and interpolation as HIP kernels, on zoom="gpu"), a slice of patch size is passed
as it is, and the arg-max map goes back by order 0 as before.  On zoom="gpu" an order-3 volume must be float32 (the cast does not
commute with the spline; ValueError otherwise).  Any other order is a ValueError before any GPU work.
The metric functions, test_single_volume and test_all_case also take metrics.binary's `voxelspacing=None, connectivity=1` (medpy's
meaning: None is 1.0, a number is broadcast, a sequence has one entry per axis of the scored map - three for the [S, X, Y] volume of
test_single_volume; connectivity 1..ndim).  With both at their defaults every function takes the path it took without them.  Otherwise
surface="host" gives hd95 / asd from metrics.binary with the two arguments on the label map of the same predict functions, and
surface="gpu" from surface_gpu.spaced_metrics / spaced_pair_metrics (float64 records, csrc/surface.hip) on the device tensors that are
there already - zoom="gpu" and cc="gpu" included.  A bad spacing or connectivity is a ValueError before any GPU work.
What `nms` keeps: test_all_case takes `nms_mode="foreground"` (default: getLargestCC / largest_cc, every non-zero label one foreground),
"value" (the reference's own meaning through skimage.measure.label: the largest component of EQUAL values, cc_host.getLargestCC_by_value
/ cc_gpu.largest_cc_by_value) or "per_class" (the largest component of every class, cc_host.keep_largest_per_class /
cc_gpu.largest_per_class); the keyword is read only when `nms` is set, any other value is a ValueError before any GPU work.
test_single_volume takes `nms=0, cc="host"`: nms=1 keeps each class's largest component of the [S, X, Y] prediction (csrc/cc.hip by value on
cc="gpu", which needs surface="gpu") before the overlap counts and the surface metrics.
predict_volume, test_single_volume, predict_case and test_all_case take `act_dtype="f32"` (default: every path exactly as without the
keyword) or "f16": the forwards of that call run inside `ops.eval_half()` - the U-Net / the V-Net (batchnorm) keep their activations as
f16 -, everything before and after them is unchanged.  With zoom="gpu" predict_volume takes the logits as the f16 tensor the last
convolution wrote (`eval_half(logits="stored")`) into arco_argmax_zoom_back2d_h; on zoom="host" and in predict_case the logits leave as
fp32 and go through the same softmax / window kernels as before.  The switches of `ops` are put back when the call returns or raises.
Any other value is a ValueError before any GPU work.
Inference, the sliding window, the overlap counts and the empty-set conventions are those modules' own."""
import contextlib

import numpy as np
import torch

from . import _lib as _L
from . import glue as _glue
from . import ops as _ops
from . import test_2D as _t2d
from . import test_util as _t3d
from .utils import cc_gpu as _cc_gpu
from .utils import cc_host as _cc_host
from .utils import surface_gpu as _surface_gpu
from .utils import zoom_gpu as _zoom_gpu
from .utils.metrics import binary as _binary


def _unit(voxelspacing, connectivity):
    """Both surface arguments at their defaults: the unit-spacing, connectivity-1 paths."""
    return voxelspacing is None and isinstance(connectivity, int) and connectivity == 1


def _pair_device(pred, gt, voxelspacing, connectivity):
    """(hd95, asd) of one mask pair from the surface kernels: the integer histogram at the defaults, else the float64 records."""
    if _unit(voxelspacing, connectivity):
        return _surface_gpu.pair_metrics(pred, gt)
    return _surface_gpu.spaced_pair_metrics(pred, gt, voxelspacing, connectivity)


def _classes_device(pred, gt, classes, voxelspacing, connectivity):
    """[(hd95, asd) or None] per class of two label tensors on the device, by the same choice."""
    if _unit(voxelspacing, connectivity):
        return _surface_gpu.surface_metrics(pred, gt, classes)
    return _surface_gpu.spaced_metrics(pred, gt, classes, voxelspacing, connectivity)


# what `nms` keeps: nms_mode -> (host function of the label map, device function of the label map and the class count)
_NMS = {"foreground": (_t3d.getLargestCC, lambda x, classes: _cc_gpu.largest_cc(x)),
        "value": (_cc_host.getLargestCC_by_value, _cc_gpu.largest_cc_by_value),
        "per_class": (_cc_host.keep_largest_per_class, _cc_gpu.largest_per_class)}
NMS_MODES = tuple(_NMS)


def _check_nms_mode(nms_mode):
    """The `nms_mode=` keyword of test_all_case: what `nms` keeps."""
    if nms_mode not in NMS_MODES:
        raise ValueError(f"nms_mode must be one of {NMS_MODES}, got {nms_mode!r}")
    return nms_mode


ACT_DTYPES = ("f32", "f16")


def check_act_dtype(act_dtype):
    """The `act_dtype=` keyword of the inference entry points: "f32" (default) or "f16" (the forwards inside `ops.eval_half()`)."""
    if act_dtype not in ACT_DTYPES:
        raise ValueError(f"act_dtype must be one of {ACT_DTYPES}, got {act_dtype!r}")
    return act_dtype


def _act_scope(act_dtype, logits="f32"):
    """The scope the forwards of a call run in: `ops.eval_half` for "f16", nothing for "f32"."""
    return _ops.eval_half(logits=logits) if act_dtype == "f16" else contextlib.nullcontext()


def _shape(x):
    return tuple(x.shape) if torch.is_tensor(x) else np.shape(x)


def _metric_list(cnt, classes, surface_of):
    """test_single_volume's [(dice, jc, hd95, asd)] per class from the overlap counts; surface_of(c) is the (hd95, asd) of a class that
    both volumes hold, the others get (0.0, 0.0)."""
    metric_list = []
    for c in range(1, classes):
        dice, jc = _t2d._dice_jc(int(cnt[c, 0]), int(cnt[c, 1]), int(cnt[c, 2]))
        hd95, asd = surface_of(c) if cnt[c, 0] > 0 and cnt[c, 1] > 0 else (0.0, 0.0)
        metric_list.append((dice, jc, hd95, asd))
    return metric_list


def calculate_metric_percase_2d(pred, gt, surface="host", voxelspacing=None, connectivity=1):
    """(dice, jc, hd95, asd) of two binary masks (numpy or torch) with test_2D.calculate_metric_percase's conventions."""
    unit = _unit(voxelspacing, connectivity)
    if _surface_gpu.check_route(surface) == "host" and unit:
        return _t2d.calculate_metric_percase(pred, gt)
    if not unit:
        _surface_gpu.check_spaced_args(voxelspacing, connectivity, len(_shape(pred)))
    if surface == "host":
        pred = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred) > 0
        gt = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt) > 0
        dice, jc = _t2d._dice_jc(int(pred.sum()), int(gt.sum()), int(np.logical_and(pred, gt).sum()))
        hd95 = asd = 0.0
        if pred.sum() > 0 and gt.sum() > 0:
            asd = _binary.asd(pred, gt, voxelspacing, connectivity)
            hd95 = _binary.hd95(pred, gt, voxelspacing, connectivity)
        return dice, jc, hd95, asd
    p = (pred if torch.is_tensor(pred) else torch.from_numpy(np.asarray(pred) > 0)) > 0
    g = (gt if torch.is_tensor(gt) else torch.from_numpy(np.asarray(gt) > 0)) > 0
    n_pred, n_gt, n_both = int(p.sum()), int(g.sum()), int((p & g.to(p.device)).sum())
    dice, jc = _t2d._dice_jc(n_pred, n_gt, n_both)
    hd95 = asd = 0.0
    if n_pred > 0 and n_gt > 0:
        hd95, asd = _pair_device(p, g, voxelspacing, connectivity)
    return dice, jc, hd95, asd


@torch.no_grad()
def _predict_volume_host(image, net, patch_size, batch=32, device="cuda:0", order=0, act_dtype="f32"):
    """The host route's label map, an int64 numpy array.  order=0, act_dtype="f32" is a plain call of test_2D.predict_volume.  Otherwise
    its loop is restated here, order 0 with the two zoom calls as that module makes them and the forward inside `ops.eval_half()` for
    act_dtype="f16" (the logits leave as fp32).  order=3 restates the loop
    (that module stays as it is) with the reference's test.py:116-135 in place of the two zoom calls: a slice goes to the patch by
    scipy's zoom(order=3) only when its size differs from the patch - a slice of patch size is passed as it is, a cubic zoom by 1.0 is
    not the identity in bits - and the arg-max map comes back by order 0 under the same condition."""
    if order == 0 and act_dtype == "f32":
        return _t2d.predict_volume(image, net, patch_size, batch=batch, device=device)
    from scipy.ndimage import zoom
    image = np.asarray(image)
    S, x, y = image.shape
    as_is = order == 3 and (x, y) == (patch_size[0], patch_size[1])          # (order 0 zooms every slice, as test_2D does)
    zoomed = image if as_is else np.stack([zoom(image[i], (patch_size[0] / x, patch_size[1] / y), order=order) for i in range(S)])
    prediction = np.zeros((S, x, y), dtype=np.int64)
    was_training = net.training
    net.eval()
    for s0 in range(0, S, batch):
        inp = torch.from_numpy(np.ascontiguousarray(zoomed[s0:s0 + batch])).unsqueeze(1).float().to(device)
        with _act_scope(act_dtype):
            logits = net(inp)[0]
        out = _glue.softmax_max(logits)[1].cpu().numpy()
        for i in range(out.shape[0]):
            prediction[s0 + i] = out[i] if as_is else zoom(out[i], (x / patch_size[0], y / patch_size[1]), order=0)
    if was_training:
        net.train()
    return prediction


@torch.no_grad()
def predict_volume(image, net, patch_size=(256, 256), batch=32, device="cuda:0", zoom="host", order=0, act_dtype="f32"):
    """Label map of a [S, X, Y] volume.  zoom="host": test_2D.predict_volume, an int64 numpy array.  zoom="gpu": the same label map as an
    int64 tensor ON THE DEVICE - the volume is uploaded once as float32 (nearest sampling and zero fill commute with the cast),
    zoom_gpu.zoom_nearest takes every slice to the patch, the eval-mode net runs in the same batches, and zoom_gpu.argmax_zoom_back
    turns each batch of logits into labels of the slices' own size.  ValueError, before any launch, when scipy's round trip would not
    come back to (X, Y) (the host route fails on its assignment there).
    order=3: the slices go to the patch by the cubic-spline zoom where their size differs from the patch (test.py:123-124) and as they
    are where it does not - scipy's zoom(order=3) on the host, zoom_gpu.zoom_cubic on the device, where the volume must be
    float32 -; the way back is unchanged (at patch size argmax_zoom_back samples every pixel: the arg-max map itself).
    act_dtype="f16": the forwards run inside `ops.eval_half()`; on zoom="gpu" the logits stay the f16 tensor the last convolution
    wrote and argmax_zoom_back reads them as stored (arco_argmax_zoom_back2d_h) - no fp32 logits exist."""
    _zoom_gpu.check_zoom(zoom)
    _zoom_gpu.check_order(order)
    check_act_dtype(act_dtype)
    if zoom == "host":
        return _predict_volume_host(image, net, patch_size, batch=batch, device=device, order=order, act_dtype=act_dtype)
    image = np.asarray(image)
    if order == 3 and image.dtype != np.float32:
        raise ValueError("zoom=\"gpu\", order=3 takes a float32 volume (the cast does not commute with the spline): cast it with "
                         f"image.astype(np.float32) first, got {image.dtype}")
    S, x, y = image.shape
    Z0, Z1 = (_zoom_gpu.zoomed_size(n, p)[0] for n, p in zip((x, y), patch_size))      # scipy's int(round(n * (p / n)))
    back = tuple(int(round(Z * (n / p))) for Z, n, p in zip((Z0, Z1), (x, y), patch_size))
    if min(x, y) < 2:
        raise ValueError(f"zoom=\"gpu\": a slice axis of one point is not supported, got slices of {(x, y)}")
    if back != (x, y):
        raise ValueError(f"zoom(order=0) of a {(Z0, Z1)} map by {(x / patch_size[0], y / patch_size[1])} has shape {back}, not {(x, y)}")
    vol = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)
    if order == 0:
        zoomed = _zoom_gpu.zoom_nearest(vol, (Z0, Z1))
    else:
        zoomed = vol if (x, y) == (patch_size[0], patch_size[1]) else _zoom_gpu.zoom_cubic(vol, (Z0, Z1))
    prediction = torch.empty((S, x, y), dtype=torch.int64, device=vol.device)
    was_training = net.training
    net.eval()
    for s0 in range(0, S, batch):
        with _act_scope(act_dtype, logits="stored"):
            logits = net(zoomed[s0:s0 + batch].unsqueeze(1))[0]
        prediction[s0:s0 + batch] = _zoom_gpu.argmax_zoom_back(logits, (x, y))
    if was_training:
        net.train()
    return prediction


@torch.no_grad()
def test_single_volume(image, label, net, classes, patch_size=(256, 256), device="cuda:0", surface="host", zoom="host",
                       voxelspacing=None, connectivity=1, nms=0, cc="host", order=0, act_dtype="f32"):
    """test_2D.test_single_volume; with surface="gpu" the surface metrics of all classes come from one call on the label volumes that
    are on the device for the overlap counts already.  zoom="gpu" (with surface="gpu" only) is the device-resident case: the label map
    of predict_volume(zoom="gpu") goes to the overlap counts and the surface kernels as the device tensor it is.  Every class is scored on
    the [S, X, Y] volume as the 3-D object it is, so a voxelspacing has three entries.
    nms=1 keeps, before anything is counted or measured, only the largest component of every class of the [S, X, Y] prediction (the 3-D
    object it is, full connectivity): cc="host" (default) through cc_host.keep_largest_per_class on the host map, cc="gpu" (with
    surface="gpu" only) through cc_gpu.largest_per_class - with zoom="gpu" the label map then never leaves the device.
    order=3 is predict_volume's: the cubic-spline zoom of the slices to the patch on either route, everything after it unchanged.
    act_dtype="f16" is predict_volume's too: the forwards inside `ops.eval_half()`, everything around them unchanged."""
    _surface_gpu.check_route(surface)
    _zoom_gpu.check_order(order)
    check_act_dtype(act_dtype)
    if _zoom_gpu.check_zoom(zoom) == "gpu" and surface != "gpu":
        raise ValueError('zoom="gpu" is the device-resident head of surface="gpu"; got surface=%r' % (surface,))
    if _cc_gpu.check_cc(cc) == "gpu" and surface != "gpu":
        raise ValueError('cc="gpu" is the device-resident tail of surface="gpu"; got surface=%r' % (surface,))
    unit = _unit(voxelspacing, connectivity)
    if surface == "host" and unit and not nms and order == 0 and act_dtype == "f32":
        return _t2d.test_single_volume(image, label, net, classes, patch_size, device=device)
    if not unit:
        _surface_gpu.check_spaced_args(voxelspacing, connectivity, 3)
    if surface == "host":
        prediction = _predict_volume_host(image, net, patch_size, device=device, order=order, act_dtype=act_dtype)
        if nms:
            prediction = _cc_host.keep_largest_per_class(prediction)
        cnt = _t2d.overlap_counts(torch.from_numpy(prediction).to(device), torch.from_numpy(np.asarray(label, dtype=np.int64)).to(device),
                                  classes).cpu().numpy()
        return _metric_list(cnt, classes, lambda c: (_binary.hd95(prediction == c, label == c, voxelspacing, connectivity),
                                                     _binary.asd(prediction == c, label == c, voxelspacing, connectivity)))
    if zoom == "gpu":
        pred_d = predict_volume(image, net, patch_size, device=device, zoom="gpu", order=order, act_dtype=act_dtype)
        if nms and cc == "host":
            pred_d = torch.from_numpy(_cc_host.keep_largest_per_class(pred_d.cpu().numpy())).to(device)
    else:
        prediction = _predict_volume_host(image, net, patch_size, device=device, order=order, act_dtype=act_dtype)
        if nms and cc == "host":
            prediction = _cc_host.keep_largest_per_class(prediction)
        pred_d = torch.from_numpy(prediction).to(device)
    if nms and cc == "gpu":
        pred_d = _cc_gpu.largest_per_class(pred_d, classes)
    lab_d = torch.from_numpy(np.asarray(label, dtype=np.int64)).to(device)
    cnt = _t2d.overlap_counts(pred_d, lab_d, classes).cpu().numpy()
    scored = [] if classes <= 1 else _classes_device(pred_d, lab_d, range(1, classes), voxelspacing, connectivity)
    return _metric_list(cnt, classes, lambda c: scored[c - 1])


def calculate_metric_percase_3d(pred, gt, surface="host", voxelspacing=None, connectivity=1):
    """(dice, jc, hd95, asd) as test_util.calculate_metric_percase; with surface="gpu" both surface metrics from one kernel call."""
    unit = _unit(voxelspacing, connectivity)
    if _surface_gpu.check_route(surface) == "host" and unit:
        return _t3d.calculate_metric_percase(pred, gt)
    if not unit:
        _surface_gpu.check_spaced_args(voxelspacing, connectivity, len(_shape(pred)))
    if surface == "host":
        return (_binary.dc(pred, gt), _binary.jc(pred, gt), _binary.hd95(pred, gt, voxelspacing, connectivity),
                _binary.asd(pred, gt, voxelspacing, connectivity))
    return (_binary.dc(pred, gt), _binary.jc(pred, gt)) + _pair_device(pred, gt, voxelspacing, connectivity)


@torch.no_grad()
def predict_case(net, image, stride_xy, stride_z, patch_size, num_classes, batch=4, device="cuda:0", act_dtype="f32"):
    """The label map of test_util.test_single_case as an int64 tensor [w, h, d] that stays ON THE DEVICE: neither it nor the score map
    is copied to the host.  The window loop is test_single_case's, restated (that module stays as it is): the same padding, the same
    windows in the same order, the same arco_window_accumulate / arco_score_finalize launches and the same crop;
    tests/test_eval_cc_gpu.py holds the two to each other (array_equal, ragged and padded volumes).
    act_dtype="f16": every forward runs inside `ops.eval_half()` (the V-Net's f16 route); the logits leave as fp32 and the softmax and
    the window accumulation are the same launches."""
    check_act_dtype(act_dtype)
    image = np.asarray(image)
    w, h, d = image.shape
    pads = []
    for s, p in zip((w, h, d), patch_size):
        tot = max(p - s, 0)
        pads.append((tot // 2, tot - tot // 2))
    add_pad = any(a + b > 0 for a, b in pads)
    if add_pad:
        image = np.pad(image, pads, mode='constant', constant_values=0)
    ww, hh, dd = image.shape
    px, py, pz = (int(v) for v in patch_size)
    vol = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(device)
    C = int(num_classes)
    score = torch.zeros((C, ww, hh, dd), dtype=torch.float32, device=device)
    cnt = torch.zeros((ww, hh, dd), dtype=torch.float32, device=device)
    starts = [(xs, ys, zs) for xs in _t3d._window_starts(ww, px, stride_xy) for ys in _t3d._window_starts(hh, py, stride_xy)
              for zs in _t3d._window_starts(dd, pz, stride_z)]
    was_training = net.training
    net.eval()
    for s0 in range(0, len(starts), batch):
        grp = starts[s0:s0 + batch]
        patches = torch.stack([vol[xs:xs + px, ys:ys + py, zs:zs + pz] for xs, ys, zs in grp]).unsqueeze(1)
        with _act_scope(act_dtype):
            y1 = net(patches)
        if isinstance(y1, (tuple, list)):
            y1 = y1[0]
        assert int(y1.shape[1]) == C, (y1.shape, C)
        y = _glue.softmax(y1)                                    # [n, C, px, py, pz] planes
        for i, (xs, ys, zs) in enumerate(grp):
            _L.call("arco_window_accumulate", _L.ptr(y[i]), C, px, py, pz, _L.ptr(score), _L.ptr(cnt), ww, hh, dd, xs, ys, zs)
    if was_training:
        net.train()
    label = torch.empty((ww, hh, dd), dtype=torch.int64, device=device)
    _L.call("arco_score_finalize", _L.ptr(score), _L.ptr(cnt), C, ww * hh * dd, _L.ptr(label))
    if add_pad:
        (wl, _), (hl, _), (dl, _) = pads
        label = label[wl:wl + w, hl:hl + h, dl:dl + d].contiguous()
    return label


def _metric_percase_3d_device(pred, gt, voxelspacing=None, connectivity=1):
    """calculate_metric_percase_3d(surface="gpu") for two label tensors on the device; (0, 0, 0, 0) for an all-background prediction
    (test_util.py:57-58).  The host receives the overlap counts and the non-empty histogram bins, no volume.  (One mask `!= 0` serves
    both: labels are class indices >= 0, for which metrics.binary's `astype(bool)` and pair_metrics' `> 0` are the same.)"""
    p, g = (pred != 0).to(torch.int64), (gt != 0).to(torch.int64)
    n_pred, n_gt, n_both = _t2d.overlap_counts(p, g, 2)[1].cpu().tolist()
    if n_pred == 0:
        return (0, 0, 0, 0)
    dice = 2.0 * n_both / float(n_pred + n_gt)                                   # metrics.binary.dc / jc on the counts
    jc = float(n_both) / float(n_pred + n_gt - n_both)
    return (dice, jc) + _pair_device(p, g, voxelspacing, connectivity)


def test_all_case(model, cases, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4, preproc_fn=None,
                  metric_detail=0, nms=0, device="cuda:0", surface="host", cc="host", voxelspacing=None, connectivity=1,
                  nms_mode="foreground", act_dtype="f32"):
    """test_util.test_all_case: the mean (dice, jc, hd95, asd) over `cases` (an all-background prediction scores (0, 0, 0, 0)).
    cc="host" (default) takes the largest component of `nms` from test_util.getLargestCC on the host; cc="gpu" (with surface="gpu"
    only) is the device-resident tail: the label map of predict_case stays a device tensor, goes through cc_gpu.largest_cc with `nms`,
    and dice / jc / hd95 / asd come from the overlap-count and surface-distance kernels on it - no volume and no score map reach the
    host.  Like getLargestCC, cc_gpu.largest_cc takes every non-zero label as one foreground (skimage.measure.label, which the
    reference calls, joins only voxels of the same value): equal for the two-class case `nms` is used on, not for more classes.
    nms_mode (read only when `nms` is set) chooses what `nms` keeps: "foreground" (default) is that getLargestCC / largest_cc; "value" is
    the reference's own meaning, the largest component of equal values (cc_host.getLargestCC_by_value / cc_gpu.largest_cc_by_value);
    "per_class" keeps the largest component of every class (cc_host.keep_largest_per_class / cc_gpu.largest_per_class).
    act_dtype="f16": the forwards of every case run inside `ops.eval_half()` - predict_case's on cc="gpu", test_util.test_single_case's
    (that module stays as it is; the scope is entered around the call) otherwise."""
    _surface_gpu.check_route(surface)
    check_act_dtype(act_dtype)
    if _cc_gpu.check_cc(cc) == "gpu" and surface != "gpu":
        raise ValueError('cc="gpu" is the device-resident tail of surface="gpu"; got surface=%r' % (surface,))
    mode = _check_nms_mode(nms_mode) if nms else "foreground"
    unit = _unit(voxelspacing, connectivity)
    if surface == "host" and unit and mode == "foreground" and act_dtype == "f32":
        return _t3d.test_all_case(model, cases, num_classes, patch_size=patch_size, stride_xy=stride_xy, stride_z=stride_z,
                                  preproc_fn=preproc_fn, metric_detail=metric_detail, nms=nms, device=device)
    if not unit:
        _surface_gpu.check_spaced_args(voxelspacing, connectivity, 3)
    total, n = np.zeros(4), 0
    for ith, (image, label) in enumerate(cases):
        if preproc_fn is not None:
            image = preproc_fn(image)
        if cc == "gpu":
            prediction = predict_case(model, image, stride_xy, stride_z, patch_size, num_classes, device=device, act_dtype=act_dtype)
            if nms:
                prediction = _NMS[mode][1](prediction, num_classes)
            single = _metric_percase_3d_device(prediction, torch.from_numpy(np.asarray(label) != 0).to(prediction.device),
                                               voxelspacing, connectivity)
        else:
            with _act_scope(act_dtype):
                prediction, _ = _t3d.test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, device=device)
            if nms:
                prediction = _NMS[mode][0](prediction)
            single = ((0, 0, 0, 0) if np.sum(prediction) == 0 else
                      calculate_metric_percase_3d(prediction, np.asarray(label), surface, voxelspacing, connectivity))
        if metric_detail:
            print('%02d,\t%.5f, %.5f, %.5f, %.5f' % (ith, *single))
        total += np.asarray(single, dtype=np.float64)
        n += 1
    avg = total / max(n, 1)
    print('average metric is {}'.format(avg))
    return avg
