"""hd95 / asd on the GPU: the surface distances of utils/metrics.py (medpy.metric.binary restated) for unit voxel spacing and
connectivity 1 - the only way the reference calls them (test_2D.py:52-66, test_util.py:214-220) - as HIP kernels (csrc/surface.hip).

With unit spacing every squared surface distance is an integer, so the device returns a HISTOGRAM of squared distances
  hist[class][direction][k],  direction 0 = border(pred) -> border(gt), 1 = border(gt) -> border(pred),
  k = 0 .. (D-1)^2 + (H-1)^2 + (W-1)^2
computed in integer arithmetic (exact, independent of the order of arrival).  Only the non-empty bins travel to the host, which
finishes in float64 with numpy's own percentile:
  v = repeat(sqrt(k), count);  hd95 = percentile(v of both directions pooled, 95);  asd = mean(v of direction 0)
sqrt of the integer k is bit for bit what distance_transform_edt returns at that voxel, so hd95 equals the host route exactly and asd
up to the order of one float64 sum.  Anisotropic spacing breaks the integer histogram: a `voxelspacing` or a `connectivity` other
than 1 takes the float64 record route of the same file through the `spaced_*` functions at the end of this module, which return
one squared distance per border voxel; `pair_metrics` / `hd95` / `asd` stay the integer-exact unit-spacing route and refuse both."""
import numpy as np
import torch

from .. import _lib as L

MAX_DIM = 4096          # csrc/surface.hip SF_MAXDIM
MAX_CLASSES = 32        # csrc/surface.hip SF_MAXCLS
ROUTES = ("host", "gpu")

_EMPTY = ('The first supplied array does not contain any binary object.',
          'The second supplied array does not contain any binary object.')      # metrics.binary._surface_distances


def check_route(surface):
    """The `surface=` keyword of the evaluation entry points: "host" (utils/metrics.py, scipy) or "gpu" (this module)."""
    if surface not in ROUTES:
        raise ValueError(f"surface must be one of {ROUTES}, got {surface!r}")
    return surface


def nbins(shape):
    """Bins of one histogram row for a volume of `shape`: the largest squared distance plus one."""
    return int(sum((int(s) - 1) ** 2 for s in shape)) + 1


def _class_range(classes):
    cls = [int(c) for c in classes]
    if not cls or cls != list(range(cls[0], cls[0] + len(cls))):
        raise ValueError(f"classes must be a non-empty contiguous ascending range, got {list(classes)!r}")
    if len(cls) > MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} classes per call, got {len(cls)}")
    return cls[0], cls[-1]


def _map_ndim(shape, ndim):
    if len(shape) not in (2, 3):
        raise ValueError(f"label maps must be 2-D or 3-D, got shape {tuple(shape)}")
    ndim = len(shape) if ndim is None else int(ndim)
    if ndim not in (2, 3) or (ndim == 2 and len(shape) == 3 and shape[0] != 1):
        raise ValueError(f"ndim must be 2 or 3, and 2 only for a map [H, W] or [1, H, W]; got shape {tuple(shape)} and ndim {ndim}")
    if min(shape) < 1 or max(shape) > MAX_DIM:
        raise ValueError(f"every dim must be in 1..{MAX_DIM}, got {tuple(shape)}")
    return ndim


def _check_pair(who, pred, gt, ndim):
    """The checks of the two label tensors of a launch (`who` takes them, for the messages); the map's ndim."""
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)):
        raise TypeError(f"{who} torch tensors on the GPU")
    if pred.dtype.is_floating_point or gt.dtype.is_floating_point or pred.dtype == torch.bool or gt.dtype == torch.bool:
        raise TypeError(f"{who} integer label tensors")
    if pred.shape != gt.shape:
        raise ValueError(f"shapes differ: {tuple(pred.shape)} vs {tuple(gt.shape)}")
    return _map_ndim(tuple(pred.shape), ndim)


def _launch_pair(pred, gt):
    """(D, H, W, pred, gt) as a launch takes them: on the GPU, int64, contiguous."""
    L.require_gpu(pred, gt)
    D, H, W = (1, *pred.shape) if pred.dim() == 2 else pred.shape
    return D, H, W, pred.to(torch.int64).contiguous(), gt.to(torch.int64).contiguous()


def surface_histograms(pred, gt, classes, ndim=None):
    """int64 [len(classes), 2, nbins(shape)] on the device for two integer label tensors (2-D or 3-D, same shape, on the GPU).
    ndim (default: the tensors' rank) says how many axes have neighbours: a [1, H, W] tensor with ndim=2 is the 2-D map [H, W], and
    an [H, W] tensor with ndim=3 is the one-slice volume [1, H, W], whose every voxel is a border voxel (its z neighbours lie outside)."""
    c_lo, c_hi = _class_range(classes)
    ndim = _check_pair("surface_histograms takes", pred, gt, ndim)
    D, H, W, p, g = _launch_pair(pred, gt)
    nc, nb = c_hi - c_lo + 1, nbins(pred.shape)
    ws_bytes = L.query("arco_surface_ws_bytes", D, H, W, nc)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=p.device)
    hist = torch.empty((nc, 2, nb), dtype=torch.int64, device=p.device)
    with torch.cuda.device(p.device):
        L.call("arco_surface_hist", L.ptr(p), L.ptr(g), D, H, W, ndim, c_lo, c_hi, L.ptr(ws), ws_bytes, L.ptr(hist), hist.numel() * 8)
    return hist


def _distances(bins, counts):
    return np.repeat(np.sqrt(np.asarray(bins).astype(np.float64)), np.asarray(counts))


def finish_distances(d0, d1):
    """(hd95, asd) in float64 from the distances of the two directions; None when a direction is empty."""
    if d0.size == 0 or d1.size == 0:
        return None
    return float(np.percentile(np.hstack((d0, d1)), 95)), float(d0.mean())


def finish(bins0, counts0, bins1, counts1):
    """`finish_distances` from the non-empty bins of the two directions."""
    return finish_distances(_distances(bins0, counts0), _distances(bins1, counts1))


def finish_histogram(hist):
    """`finish` for one class's dense histogram [2, nbins] (a numpy array)."""
    hist = np.asarray(hist)
    b0, b1 = np.flatnonzero(hist[0]), np.flatnonzero(hist[1])
    return finish(b0, hist[0][b0], b1, hist[1][b1])


def surface_metrics(pred, gt, classes):
    """[(hd95, asd) or None] per class; None where the class has no voxel in pred or in gt (the host functions raise
    RuntimeError there and their callers guard for it)."""
    hist = surface_histograms(pred, gt, classes)
    nz = torch.nonzero(hist)                                            # [k, 3] = (class, direction, bin), row-major order
    rec = torch.cat((nz, hist[nz[:, 0], nz[:, 1], nz[:, 2]].unsqueeze(1)), dim=1).cpu().numpy()
    out = []
    for c in range(hist.shape[0]):
        r0 = rec[(rec[:, 0] == c) & (rec[:, 1] == 0)]
        r1 = rec[(rec[:, 0] == c) & (rec[:, 1] == 1)]
        out.append(finish(r0[:, 2], r0[:, 3], r1[:, 2], r1[:, 3]))
    return out


def _binary_args(voxelspacing, connectivity):
    if voxelspacing is not None:
        raise ValueError("the GPU surface metrics are for unit voxel spacing (voxelspacing=None); "
                         "use the host route arco_amd.utils.metrics.binary for a voxelspacing")
    if connectivity != 1:
        raise ValueError("the GPU surface metrics are for connectivity 1; use the host route arco_amd.utils.metrics.binary "
                         f"for connectivity {connectivity!r}")


def _mask(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x) > 0)      # (a fresh bool array: one byte per voxel to upload)
    if device is None:
        device = t.device if t.is_cuda else "cuda:0"
    return (t.to(device) > 0).to(torch.int64)


def _pair(metrics, result, reference, device, *args):
    """(hd95, asd) of one pair of binary masks from metrics(pred, gt, (1,), *args); metrics.binary's RuntimeError for an empty mask."""
    a = _mask(result, device)
    b = _mask(reference, a.device)
    got = metrics(a, b, (1,), *args)[0]
    if got is None:
        any_a, any_b = torch.stack((a.any(), b.any())).cpu().tolist()
        raise RuntimeError(_EMPTY[0] if not any_a else _EMPTY[1])
    return got


def pair_metrics(result, reference, voxelspacing=None, connectivity=1, device=None):
    """(hd95, asd) of one pair of binary masks (`> 0`; numpy or torch, 2-D or 3-D) from ONE histogram call.  Raises
    metrics.binary's RuntimeError when a mask is empty."""
    _binary_args(voxelspacing, connectivity)
    return _pair(surface_metrics, result, reference, device)


def hd95(result, reference, voxelspacing=None, connectivity=1, device=None):
    """metrics.binary.hd95 on the GPU."""
    return pair_metrics(result, reference, voxelspacing, connectivity, device)[0]


def asd(result, reference, voxelspacing=None, connectivity=1, device=None):
    """metrics.binary.asd on the GPU."""
    return pair_metrics(result, reference, voxelspacing, connectivity, device)[1]


# ---- a voxel spacing and a connectivity: float64 records instead of the integer histogram (arco_surface_sp_dist) --------------------------
def _spacing(voxelspacing, ndim):
    """medpy's voxelspacing for a map of `ndim` axes as a tuple of floats: None is 1.0, a scalar is broadcast, a sequence has one entry
    per axis."""
    if voxelspacing is None:
        return (1.0,) * ndim
    sp = np.asarray(voxelspacing, dtype=np.float64)
    if sp.ndim == 0:
        sp = np.full(ndim, float(sp))
    if sp.shape != (ndim,):
        raise ValueError(f"voxelspacing must be None, a number or {ndim} numbers (one per axis), got {voxelspacing!r}")
    if not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError(f"every voxelspacing must be finite and greater than 0, got {voxelspacing!r}")
    return tuple(float(v) for v in sp)


def _connectivity(connectivity, ndim):
    if not isinstance(connectivity, (int, np.integer)) or isinstance(connectivity, bool) or not 1 <= connectivity <= ndim:
        raise ValueError(f"connectivity must be an integer in 1..{ndim}, got {connectivity!r}")
    return int(connectivity)


def check_spaced_args(voxelspacing, connectivity, ndim):
    """ValueError for a voxelspacing or a connectivity that a map of `ndim` axes cannot take; (spacing per axis, connectivity)."""
    return _spacing(voxelspacing, ndim), _connectivity(connectivity, ndim)


def spaced_launch(pred, gt, classes, voxelspacing=None, connectivity=1, ndim=None, cap=None):
    """One arco_surface_sp_dist call for two integer label tensors on the GPU: (val float64 [cap], tag int32 [cap], count int64 [1]) ON
    THE DEVICE, not waited for.  Every argument check comes before any GPU work.  cap defaults to 2 * voxels, which cannot overflow."""
    c_lo, c_hi = _class_range(classes)
    ndim = _check_pair("the spaced surface functions take", pred, gt, ndim)
    sp = _spacing(voxelspacing, ndim)
    conn = _connectivity(connectivity, ndim)
    cap = 2 * pred.numel() if cap is None else int(cap)
    if cap < 1:
        raise ValueError(f"cap must be at least 1, got {cap}")
    D, H, W, p, g = _launch_pair(pred, gt)
    sz, sy, sx = (1.0, *sp) if ndim == 2 else sp
    ws_bytes = L.query("arco_surface_sp_ws_bytes", D, H, W, c_hi - c_lo + 1)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=p.device)
    val = torch.empty(cap, dtype=torch.float64, device=p.device)
    tag = torch.empty(cap, dtype=torch.int32, device=p.device)
    count = torch.empty(1, dtype=torch.int64, device=p.device)
    with torch.cuda.device(p.device):
        L.call("arco_surface_sp_dist", L.ptr(p), L.ptr(g), D, H, W, ndim, conn, sz, sy, sx, c_lo, c_hi, L.ptr(ws), ws_bytes,
               L.ptr(val), L.ptr(tag), cap, L.ptr(count))
    return val, tag, count


def spaced_records(pred, gt, classes, voxelspacing=None, connectivity=1, ndim=None, cap=None):
    """(val, tag): the records of spaced_launch on the host - float64 SQUARED distances in the order they arrived, and int32 tags
    (class index * 2 + direction).  Only the first `count` records travel.  RuntimeError when the kernels counted more records than
    the capacity `cap`."""
    val, tag, count = spaced_launch(pred, gt, classes, voxelspacing, connectivity, ndim, cap)
    n = int(count.item())
    if n > val.numel():
        raise RuntimeError(f"arco_amd: {n} surface records do not fit the capacity of {val.numel()}")
    return val[:n].cpu().numpy(), tag[:n].cpu().numpy()


def spaced_distances(pred, gt, classes, voxelspacing=None, connectivity=1, ndim=None):
    """[(d0, d1)] per class: two ascending float64 numpy arrays of surface distances, d0 from border(pred == c) to border(gt == c) and
    d1 the other way; both empty for a class absent from either map.  The squared records are sorted on the host - which makes the
    result independent of the order they arrived in - and np.sqrt is taken there."""
    classes = list(classes)
    val, tag = spaced_records(pred, gt, classes, voxelspacing, connectivity, ndim)
    return [tuple(np.sqrt(np.sort(val[tag == 2 * c + d])) for d in (0, 1)) for c in range(len(classes))]


def spaced_metrics(pred, gt, classes, voxelspacing=None, connectivity=1):
    """[(hd95, asd) or None] per class, as surface_metrics, with metrics.binary's voxelspacing and connectivity."""
    return [finish_distances(d0, d1) for d0, d1 in spaced_distances(pred, gt, classes, voxelspacing, connectivity)]


def spaced_pair_metrics(result, reference, voxelspacing=None, connectivity=1, device=None):
    """pair_metrics with a voxelspacing (None, a number, or one number per axis) and a connectivity (1..ndim): (hd95, asd) of one pair of
    binary masks from ONE call.  ValueError for a bad argument before any GPU work; metrics.binary's RuntimeError for an empty mask."""
    ndim = _map_ndim(tuple(result.shape if torch.is_tensor(result) else np.shape(result)), None)
    check_spaced_args(voxelspacing, connectivity, ndim)
    return _pair(spaced_metrics, result, reference, device, voxelspacing, connectivity)


def spaced_hd95(result, reference, voxelspacing=None, connectivity=1, device=None):
    """metrics.binary.hd95 with its voxelspacing and connectivity on the GPU."""
    return spaced_pair_metrics(result, reference, voxelspacing, connectivity, device)[0]


def spaced_asd(result, reference, voxelspacing=None, connectivity=1, device=None):
    """metrics.binary.asd with its voxelspacing and connectivity on the GPU."""
    return spaced_pair_metrics(result, reference, voxelspacing, connectivity, device)[1]
