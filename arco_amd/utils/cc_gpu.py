"""Connected components and the largest one on the GPU (csrc/cc.hip): the device twin of test_util.getLargestCC, the reference's
`nms` post-processing (test_util.py:11-15), so that a label map can stay on the device from the arg-max to the metrics.

  components(x, connectivity, ndim) -> (labels, largest, info), all on the device and in the shape of x
    labels   int32: 0 on background (x == 0), else 1 + the smallest linear index of the voxel's component
    largest  uint8: 1 on the component with the most voxels; of several that large, the one whose first voxel comes first in memory
    info     int64 [3] = {components, linear index of the winner's first voxel, its voxel count}; {0, -1, 0} without foreground
  largest_cc(x) -> bool tensor on the device, getLargestCC's result (full connectivity).
Neighbours differ by +-1 in at most `connectivity` axes: scipy's generate_binary_structure(ndim, connectivity).  The tie rule is that of
getLargestCC's `labels == argmax(bincount(labels)[1:]) + 1` on scipy's raster-order numbering.  Everything is integer and independent of
the order of arrival, so two runs give identical tensors.

Like getLargestCC - and unlike skimage.measure.label, which the reference calls and which joins only voxels of the SAME value - every
non-zero label is one foreground.  The two agree on the binary maps the reference uses `nms` on and would differ for more than two
classes; the host function stays as it is and this route is pinned to it.

The BY-VALUE meaning (the ccv_* kernels of csrc/cc.hip) stands beside it, for label maps of `classes` classes (2..256): a voxel is in range when
1 <= x <= classes - 1, and two in-range voxels are connected only when they are neighbours AND have equal values.
  components_by_value(x, classes, connectivity, ndim) -> (labels, keep, info), all on the device
    labels   int32: 0 on background (anything not in range), else 1 + the smallest linear index of the voxel's component
    keep     uint8: 1 where the voxel lies in the largest component of ITS OWN class (ties: the first in memory)
    info     int64 [classes + 1, 3]: rows 1..classes-1 {components, winner's first index, its voxels} per class ({0, -1, 0} when absent),
             row 0 the same over all classes together, row `classes` {voxels outside 0..classes-1, the first one's index or -1, 0}
  largest_per_class(x, classes) -> int64 tensor: x where keep, 0 elsewhere (cc_host.keep_largest_per_class)
  largest_cc_by_value(x, classes) -> bool tensor: the one component of info[0] (cc_host.getLargestCC_by_value: what the reference's
    getLargestCC computes through skimage; not pinned to skimage itself, which is not a dependency)"""
import numpy as np
import torch

from .. import _lib as L

MAX_DIM = 4096          # csrc/cc.hip CC_MAXDIM
MAX_VOXELS = 1 << 31    # exclusive: linear indices are int32
MAX_CLASSES = 256       # csrc/cc.hip CCV_MAXCLASSES: classes are kept as bytes
ROUTES = ("host", "gpu")


def check_cc(cc):
    """The `cc=` keyword of eval_surface.test_all_case: "host" (test_util.getLargestCC, scipy) or "gpu" (this module)."""
    if cc not in ROUTES:
        raise ValueError(f"cc must be one of {ROUTES}, got {cc!r}")
    return cc


def _check_classes(classes):
    if isinstance(classes, bool) or not isinstance(classes, (int, np.integer)):
        raise TypeError(f"classes must be an int, got {classes!r}")
    if not 2 <= classes <= MAX_CLASSES:
        raise ValueError(f"classes must be in 2..{MAX_CLASSES}, got {classes}")
    return int(classes)


def _check_map(name, x, connectivity, ndim, *classes):
    """The argument checks of `components` and `components_by_value` (`name`; the latter passes its `classes`, checked in their
    place), all before any GPU work; (D, H, W, ndim, connectivity) with the defaults filled in."""
    if not torch.is_tensor(x):
        raise TypeError(f"{name} takes a torch tensor on the GPU")
    if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
        raise TypeError(f"{name} takes an integer label tensor")
    for c in classes:
        _check_classes(c)
    if x.dim() not in (2, 3):
        raise ValueError(f"the label map must be 2-D or 3-D, got shape {tuple(x.shape)}")
    ndim = x.dim() if ndim is None else int(ndim)
    if ndim not in (2, 3) or (ndim == 2 and x.dim() == 3 and x.shape[0] != 1):
        raise ValueError(f"ndim must be 2 or 3, and 2 only for a map [H, W] or [1, H, W]; got shape {tuple(x.shape)} and ndim {ndim}")
    connectivity = ndim if connectivity is None else int(connectivity)
    if not 1 <= connectivity <= ndim:
        raise ValueError(f"connectivity must be in 1..{ndim}, got {connectivity}")
    if min(x.shape) < 1 or max(x.shape) > MAX_DIM:
        raise ValueError(f"every dim must be in 1..{MAX_DIM}, got {tuple(x.shape)}")
    if x.numel() >= MAX_VOXELS:
        raise ValueError(f"at most 2^31 - 1 voxels, got shape {tuple(x.shape)}")
    L.require_gpu(x)
    D, H, W = (1, *x.shape) if x.dim() == 2 else x.shape
    return D, H, W, ndim, connectivity


def _to_device(t, device):
    """The tensor on `device`; by default where it is when that is a GPU, else on cuda:0."""
    if device is None:
        device = t.device if t.is_cuda else "cuda:0"
    return t.to(device)


def components(x, connectivity=None, ndim=None):
    """(labels int32, largest uint8, info int64 [3]) on the device for one integer label tensor (2-D or 3-D, on the GPU).
    ndim (default: the tensor's rank) says how many axes there are: a [1, H, W] tensor with ndim=2 is the map [H, W], an [H, W] tensor
    with ndim=3 the one-slice volume [1, H, W].  connectivity in 1..ndim (default ndim: 8 neighbours in 2-D, 26 in 3-D)."""
    D, H, W, ndim, connectivity = _check_map("components", x, connectivity, ndim)
    v = x.to(torch.int64).contiguous()
    ws_bytes = L.query("arco_cc_ws_bytes", D, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=v.device)
    labels = torch.empty(x.shape, dtype=torch.int32, device=v.device)
    largest = torch.empty(x.shape, dtype=torch.uint8, device=v.device)
    info = torch.empty(3, dtype=torch.int64, device=v.device)
    with torch.cuda.device(v.device):
        L.call("arco_cc_largest", L.ptr(v), D, H, W, ndim, connectivity, L.ptr(ws), ws_bytes, L.ptr(labels), labels.numel() * 4,
               L.ptr(largest), largest.numel(), L.ptr(info), 24)
    return labels, largest, info


def largest_cc(x, device=None):
    """test_util.getLargestCC on the GPU: the largest component (full connectivity) of `x != 0` (numpy or torch, 2-D or 3-D) as a bool
    tensor on the device.  AssertionError when there is no foreground, as the host function."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x) != 0)          # (a fresh bool array: one byte per voxel to upload)
    t = _to_device(t, device)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        t = (t != 0).to(torch.uint8)
    _, largest, info = components(t)
    assert int(info[0]) != 0                       # assume at least 1 CC
    return largest.bool()


def components_by_value(x, classes, connectivity=None, ndim=None):
    """(labels int32, keep uint8, info int64 [classes + 1, 3]) on the device for one integer label tensor (2-D or 3-D, on the GPU): the
    components of equal values and the largest one of every class (module docstring).  The tensor, ndim, connectivity and size rules are
    those of `components`; classes in 2..256.  Nothing is synchronised."""
    D, H, W, ndim, connectivity = _check_map("components_by_value", x, connectivity, ndim, classes)
    classes = int(classes)
    v = x.to(torch.int64).contiguous()
    ws_bytes = L.query("arco_cc_value_ws_bytes", D, H, W, classes)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=v.device)
    labels = torch.empty(x.shape, dtype=torch.int32, device=v.device)
    keep = torch.empty(x.shape, dtype=torch.uint8, device=v.device)
    info = torch.empty((classes + 1, 3), dtype=torch.int64, device=v.device)
    with torch.cuda.device(v.device):
        L.call("arco_cc_value_largest", L.ptr(v), D, H, W, ndim, connectivity, classes, L.ptr(ws), ws_bytes, L.ptr(labels),
               labels.numel() * 4, L.ptr(keep), keep.numel(), L.ptr(info), info.numel() * 8)
    return labels, keep, info


def _label_tensor(x, device):
    """A numpy array or tensor of labels as an integer tensor on the device (bool: 0 / 1)."""
    if not torch.is_tensor(x):
        x = np.ascontiguousarray(x)
        x = torch.from_numpy(x if x.flags.writeable else x.copy())                 # (torch takes no read-only arrays)
    t = x
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError("a label map by value must be of an integer (or bool) type")
    if t.dim() not in (2, 3):
        raise ValueError(f"the label map must be 2-D or 3-D, got shape {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return _to_device(t, device)


def _refuse_out_of_range(t, classes, info):
    n, first, _ = info[classes].tolist()
    if n:
        raise ValueError(f"{n} labels outside 0..{classes - 1}; the first is {int(t.reshape(-1)[first])} at linear index {first}")


def largest_per_class(x, classes, device=None):
    """cc_host.keep_largest_per_class on the GPU: the label map `x` (numpy or torch, 2-D or 3-D, labels 0..classes-1) with all but the
    largest component (full connectivity, equal values) of every class zeroed, as an int64 tensor on the device.  ValueError naming the
    first offending linear index when a label lies outside 0..classes-1."""
    classes = _check_classes(classes)
    t = _label_tensor(x, device)
    _, keep, info = components_by_value(t, classes)
    _refuse_out_of_range(t, classes, info)
    t = t.to(torch.int64)
    return torch.where(keep.bool(), t, torch.zeros_like(t))


def largest_cc_by_value(x, classes, device=None):
    """cc_host.getLargestCC_by_value on the GPU - the reference's getLargestCC as skimage.measure.label means it: the one component of
    equal values (full connectivity) with the most voxels over all classes, as a bool tensor on the device.  AssertionError when there is
    no foreground, as the host function; ValueError when a label lies outside 0..classes-1."""
    classes = _check_classes(classes)
    t = _label_tensor(x, device)
    labels, _, info = components_by_value(t, classes)
    _refuse_out_of_range(t, classes, info)
    n, first, _ = info[0].tolist()
    assert n != 0                                  # assume at least 1 CC
    return labels == first + 1
