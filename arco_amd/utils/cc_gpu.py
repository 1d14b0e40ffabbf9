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
classes; the host function stays as it is and this route is pinned to it."""
import numpy as np
import torch

from .. import _lib as L

MAX_DIM = 4096          # csrc/cc.hip CC_MAXDIM
MAX_VOXELS = 1 << 31    # exclusive: linear indices are int32
ROUTES = ("host", "gpu")


def check_cc(cc):
    """The `cc=` keyword of eval_surface.test_all_case: "host" (test_util.getLargestCC, scipy) or "gpu" (this module)."""
    if cc not in ROUTES:
        raise ValueError(f"cc must be one of {ROUTES}, got {cc!r}")
    return cc


def components(x, connectivity=None, ndim=None):
    """(labels int32, largest uint8, info int64 [3]) on the device for one integer label tensor (2-D or 3-D, on the GPU).
    ndim (default: the tensor's rank) says how many axes there are: a [1, H, W] tensor with ndim=2 is the map [H, W], an [H, W] tensor
    with ndim=3 the one-slice volume [1, H, W].  connectivity in 1..ndim (default ndim: 8 neighbours in 2-D, 26 in 3-D)."""
    if not torch.is_tensor(x):
        raise TypeError("components takes a torch tensor on the GPU")
    if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
        raise TypeError("components takes an integer label tensor")
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
    if device is None:
        device = t.device if t.is_cuda else "cuda:0"
    t = t.to(device)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        t = (t != 0).to(torch.uint8)
    _, largest, info = components(t)
    assert int(info[0]) != 0                       # assume at least 1 CC
    return largest.bool()
