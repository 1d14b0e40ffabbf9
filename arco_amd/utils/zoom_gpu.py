"""The zoom(order=0) round trip of 2-D evaluation on the GPU (csrc/zoom.hip): the device twin of the two scipy.ndimage.zoom calls
test_2D.predict_volume makes per slice (test_2D.py:72-88), so that a 2-D case can stay on the device from the upload of the volume to
the four metrics.

  zoom_nearest(x, out_size)           [S, n0, n1] float32 / int64 on the device -> [S, N0, N1] of the same dtype: what
                                      scipy.ndimage.zoom(x[s], (N0 / n0, N1 / n1), order=0) gives for every slice, bit for bit
  argmax_zoom_back(logits, out_size)  [n, C, P0, P1] logits on the device -> int64 [n, x, y]: zoom_nearest(glue.softmax_max(logits)[1],
                                      (x, y)) as one kernel that computes the softmax only of the pixels the zoom samples
  zoomed_size(n_in, target)           the length scipy gives the zoomed axis and its coordinate step (dataloaders.gpu_ingest's)

scipy's order-0 rule with mode 'constant': output index o reads input index floor(o * z + 0.5), z = (n_in - 1) / (n_out - 1) in
float64, and is 0 where o * z falls outside [0, n_in - 1] - for some sizes the last index lands one ulp above n_in - 1 and scipy zeroes
the whole last row or column.  The kernels reproduce that, edge cases included; `z` is computed here, in Python float64, by the same
division scipy makes."""
import torch

from .. import _lib as L
from .._contrast import rows_view
from ..dataloaders.gpu_ingest import zoomed_size  # noqa: F401  (part of this module's interface)

MAX_CLASSES = 32        # csrc/zoom.hip ZOOM_MAXC (glue.hip GL_MAXC)
ROUTES = ("host", "gpu")


def check_zoom(zoom):
    """The `zoom=` keyword of eval_surface.predict_volume / test_single_volume: "host" (scipy, test_2D.predict_volume) or "gpu" (this
    module)."""
    if zoom not in ROUTES:
        raise ValueError(f"zoom must be one of {ROUTES}, got {zoom!r}")
    return zoom


def _out_size(out_size):
    N0, N1 = (int(v) for v in out_size)
    if N0 < 2 or N1 < 2:
        raise ValueError(f"every output axis must have at least 2 points, got {(N0, N1)}")
    return N0, N1


def _step(n_in, n_out):
    return (n_in - 1) / (n_out - 1)


def zoom_nearest(x, out_size):
    """scipy.ndimage.zoom(order=0) of every slice of x [S, n0, n1] (float32 or int64, on the device) to out_size = (N0, N1)."""
    N0, N1 = _out_size(out_size)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise TypeError("zoom_nearest takes a torch tensor on the GPU")
    if x.dtype not in (torch.float32, torch.int64):
        raise TypeError(f"zoom_nearest takes float32 or int64, got {x.dtype}")
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"zoom_nearest takes a non-empty [S, n0, n1] tensor, got shape {tuple(x.shape)}")
    S, n0, n1 = (int(v) for v in x.shape)
    x = x.contiguous()
    out = torch.empty((S, N0, N1), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        L.call("arco_zoom_nearest2d", L.ptr(x), S, n0, n1, N0, N1, _step(n0, N0), _step(n1, N1), x.element_size(), L.ptr(out))
    return out


def argmax_zoom_back(logits, out_size):
    """int64 [n, x, y] on the device: argmax(softmax(logits, dim=1), dim=1) of [n, C, P0, P1] logits zoomed (order 0) to out_size =
    (x, y).  Any layout of the logits that _contrast.rows_view takes without a copy (channels-last, a channel slice of it) is read in
    place."""
    N0, N1 = _out_size(out_size)
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise TypeError("argmax_zoom_back takes a torch tensor on the GPU")
    if logits.dim() != 4 or min(logits.shape) < 1:
        raise ValueError(f"argmax_zoom_back takes non-empty [n, C, P0, P1] logits, got shape {tuple(logits.shape)}")
    n, C, P0, P1 = (int(v) for v in logits.shape)
    if C > MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} classes, got {C}")
    r, ld = rows_view(logits.detach())
    if r.dtype != torch.float32:
        r, ld = r.float().contiguous(), C
    out = torch.empty((n, N0, N1), dtype=torch.int64, device=logits.device)
    with torch.cuda.device(logits.device):
        L.call("arco_argmax_zoom_back2d", L.ptr(r), ld, C, n, P0, P1, N0, N1, _step(P0, N0), _step(P1, N1), L.ptr(out))
    return out
