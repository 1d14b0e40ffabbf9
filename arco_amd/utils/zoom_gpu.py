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
division scipy makes.

zoom(order=3), which the reference's test.py:124 applies to the image slices (only the arg-max map goes back by order 0):
  spline_prefilter(x)                 [S, n0, n1] float32 on the device -> float64 cubic B-spline coefficients [S, n0, n1]: scipy's
                                      prefilter with the mirror boundary it uses for mode 'constant', axis 0 then axis 1
  zoom_cubic(x, out_size)             [S, n0, n1] float32 on the device -> float32 [S, N0, N1]: scipy.ndimage.zoom(x[s], (N0 / n0,
                                      N1 / n1), order=3) of every slice - the prefilter, then the 4 x 4-tap interpolation in float64 at
                                      the same sample positions, with the same zeroed last row or column as order 0
  check_order(order)                  the `order=` keyword of the evaluation entry points: 0 or 3
  spline_constants(n0, n1)            the doubles the prefilter kernels are handed: (z, gain, z^(n0 - 1), z^(n1 - 1))
Both are held bit for bit to the float64 restatement of tests/zoom_cubic_kernel_refs.py, which tests/test_zoom_cubic_kernels_cpu.py
holds to scipy: float32 results equal but for a rounding tie about once in 1e8 outputs.  The pole, the gain and the powers of the pole
are computed here in Python float64, by the expressions of that restatement; the kernels take no power themselves."""
import math

import torch

from .. import _lib as L
from .._contrast import rows_view
from ..dataloaders.gpu_ingest import zoomed_size  # noqa: F401  (part of this module's interface)

MAX_CLASSES = 32        # csrc/zoom.hip ZOOM_MAXC (glue.hip GL_MAXC)
ROUTES = ("host", "gpu")
ORDERS = (0, 3)
SPLINE_POLE = math.sqrt(3.0) - 2.0                                  # the pole of the cubic B-spline prefilter
SPLINE_GAIN = (1.0 - SPLINE_POLE) * (1.0 - 1.0 / SPLINE_POLE)


def check_zoom(zoom):
    """The `zoom=` keyword of eval_surface.predict_volume / test_single_volume: "host" (scipy, test_2D.predict_volume) or "gpu" (this
    module)."""
    if zoom not in ROUTES:
        raise ValueError(f"zoom must be one of {ROUTES}, got {zoom!r}")
    return zoom


def check_order(order):
    """The `order=` keyword of eval_surface.predict_volume / test_single_volume: 0 (nearest, the default) or 3 (cubic spline) for the
    zoom of the image slices to the patch; the arg-max map always goes back by order 0."""
    if isinstance(order, bool) or order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    return int(order)


def spline_constants(n0, n1):
    """(z, gain, z^(n0 - 1), z^(n1 - 1)) in Python float64, as arco_spline_prefilter2d takes them."""
    return SPLINE_POLE, SPLINE_GAIN, SPLINE_POLE ** (n0 - 1), SPLINE_POLE ** (n1 - 1)


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
    place.  float16 logits (the stored logits of `ops.eval_half(logits="stored")`) go to arco_argmax_zoom_back2d_h, which widens each
    sampled row in registers: the labels of the fp32 cast of the same logits, without the cast pass."""
    N0, N1 = _out_size(out_size)
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise TypeError("argmax_zoom_back takes a torch tensor on the GPU")
    if logits.dim() != 4 or min(logits.shape) < 1:
        raise ValueError(f"argmax_zoom_back takes non-empty [n, C, P0, P1] logits, got shape {tuple(logits.shape)}")
    n, C, P0, P1 = (int(v) for v in logits.shape)
    if C > MAX_CLASSES:
        raise ValueError(f"at most {MAX_CLASSES} classes, got {C}")
    r, ld = rows_view(logits.detach())                       # float32 or float16 rows (any other dtype arrives as float32)
    entry = L.h("arco_argmax_zoom_back2d", r)     # f16 rows are read as stored
    out = torch.empty((n, N0, N1), dtype=torch.int64, device=logits.device)
    with torch.cuda.device(logits.device):
        L.call(entry, L.ptr(r), ld, C, n, P0, P1, N0, N1, _step(P0, N0), _step(P1, N1), L.ptr(out))
    return out


def _cubic_input(x, name):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise TypeError(f"{name} takes a torch tensor on the GPU")
    if x.dtype != torch.float32:
        raise TypeError(f"{name} takes float32, got {x.dtype}")
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{name} takes a non-empty [S, n0, n1] tensor, got shape {tuple(x.shape)}")
    S, n0, n1 = (int(v) for v in x.shape)
    if n0 < 2 or n1 < 2:
        raise ValueError(f"{name}: every input axis must have at least 2 points, got slices of {(n0, n1)}")
    return S, n0, n1


def _prefilter(x, S, n0, n1):
    coef = torch.empty((S, n0, n1), dtype=torch.float64, device=x.device)
    L.call("arco_spline_prefilter2d", L.ptr(x), S, n0, n1, *spline_constants(n0, n1), 3, L.ptr(coef))
    return coef


def spline_prefilter(x):
    """float64 cubic B-spline coefficients [S, n0, n1] of the float32 slices x [S, n0, n1] on the device: what
    scipy.ndimage.spline_filter(x[s], order=3, output=float64, mode='constant') computes (equal to a few ulp; bit for bit the
    restatement of tests/zoom_cubic_kernel_refs.py)."""
    S, n0, n1 = _cubic_input(x, "spline_prefilter")
    with torch.cuda.device(x.device):
        return _prefilter(x.contiguous(), S, n0, n1)


def zoom_cubic(x, out_size):
    """scipy.ndimage.zoom(order=3) of every slice of x [S, n0, n1] (float32, on the device) to out_size = (N0, N1): float32."""
    N0, N1 = _out_size(out_size)
    S, n0, n1 = _cubic_input(x, "zoom_cubic")
    x = x.contiguous()
    out = torch.empty((S, N0, N1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        coef = _prefilter(x, S, n0, n1)
        L.call("arco_zoom_cubic2d", L.ptr(coef), S, n0, n1, N0, N1, _step(n0, N0), _step(n1, N1), L.ptr(out))
    return out
