"""Cases, references and checkers for the surface-distance kernels with a voxel spacing and a connectivity
(arco_amd/csrc/surface.hip, the spaced_* functions of arco_amd/utils/surface_gpu.py).

The kernels return one record per border voxel of A with a border voxel of B to measure to: val = the float64 SQUARED distance,
tag = class index * 2 + direction (direction 0: A = pred == c, B = gt == c; 1 the other way round).  With
  w_a(e) = fl(fl(s_a * e) * fl(s_a * e))
the kernels' value is, bit for bit, the minimum over the border voxels of B of fl(fl(w_x(dx) + w_y(dy)) + w_z(dz)) (2-D: fl(w_x + w_y)):
float64 addition is monotone, so the separable minimum of the three passes equals the minimum of the sums.  Two references:
  brute_records    an O(n^2) numpy restatement in exactly that operation order (numpy rounds every elementwise operation once and
                   fuses nothing), with an O(n^2) border that shares no code with scipy.ndimage - the EXACT reference;
  scipy_distances  metrics.binary._surface_distances (binary_erosion, distance_transform_edt(sampling=)), which forms the same three
                   products but adds them z, y, x: equal up to the last bits, held to REL_SCIPY below.

REL_SCIPY = 4 * 2^-52 relative on the distance: each side makes two roundings in its sum of three exactly-equal weights (relative
2^-53 each, all terms >= 0, so the two squared values differ by at most 4 * 2^-53 = 2 * 2^-52 relative); the square root halves a
relative difference (1 * 2^-52) and rounds once on either side (2 * 2^-53 = 1 * 2^-52 more): 2 * 2^-52, doubled for slack = 4 * 2^-52.
(Measured: 0.83 * 2^-52.)

Shapes: those of tests/surface_kernel_refs.py that sit at an edge of a pass.  The float64 min-plus pass stages its line in an LDS tile of
128 entries, so the lines of 300 take three chunks; a row of 130 is two ballot words plus a ragged third; 70 and 67 are lines longer
than one wave along H and along D.  Two planted cases: `nearest_by_index`, where the voxel nearest by index is not the nearest in
millimetres, and `diagonal_holes`, two holes joined only diagonally inside a filled block, whose border grows with the connectivity."""
import functools
import itertools

import numpy as np
import torch

import surface_kernel_refs as R
from arco_amd.utils import metrics

GUARD, SENT32, SENT64 = R.GUARD, R.SENT32, R.SENT64
BRUTE_MAX_VOXELS = R.BRUTE_MAX_VOXELS       # the brute force builds an |border A| x |border B| table; both are within the volume
REL_SCIPY = 4 * 2.0 ** -52
TILE = 128                                   # csrc/surface.hip: the float64 tile of sf_minplus_kernel

SPACINGS = {
    "10_1.25_1.25": (10.0, 1.25, 1.25),      # ACDC
    "2.9_0.7_1.3": (2.9, 0.7, 1.3),
    "third_0.1_7.7": (1.0 / 3.0, 0.1, 7.7),
    "scalar_2": 2.0,
    "unit": (1.0, 1.0, 1.0),
}


def spacing_for(key, ndim):
    """The voxelspacing argument for a map of ndim axes: a 2-D map takes the first two entries (anisotropic in every triple above)."""
    sp = SPACINGS[key]
    return sp if np.isscalar(sp) else tuple(sp[:ndim])


def per_axis(voxelspacing, ndim):
    return (float(voxelspacing),) * ndim if np.isscalar(voxelspacing) else tuple(float(v) for v in voxelspacing)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def _nearest_by_index():
    pred, gt = np.zeros((3, 3, 5), dtype=np.int64), np.zeros((3, 3, 5), dtype=np.int64)
    pred[0, 0, 0] = 1
    gt[1, 0, 0] = 1                          # one voxel away along z: 10 mm with spacing (10, 1, 1)
    gt[0, 0, 3] = 1                          # three voxels away along x: 3 mm
    return dict(pred=pred, gt=gt, classes=[1], empty=[])


def _diagonal_holes():
    pred, gt = np.zeros((7, 7, 7), dtype=np.int64), np.zeros((7, 7, 7), dtype=np.int64)
    pred[1:6, 1:6, 1:6] = 1
    pred[2, 2, 3] = pred[3, 3, 3] = 0        # two holes that touch only across an edge
    gt[1:5, 2:6, 1:6] = 1
    gt[3, 3, 3] = 0
    return dict(pred=pred, gt=gt, classes=[1], empty=[])


_SHARED = ["2d_24x20", "2d_1x7", "3d_14x12x10", "3d_3x5x130", "3d_5x70x9", "3d_67x4x6", "3d_2x300x3", "3d_300x3x2", "3d_full",
           "3d_absent", "3d_from_class_2"]
_PLANTED = {"nearest_by_index": _nearest_by_index, "diagonal_holes": _diagonal_holes}
CASES = _SHARED + list(_PLANTED)


@functools.lru_cache(maxsize=None)
def case(name):
    """pred, gt (read-only), classes, empty, shape, ndim."""
    if name in _PLANTED:
        c = _PLANTED[name]()
        c["name"], c["shape"], c["ndim"] = name, c["pred"].shape, c["pred"].ndim
        for a in (c["pred"], c["gt"]):
            a.setflags(write=False)
        return c
    return R.case(name)


def combos():
    """Every (case, spacing key, connectivity 1..ndim)."""
    return [(n, s, k) for n in CASES for s in SPACINGS for k in range(1, (2 if n.startswith("2d") else 3) + 1)]


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def offsets(ndim, connectivity):
    """The neighbour offsets in {-1, 0, 1}^ndim with 1 to `connectivity` non-zero components."""
    return [o for o in itertools.product((-1, 0, 1), repeat=ndim) if 1 <= sum(v != 0 for v in o) <= connectivity]


def brute_border(x, connectivity):
    """x[v] and one neighbour unset; outside the array counts as unset.  Voxel by voxel."""
    out = np.zeros_like(x)
    for v in np.argwhere(x):
        for o in offsets(x.ndim, connectivity):
            u = v + o
            if (u < 0).any() or (u >= x.shape).any() or not x[tuple(u)]:
                out[tuple(v)] = True
                break
    return out


@functools.lru_cache(maxsize=None)
def border_points(name, which, k, connectivity):
    """Coordinates [n, ndim] int64 of brute_border(case(name)[which] == k) (computed once; read-only)."""
    pts = np.argwhere(brute_border(case(name)[which] == k, connectivity)).astype(np.int64)
    pts.setflags(write=False)
    return pts


def _brute_d2(pa, pb, sp):
    """For each row of pa the minimum over the rows of pb of fl(fl(w_x + w_y) + w_z) (2-D: fl(w_x + w_y)); one rounding per operation."""
    e = (pa[:, None, :] - pb[None, :, :]).astype(np.float64)           # exact small integers
    w = []
    for ax in range(pa.shape[1]):
        t = np.float64(sp[ax]) * e[:, :, ax]
        w.append(t * t)
    s = w[-1] + w[-2]                                                  # x, then y
    if len(w) == 3:
        s = s + w[0]                                                   # then z
    return s.min(axis=1)


@functools.lru_cache(maxsize=None)
def brute_records(name, spacing_key, connectivity):
    """{(class index, direction): ascending float64 squared distances} for a case of this module (computed once; read-only)."""
    c = case(name)
    assert int(np.prod(c["shape"])) <= BRUTE_MAX_VOXELS
    sp = per_axis(spacing_for(spacing_key, c["ndim"]), c["ndim"])
    out = {}
    for i, k in enumerate(c["classes"]):
        pa, pb = border_points(name, "pred", k, connectivity), border_points(name, "gt", k, connectivity)
        both = len(pa) > 0 and len(pb) > 0
        out[(i, 0)] = np.sort(_brute_d2(pa, pb, sp)) if both else np.zeros(0)
        out[(i, 1)] = np.sort(_brute_d2(pb, pa, sp)) if both else np.zeros(0)
        for a in (out[(i, 0)], out[(i, 1)]):
            a.setflags(write=False)
    return out


def scipy_distances(a, b, voxelspacing, connectivity):
    """(ascending distances a -> b, b -> a) from metrics.binary._surface_distances; two empty arrays when a mask is empty."""
    if not (a.any() and b.any()):
        return np.zeros(0), np.zeros(0)
    return (np.sort(metrics.binary._surface_distances(a, b, voxelspacing, connectivity)),
            np.sort(metrics.binary._surface_distances(b, a, voxelspacing, connectivity)))


# ---- checkers -----------------------------------------------------------------------------------------------------------------------------
def group(val, tag, n_classes):
    """The records of one call as {(class index, direction): ascending float64 array}."""
    val = val.cpu().numpy() if torch.is_tensor(val) else np.asarray(val)
    tag = tag.cpu().numpy() if torch.is_tensor(tag) else np.asarray(tag)
    assert val.dtype == np.float64 and val.shape == tag.shape
    assert ((tag >= 0) & (tag < 2 * n_classes)).all()
    return {(i, d): np.sort(val[tag == 2 * i + d]) for i in range(n_classes) for d in (0, 1)}


def exact(got, ref):
    """Every group array_equal as float64: the same number of records and the same bits."""
    if set(got) != set(ref):
        return False
    return all(got[k].dtype == np.float64 and got[k].shape == ref[k].shape and bool(np.array_equal(got[k], ref[k])) for k in ref)


def within(got, ref, rel):
    """Ascending arrays of equal length, elementwise within `rel` relative of ref."""
    return got.shape == ref.shape and bool((np.abs(got - ref) <= rel * np.abs(ref)).all())


guarded, guards_intact = R.guarded, R.guards_intact


def run_guarded(L, name, spacing_key, connectivity, cap=None):
    """The entry point itself on exactly-sized buffers (cap defaults to the reference's number of records) with sentinels behind val,
    tag, count and the workspace: (count, val [min(count, cap)] float64, tag, the four whole buffers with their sizes)."""
    c = case(name)
    ndim = c["ndim"]
    D, H, W = (1, *c["shape"]) if ndim == 2 else c["shape"]
    sz, sy, sx = (1.0,) * (3 - ndim) + per_axis(spacing_for(spacing_key, ndim), ndim)
    nc = len(c["classes"])
    if cap is None:
        cap = max(sum(v.size for v in brute_records(name, spacing_key, connectivity).values()), 1)
    ws_bytes = L.query("arco_surface_sp_ws_bytes", D, H, W, nc)
    assert ws_bytes == nc * 2 * 2 * D * H * W * 8
    ws, val = guarded(ws_bytes // 8, torch.int64).cuda(), guarded(cap, torch.int64).cuda()
    tag, count = guarded(cap, torch.int32).cuda(), guarded(1, torch.int64).cuda()
    p, g = torch.tensor(c["pred"]).cuda(), torch.tensor(c["gt"]).cuda()
    L.call("arco_surface_sp_dist", L.ptr(p), L.ptr(g), D, H, W, ndim, connectivity, sz, sy, sx, c["classes"][0], c["classes"][-1],
           L.ptr(ws), ws_bytes, L.ptr(val), L.ptr(tag), cap, L.ptr(count))
    torch.cuda.synchronize()
    n = int(count[0].item())
    k = min(n, cap)
    bufs = ((ws.cpu(), ws_bytes // 8), (val.cpu(), cap), (tag.cpu(), cap), (count.cpu(), 1))
    return n, val[:k].view(torch.float64).cpu().numpy(), tag[:k].cpu().numpy(), bufs
