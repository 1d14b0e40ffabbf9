"""Cases, references and checkers for the connected-components-by-value kernels (arco_amd/csrc/cc.hip, arco_amd/utils/cc_gpu.py).

The kernels return, for an integer label volume, a class count C (2..256) and a connectivity c in 1..ndim (scipy's
generate_binary_structure(ndim, c)) - a voxel is IN RANGE when 1 <= x <= C - 1, two in-range voxels are connected when they are
neighbours AND have equal values:
  labels   int32, 0 on background (anything not in range), else 1 + the smallest flat index of the voxel's component
  keep     uint8, 1 where the voxel lies in the component of ITS OWN class with the most voxels (ties: the first in memory)
  info     int64 [C + 1, 3]: rows 1..C-1 {components of the class, flat index of the winner's first voxel, its voxel count}, {0, -1, 0}
           for an absent class; row 0 the same over all classes together; row C {voxels outside 0..C-1, the first one's index or -1, 0}
Two references that share no code:
  scipy_ref   scipy.ndimage.label once per class; canonical labels and winners by bincount
  flood_ref   a breadth-first flood fill in raster order in plain Python that compares values, for cases of up to FLOOD_MAX_VOXELS voxels
Everything is an integer, so the only check is equality.

A case is an array, the `ndim` it is run with and its class count.  Each case sits at an edge of one pass of the kernels: a row is
balloted into 64-bit words of in-range bits and of run-start bits (widths 1, 63, 64, 65, 130; value changes inside the words and at
columns 62|63, 63|64, 64|65), a run piece ends at a value change as well as at background, a merge compares values (stacked rows and
planes, checkerboards and nests of different values must stay apart), winners are chosen per class (ties, absent classes, values out
of range).  The volume builders and the buffer guards are those of tests/cc_kernel_refs.py."""
import functools
import itertools

import numpy as np
import torch

import cc_kernel_refs as B
from cc_kernel_refs import GUARD, SENT, guarded, guards_intact, same, untouched, _as_ndim          # noqa: F401

FLOOD_MAX_VOXELS = 4000


# ---- volumes -----------------------------------------------------------------------------------------------------------------------------
def _vrows(W, planes=2):
    """[planes, 9, W] over values 0..3: a full row of one value, 1 2 1 2, the runs 1 1 2 2 1, value changes at 62|63, 63|64 and 64|65,
    1 2 1 at the start and across the word boundary, random, one change at 63|64 exactly, 1 0 1 beside 1 2 1, a full row."""
    rng = np.random.default_rng(100 + W)
    x = np.zeros((planes, 9, W), dtype=np.int64)
    col = np.arange(W)
    for z in range(planes):
        x[z, 0] = 1
        x[z, 1] = 1 + col % 2
        x[z, 2] = np.resize(np.array([1, 1, 2, 2, 1]), W)
        x[z, 3] = np.where(col < 63, 1, np.where(col == 63, 2, np.where(col == 64, 1, 2)))
        x[z, 4, :3] = (1, 2, 1)[:min(W, 3)]
        x[z, 4, 62:66] = (3, 1, 2, 1)[:max(min(W, 66) - 62, 0)]
        x[z, 5] = rng.integers(0, 4, size=W)
        x[z, 6] = np.where(col < 64, 1, 2)
        x[z, 7, 0::4] = 1
        x[z, 7, 2::8] = 2
        x[z, 8] = 3 - z % 2
    x[planes - 1, 8] = 0
    return x


def _random(seed, shape, density, values):
    return B._random(1000 + seed, shape, density, values=values)


def _fill(x, value=2):
    """The binary shape x (value 1) with `value` in its gaps."""
    return np.where(x != 0, 1, value).astype(np.int64)


def _stacked_rows(H, W):
    return np.repeat((1 + np.arange(H) % 2)[:, None], W, axis=1).astype(np.int64)


def _stacked_planes(D, H, W):
    return np.broadcast_to((1 + np.arange(D) % 2)[:, None, None], (D, H, W)).astype(np.int64)


def _checkerboard(shape):
    return (1 + np.indices(shape).sum(axis=0) % 2).astype(np.int64)


def _nest(shape):
    """Class 1 around class 2 around class 1 (concentric boxes, one cell of background all around)."""
    x = np.zeros(shape, dtype=np.int64)
    for k, v in ((1, 1), (3, 2), (5, 1)):
        x[tuple(slice(min(k, s // 2), max(s - k, s // 2)) for s in shape)] = v
    return x


def _diagonal(shape, axes, sea):
    """A line of 2s that steps by one along each of `axes` at once, in a sea of `sea` (0: background, 1: the other class)."""
    return np.where(B._diagonal(shape, axes) != 0, 2, sea).astype(np.int64)


def _blobs(shape, corners, values, extra_on_last=False):
    """3 x 3 (x 3) blobs of `values` at `corners`; the twin case gives the one that comes last in memory one voxel more."""
    x = np.zeros(shape, dtype=np.int64)
    for c, v in zip(corners, values):
        x[tuple(slice(i, i + 3) for i in c)] = v
    if extra_on_last:
        last = list(corners[-1])
        last[-1] += 3
        x[tuple(last)] = values[-1]
    return x


def _single(shape, where, value):
    x = np.zeros(shape, dtype=np.int64)
    x[where] = value
    return x


# name -> (builder, ndim the case is run with, classes)
_BUILDERS = {
    "w1": (lambda: _vrows(1), 3, 4),
    "w63": (lambda: _vrows(63), 3, 4),
    "w64": (lambda: _vrows(64), 3, 4),
    "w65": (lambda: _vrows(65), 3, 4),
    "w130": (lambda: _vrows(130), 3, 4),
    "w130_2d": (lambda: _vrows(130, 1)[0], 2, 4),
    "one_two_one": (lambda: np.array([[1, 2, 1]], dtype=np.int64), 2, 3),                # the two 1s must stay apart
    "one_two_one_rows": (lambda: np.array([[1, 2, 1], [2, 2, 2], [1, 2, 1]], dtype=np.int64), 2, 3),
    "stacked_rows": (lambda: _stacked_rows(7, 70), 2, 3),                                # vertical contact of different values
    "stacked_planes": (lambda: _stacked_planes(5, 4, 70), 3, 3),
    "checkerboard": (lambda: _checkerboard((9, 10, 11)), 3, 3),                          # diagonal contact of different values
    "checkerboard_2d": (lambda: _checkerboard((9, 67)), 2, 3),
    "nest_2d": (lambda: _nest((17, 70)), 2, 3),
    "nest_3d": (lambda: _nest((13, 14, 15)), 3, 3),
    "diagonal_2d": (lambda: _diagonal((12, 12), (0, 1), 1), 2, 3),
    "diagonal_3d": (lambda: _diagonal((10, 10, 10), (0, 1, 2), 1), 3, 3),                # the 2s are joined by connectivity 3 only
    "diagonal_zy": (lambda: _diagonal((8, 8, 5), (0, 1), 1), 3, 3),                      # ... from connectivity 2 on
    "diagonal_zx": (lambda: _diagonal((8, 5, 8), (0, 2), 1), 3, 3),
    "diagonal_3d_alone": (lambda: _diagonal((10, 10, 10), (0, 1, 2), 0), 3, 3),
    "anti_diagonal": (lambda: np.ascontiguousarray(_diagonal((8, 8, 8), (0, 1, 2), 1)[:, ::-1, ::-1]), 3, 3),
    "serpentine": (lambda: _fill(B._serpentine(33, 65)), 2, 3),                          # long walks, the gaps are a second value
    "serpentine_3d": (lambda: _fill(B._serpentine_3d(6, 9, 65)), 3, 3),
    "comb": (lambda: _fill(B._comb(20, 65)), 2, 3),
    "comb_3d": (lambda: _fill(np.stack([B._comb(9, 33), np.zeros((9, 33), dtype=np.int64), B._comb(9, 33)])), 3, 3),
    "h70": (lambda: _random(4, (3, 70, 5), 0.45, (1, 2, 3)), 3, 4),                      # more rows than one wave has lanes
    "d70": (lambda: _random(5, (70, 2, 6), 0.45, (1, 2, 3)), 3, 4),
    "h70_2d": (lambda: _random(6, (70, 7), 0.45, (1, 2, 3)), 2, 4),
    "slice_as_2d": (lambda: _random(7, (1, 12, 20), 0.6, (1, 2)), 2, 3),                 # [1, H, W] with ndim 2 ...
    "slice_as_3d": (lambda: _random(7, (1, 12, 20), 0.6, (1, 2)), 3, 3),                 # ... and the same array with ndim 3
    "map_as_3d": (lambda: _random(7, (12, 20), 0.6, (1, 2)), 3, 3),                      # [H, W] with ndim 3
    "tie_same_class": (lambda: _blobs((10, 30), [(1, 1), (6, 20)], (1, 1)), 2, 3),
    "tie_same_class_later_larger": (lambda: _blobs((10, 30), [(1, 1), (6, 20)], (1, 1), extra_on_last=True), 2, 3),
    "tie_two_classes": (lambda: _blobs((10, 30), [(1, 1), (6, 20)], (2, 1)), 2, 3),      # row 0: the class-2 blob comes first
    "tie_two_classes_later_larger": (lambda: _blobs((10, 30), [(1, 1), (6, 20)], (2, 1), extra_on_last=True), 2, 3),
    "tie_three": (lambda: _blobs((5, 10, 30), [(1, 6, 20), (1, 1, 1), (1, 1, 10)], (1, 2, 1)), 3, 4),
    "tie_three_later_larger": (lambda: _blobs((5, 10, 30), [(1, 1, 1), (1, 1, 10), (1, 6, 20)], (2, 1, 1), extra_on_last=True), 3, 4),
    "absent_class": (lambda: _random(8, (6, 7, 70), 0.4, (1, 3)), 3, 4),                 # class 2 absent, class 3 present
    "classes_above_values": (lambda: _random(9, (6, 7, 70), 0.4, (1, 2)), 3, 9),
    "all_zeros": (lambda: np.zeros((3, 4, 5), dtype=np.int64), 3, 3),
    "all_zeros_2d": (lambda: np.zeros((4, 5), dtype=np.int64), 2, 4),
    "last_corner": (lambda: _single((3, 4, 65), (-1, -1, -1), 2), 3, 3),
    "all_one_value": (lambda: np.full((4, 5, 66), 2, dtype=np.int64), 3, 3),
    "out_of_range": (lambda: _random(10, (6, 7, 9), 0.7, (-1, -7, 3, 8, 1, 2, 2, 1)), 3, 3),
    "out_of_range_2d": (lambda: _random(11, (9, 70), 0.7, (-1, 4, 9, 1, 2, 3, 3)), 2, 4),
    "only_out_of_range": (lambda: _random(12, (5, 9), 0.5, (-3, 2, 7)), 2, 2),
    "classes_2": (lambda: _random(13, (6, 9, 70), 0.3, (1,)), 3, 2),
    "classes_256": (lambda: _random(14, (6, 9, 70), 0.5, (1, 128, 255, 255, 254)), 3, 256),
    "classes_256_out": (lambda: _random(15, (9, 70), 0.5, (1, 255, 256, 300)), 2, 256),
}
for _i, (_shape, _nd) in enumerate((((20, 33, 70), 3), ((40, 130), 2))):
    for _j, _dens in enumerate((0.1, 0.3, 0.6)):
        for _nv in (3, 8):
            _BUILDERS[f"random_{_nd}d_{_dens}_v{_nv}"] = (functools.partial(_random, 20 + 10 * _i + 3 * _j + _nv, _shape, _dens,
                                                                            tuple(range(1, _nv + 1))), _nd, _nv + 1)
CASES = list(_BUILDERS)
EMPTY = ("all_zeros", "all_zeros_2d", "only_out_of_range")
BINARY_OF_B = [n for n in B.CASES if n not in ("negative_labels", "classes_1_to_3")]     # cc_kernel_refs' cases with values 0 / 1 only


@functools.lru_cache(maxsize=None)
def case(name):
    """(array, ndim, classes); the array is read-only."""
    build, ndim, classes = _BUILDERS[name]
    x = np.ascontiguousarray(build())
    x.setflags(write=False)
    return x, ndim, classes


SMALL = [n for n in CASES if case(n)[0].size <= FLOOD_MAX_VOXELS]
RUNS = [(n, c) for n in CASES for c in range(1, case(n)[1] + 1)]                  # every case at every connectivity
SMALL_RUNS = [(n, c) for n, c in RUNS if n in SMALL]


# ---- references: (labels int32, keep uint8, info int64 [C + 1, 3]) in the shape of x ---------------------------------------------------
def scipy_ref(x, connectivity, ndim, classes):
    from scipy.ndimage import generate_binary_structure, label
    x = np.asarray(x)
    a = _as_ndim(x, x.ndim if ndim is None else ndim)
    structure = generate_binary_structure(a.ndim, connectivity)
    labels, keep = np.zeros(a.size, np.int32), np.zeros(a.size, np.uint8)
    info = np.zeros((classes + 1, 3), dtype=np.int64)
    info[:, 1] = -1
    firsts, sizes = [], []
    for c in range(1, classes):
        lab, n = label(a == c, structure=structure)
        if n == 0:
            continue
        flat = lab.reshape(-1)
        idx = np.flatnonzero(flat)
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)
        counts = np.bincount(flat, minlength=n + 1)
        labels[idx] = first[flat[idx]] + 1
        win = int(np.argmax(counts[1:])) + 1                                       # scipy numbers in raster order: the first of equals
        keep[flat == win] = 1
        info[c] = (n, first[win], counts[win])
        firsts.append(first[1:])
        sizes.append(counts[1:])
    if firsts:
        firsts, sizes = np.concatenate(firsts), np.concatenate(sizes)
        order = np.argsort(firsts)                                                 # the raster-order numbering over all classes
        win = order[int(np.argmax(sizes[order]))]
        info[0] = (len(firsts), firsts[win], sizes[win])
    out = np.flatnonzero((a.reshape(-1) < 0) | (a.reshape(-1) >= classes))
    info[classes] = (out.size, out[0] if out.size else -1, 0)
    return labels.reshape(x.shape), keep.reshape(x.shape), info


def flood_ref(x, connectivity, ndim, classes):
    x = np.asarray(x)
    a = _as_ndim(x, x.ndim if ndim is None else ndim)
    shape = a.shape
    val = [int(v) if 1 <= v <= classes - 1 else 0 for v in a.reshape(-1).tolist()]
    steps = [o for o in itertools.product((-1, 0, 1), repeat=a.ndim) if 0 < sum(v != 0 for v in o) <= connectivity]
    strides = [int(np.prod(shape[i + 1:])) for i in range(a.ndim)]
    labels = [0] * len(val)
    best = {c: [0, -1, 0] for c in range(classes)}                                  # per class (0: all) {components, root, size}
    for start in range(len(val)):                                                   # raster order: `start` is its component's smallest index
        if not val[start] or labels[start]:
            continue
        labels[start] = start + 1
        todo, size = [start], 0
        while todo:
            nxt = []
            for v in todo:
                size += 1
                pos = [(v // strides[i]) % shape[i] for i in range(a.ndim)]
                for o in steps:
                    if all(0 <= pos[i] + o[i] < shape[i] for i in range(a.ndim)):
                        u = v + sum(o[i] * strides[i] for i in range(a.ndim))
                        if val[u] == val[start] and not labels[u]:
                            labels[u] = start + 1
                            nxt.append(u)
            todo = nxt
        for c in (0, val[start]):
            best[c][0] += 1
            if size > best[c][2]:                                                   # strictly larger: the first of equals stays
                best[c][1:] = [start, size]
    labels = np.asarray(labels, dtype=np.int32)
    keep = np.zeros(len(val), np.uint8)
    for c in range(1, classes):
        if best[c][0]:
            keep[labels == best[c][1] + 1] = 1
    raw = a.reshape(-1).tolist()
    out = [i for i, v in enumerate(raw) if v < 0 or v >= classes]
    info = np.array([best[c] for c in range(classes)] + [[len(out), out[0] if out else -1, 0]], dtype=np.int64)
    return labels.reshape(x.shape), keep.reshape(x.shape), info


@functools.lru_cache(maxsize=None)
def ref(name, connectivity):
    """scipy_ref of a case (computed once; read-only)."""
    x, ndim, classes = case(name)
    out = scipy_ref(x, connectivity, ndim, classes)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the entry point on guarded buffers --------------------------------------------------------------------------------------------------
def run_guarded(L, x, ndim, connectivity, classes, ws_short=0, passed=None):
    """The entry point itself on exactly-sized buffers with sentinels behind them.  Returns (status, (labels, keep, info) on the host
    - labels and keep in the shape of x -, [(buffer on the host, its size) ...] for the workspace and the three outputs).  ws_short:
    bytes by which the workspace size passed to the entry point falls short (the buffer keeps its size).  passed: {"ndim" |
    "connectivity" | "classes": the value the entry point gets instead} - the buffers are sized for the true ones."""
    a = _as_ndim(x, ndim)
    D, H, W = (1, *a.shape) if a.ndim == 2 else a.shape
    N = D * H * W
    ws_bytes = L.query("arco_cc_value_ws_bytes", D, H, W, classes)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    ws, labels = guarded(ws_bytes // 8, torch.int64).cuda(), guarded(N, torch.int32).cuda()
    keep, info = guarded(N, torch.uint8).cuda(), guarded(3 * (classes + 1), torch.int64).cuda()
    xd = torch.tensor(np.ascontiguousarray(a), dtype=torch.int64).cuda()
    arg = dict(ndim=ndim, connectivity=connectivity, classes=classes)
    arg.update(passed or {})
    rc = L.load().arco_cc_value_largest(L.ptr(xd), D, H, W, arg["ndim"], arg["connectivity"], arg["classes"], L.ptr(ws),
                                        ws_bytes - ws_short, L.ptr(labels), N * 4, L.ptr(keep), N, L.ptr(info), 24 * (classes + 1),
                                        L.stream())
    torch.cuda.synchronize()
    bufs = [(ws.cpu(), ws_bytes // 8), (labels.cpu(), N), (keep.cpu(), N), (info.cpu(), 3 * (classes + 1))]
    out = (bufs[1][0][:N].reshape(x.shape), bufs[2][0][:N].reshape(x.shape), bufs[3][0][:3 * (classes + 1)].reshape(classes + 1, 3))
    return rc, out, bufs
