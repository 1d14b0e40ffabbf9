"""Cases, references and checkers for the connected-component kernels (arco_amd/csrc/cc.hip, arco_amd/utils/cc_gpu.py).

The kernels return, for an integer label volume (foreground = != 0) and a connectivity c in 1..ndim (scipy's
generate_binary_structure(ndim, c)):
  labels   int32, 0 on background, else 1 + the smallest flat index of the voxel's component
  largest  uint8, 1 on the component with the most voxels (ties: the one whose first voxel comes first in memory)
  info     int64 [3] = {components, flat index of the winner's first voxel, its voxel count}; {0, -1, 0} without foreground
Two references that share no code:
  scipy_ref   scipy.ndimage.label; `largest` is getLargestCC's own expression labels == argmax(bincount(labels)[1:]) + 1
  flood_ref   a breadth-first flood fill in raster order in plain Python, for cases of up to FLOOD_MAX_VOXELS voxels
Everything is an integer, so the only check is equality.

A case is an array and the `ndim` it is run with: a [1, H, W] array with ndim 2 is the map [H, W] (connectivity 1..2), an [H, W]
array with ndim 3 is the one-slice volume [1, H, W] (connectivity 1..3).  Each case sits at an edge of one pass of the kernels: a
row is balloted into 64-bit words (widths 1, 63, 64, 65, 130; runs across the word boundaries), a block takes four rows, the
union walk is longest on a serpentine and on a comb whose prongs meet in the last row only."""
import functools
import itertools

import numpy as np
import torch

GUARD = 64                                   # sentinel words behind every output and behind the workspace
SENT = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
FLOOD_MAX_VOXELS = 4000


# ---- volumes -----------------------------------------------------------------------------------------------------------------------------
def _rows(W, planes=2):
    """[planes, 6, W]: a full row, an empty row, runs across the 64-bit word boundaries, every second cell, random, full."""
    rng = np.random.default_rng(W)
    x = np.zeros((planes, 6, W), dtype=np.int64)
    for z in range(planes):
        x[z, 0] = 1
        for lo, hi in ((60, 70), (100, 129), (W - 1, W)):
            x[z, 2, max(min(lo, W - 1), 0):min(hi, W)] = 1
        x[z, 3, z % 2::2] = 1
        x[z, 4] = rng.random(W) < 0.5
        x[z, 5] = 1
    x[planes - 1, 5] = 0
    return x


def _random(seed, shape, density, values=(1,)):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.choice(np.asarray(values, dtype=np.int64), size=shape), 0).astype(np.int64)


def _serpentine(H, W):
    """One component through every second row, joined alternately at the right and at the left end."""
    x = np.zeros((H, W), dtype=np.int64)
    x[0::2] = 1
    x[1::4, W - 1] = 1
    x[3::4, 0] = 1
    return x


def _serpentine_3d(D, H, W):
    """Serpentines on the even planes; an odd plane is one voxel that joins the end of the plane below to the plane above."""
    x = np.zeros((D, H, W), dtype=np.int64)
    x[0::2] = _serpentine(H, W)
    end = W - 1 if ((H - 1) // 2) % 2 == 0 else 0
    assert x[0, H - 1, end] == 1
    x[1::2, H - 1, end] = 1
    return x


def _comb(H, W):
    """Prongs in every second column that meet in the last row only."""
    x = np.zeros((H, W), dtype=np.int64)
    x[:, 0::2] = 1
    x[H - 1] = 1
    return x


def _checkerboard(shape):
    return (np.indices(shape).sum(axis=0) % 2 == 0).astype(np.int64)


def _diagonal(shape, axes):
    """A line that steps by one along each of `axes` at once."""
    x = np.zeros(shape, dtype=np.int64)
    n = min(shape[a] for a in axes)
    idx = [np.full(n, 1) for _ in shape]
    for a in axes:
        idx[a] = np.arange(n)
    x[tuple(idx)] = 1
    return x


def _blobs(shape, corners, extra_on_last=False):
    """3 x 3 (x 3) blobs at `corners`; the twin case gives the one that comes last in memory one voxel more."""
    x = np.zeros(shape, dtype=np.int64)
    for c in corners:
        x[tuple(slice(i, i + 3) for i in c)] = 1
    if extra_on_last:
        last = list(corners[-1])
        last[-1] += 3
        x[tuple(last)] = 1
    return x


def _single(shape, where):
    x = np.zeros(shape, dtype=np.int64)
    x[where] = 1
    return x


# name -> (builder, ndim the case is run with)
_BUILDERS = {
    "w1": (lambda: _rows(1), 3),
    "w63": (lambda: _rows(63), 3),
    "w64": (lambda: _rows(64), 3),
    "w65": (lambda: _rows(65), 3),
    "w130": (lambda: _rows(130), 3),
    "w130_2d": (lambda: _rows(130, 1)[0], 2),
    "h1_d1": (lambda: _random(1, (1, 1, 9), 0.5), 3),
    "h2_d3": (lambda: _random(2, (3, 2, 9), 0.5), 3),
    "h3_d2": (lambda: _random(3, (2, 3, 9), 0.5), 3),
    "h70": (lambda: _random(4, (3, 70, 5), 0.45), 3),                       # more rows than one wave has lanes
    "d70": (lambda: _random(5, (70, 2, 6), 0.45), 3),
    "h70_2d": (lambda: _random(6, (70, 7), 0.45), 2),
    "slice_as_2d": (lambda: _random(7, (1, 12, 20), 0.4), 2),               # [1, H, W] with ndim 2 ...
    "slice_as_3d": (lambda: _random(7, (1, 12, 20), 0.4), 3),               # ... and the same array with ndim 3
    "map_as_3d": (lambda: _random(7, (12, 20), 0.4), 3),                    # [H, W] with ndim 3
    "serpentine": (lambda: _serpentine(33, 65), 2),
    "serpentine_3d": (lambda: _serpentine_3d(6, 9, 65), 3),
    "comb": (lambda: _comb(20, 65), 2),
    "comb_3d": (lambda: np.stack([_comb(9, 33), np.zeros((9, 33), dtype=np.int64), _comb(9, 33)]), 3),
    "checkerboard": (lambda: _checkerboard((9, 10, 11)), 3),
    "checkerboard_2d": (lambda: _checkerboard((9, 67)), 2),
    "diagonal_2d": (lambda: _diagonal((12, 12), (0, 1)), 2),
    "diagonal_3d": (lambda: _diagonal((10, 10, 10), (0, 1, 2)), 3),         # joined by connectivity 3 only
    "diagonal_zy": (lambda: _diagonal((8, 8, 5), (0, 1)), 3),               # joined from connectivity 2 on
    "diagonal_zx": (lambda: _diagonal((8, 5, 8), (0, 2)), 3),
    "anti_diagonal": (lambda: np.ascontiguousarray(_diagonal((8, 8, 8), (0, 1, 2))[:, ::-1, ::-1]), 3),
    "tie_two": (lambda: _blobs((10, 30), [(1, 1), (6, 20)]), 2),
    "tie_two_later_larger": (lambda: _blobs((10, 30), [(1, 1), (6, 20)], extra_on_last=True), 2),
    "tie_three": (lambda: _blobs((5, 10, 30), [(1, 6, 20), (1, 1, 1), (1, 1, 10)]), 3),
    "tie_three_later_larger": (lambda: _blobs((5, 10, 30), [(1, 1, 1), (1, 1, 10), (1, 6, 20)], extra_on_last=True), 3),
    "all_ones": (lambda: np.ones((4, 5, 66), dtype=np.int64), 3),
    "last_corner": (lambda: _single((3, 4, 65), (-1, -1, -1)), 3),
    "all_zeros": (lambda: np.zeros((3, 4, 5), dtype=np.int64), 3),
    "all_zeros_2d": (lambda: np.zeros((4, 5), dtype=np.int64), 2),
    "negative_labels": (lambda: _random(8, (6, 7, 9), 0.5, values=(-1, -7, 2)), 3),
    "classes_1_to_3": (lambda: _random(9, (6, 7, 70), 0.35, values=(1, 2, 3)), 3),
    "random_small": (lambda: _random(10, (6, 9, 70), 0.3), 3),
    "random_0.1": (lambda: _random(11, (20, 33, 70), 0.1), 3),
    "random_0.3": (lambda: _random(12, (20, 33, 70), 0.3), 3),
    "random_0.6": (lambda: _random(13, (20, 33, 70), 0.6), 3),
    "random_2d_0.1": (lambda: _random(14, (40, 130), 0.1), 2),
    "random_2d_0.3": (lambda: _random(15, (40, 130), 0.3), 2),
    "random_2d_0.6": (lambda: _random(16, (40, 130), 0.6), 2),
}
CASES = list(_BUILDERS)
EMPTY = ("all_zeros", "all_zeros_2d")


@functools.lru_cache(maxsize=None)
def case(name):
    """(array, ndim); the array is read-only."""
    build, ndim = _BUILDERS[name]
    x = np.ascontiguousarray(build())
    x.setflags(write=False)
    return x, ndim


SMALL = [n for n in CASES if case(n)[0].size <= FLOOD_MAX_VOXELS]
RUNS = [(n, c) for n in CASES for c in range(1, case(n)[1] + 1)]                  # every case at every connectivity
SMALL_RUNS = [(n, c) for n, c in RUNS if n in SMALL]


def _as_ndim(x, ndim):
    """The array as the kernels take it with `ndim`: [1, H, W] -> [H, W] for ndim 2, [H, W] -> [1, H, W] for ndim 3."""
    x = np.asarray(x)
    if ndim == 2 and x.ndim == 3:
        assert x.shape[0] == 1
        return x[0]
    if ndim == 3 and x.ndim == 2:
        return x[None]
    assert x.ndim == ndim
    return x


# ---- references: (labels int32, largest uint8, info int64 [3]) in the shape of x -------------------------------------------------------
def scipy_ref(x, connectivity, ndim=None):
    from scipy.ndimage import generate_binary_structure, label
    x = np.asarray(x)
    a = _as_ndim(x, x.ndim if ndim is None else ndim)
    lab, n = label(a, structure=generate_binary_structure(a.ndim, connectivity))
    flat = lab.reshape(-1)
    if n == 0:
        return np.zeros(x.shape, np.int32), np.zeros(x.shape, np.uint8), np.array([0, -1, 0], dtype=np.int64)
    idx = np.flatnonzero(flat)
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat[idx], idx)
    first[0] = -1
    counts = np.bincount(flat)
    win = int(np.argmax(counts[1:])) + 1
    largest = lab == np.argmax(np.bincount(lab.flat)[1:]) + 1                       # getLargestCC's expression, test_util.py:11-15
    return ((first[flat] + 1).astype(np.int32).reshape(x.shape), largest.astype(np.uint8).reshape(x.shape),
            np.array([n, first[win], counts[win]], dtype=np.int64))


def flood_ref(x, connectivity, ndim=None):
    x = np.asarray(x)
    a = _as_ndim(x, x.ndim if ndim is None else ndim)
    shape = a.shape
    fg = (a != 0).reshape(-1).tolist()
    steps = [o for o in itertools.product((-1, 0, 1), repeat=a.ndim) if 0 < sum(v != 0 for v in o) <= connectivity]
    strides = [int(np.prod(shape[i + 1:])) for i in range(a.ndim)]
    labels = [0] * len(fg)
    n, best_root, best_size = 0, -1, 0
    for start in range(len(fg)):                                                    # raster order: `start` is its component's smallest index
        if not fg[start] or labels[start]:
            continue
        n += 1
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
                        if fg[u] and not labels[u]:
                            labels[u] = start + 1
                            nxt.append(u)
            todo = nxt
        if size > best_size:                                                        # strictly larger: the first of equals stays
            best_root, best_size = start, size
    labels = np.asarray(labels, dtype=np.int32).reshape(x.shape)
    largest = (labels == best_root + 1).astype(np.uint8) if n else np.zeros(x.shape, np.uint8)
    return labels, largest, np.array([n, best_root, best_size], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def ref(name, connectivity):
    """scipy_ref of a case (computed once; read-only)."""
    x, ndim = case(name)
    out = scipy_ref(x, connectivity, ndim)
    for a in out:
        a.setflags(write=False)
    return out


# ---- checkers -----------------------------------------------------------------------------------------------------------------------------
def same(got, exp):
    """Three arrays or tensors equal the reference triple in dtype, shape and every element."""
    ok = len(got) == 3
    for g, e in zip(got, exp):
        g = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        ok = ok and g.dtype == e.dtype and g.shape == e.shape and bool(np.array_equal(g, e))
    return ok


def guarded(n, dtype):
    """A buffer of n elements plus GUARD sentinel elements, all sentinel; the kernels get n."""
    return torch.full((n + GUARD,), SENT[dtype], dtype=dtype)


def guards_intact(buf, n):
    return buf.numel() == n + GUARD and bool((buf[n:] == SENT[buf.dtype]).all().item())


def untouched(buf):
    return bool((buf == SENT[buf.dtype]).all().item())


def run_guarded(L, x, ndim, connectivity, ws_short=0):
    """The entry point itself on exactly-sized buffers with sentinels behind them.  Returns (status, (labels, largest, info) on the
    host in the shape of x, [(buffer on the host, its size) ...] for the workspace and the three outputs).  ws_short: bytes by which the
    workspace size passed to the entry point falls short (the buffer keeps its size)."""
    a = _as_ndim(x, ndim)
    D, H, W = (1, *a.shape) if a.ndim == 2 else a.shape
    N = D * H * W
    ws_bytes = L.query("arco_cc_ws_bytes", D, H, W)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws, labels = guarded(ws_bytes // 4, torch.int32).cuda(), guarded(N, torch.int32).cuda()
    largest, info = guarded(N, torch.uint8).cuda(), guarded(3, torch.int64).cuda()
    xd = torch.tensor(np.ascontiguousarray(a), dtype=torch.int64).cuda()
    rc = L.load().arco_cc_largest(L.ptr(xd), D, H, W, ndim, connectivity, L.ptr(ws), ws_bytes - ws_short, L.ptr(labels), N * 4,
                                  L.ptr(largest), N, L.ptr(info), 24, L.stream())
    torch.cuda.synchronize()
    bufs = [(ws.cpu(), ws_bytes // 4), (labels.cpu(), N), (largest.cpu(), N), (info.cpu(), 3)]
    out = (bufs[1][0][:N].reshape(x.shape), bufs[2][0][:N].reshape(x.shape), bufs[3][0][:3])
    return rc, out, bufs
