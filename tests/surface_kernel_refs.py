"""Cases, references and checkers for the surface-distance kernels (arco_amd/csrc/surface.hip, arco_amd/utils/surface_gpu.py).

The kernels return hist[class][direction][k] = number of border voxels of A whose SQUARED distance to the nearest border voxel of B is
k (direction 0: A = pred == c, B = gt == c; direction 1 the other way round), nbins = sum((s - 1)^2) + 1 bins.  Two references:
  scipy_hist   from metrics.binary._surface_distances (scipy's erosion and distance transform) through np.rint(d ** 2);
  brute_hist   an O(n^2) restatement in integer arithmetic that shares no code with scipy.ndimage (the border and the minimum
               of tests/test_oracle_golden.py::_brute_surface_distances without the square root).
Everything is integer counting, so the only check is `exact`.

Shapes: each sits at an edge of one pass of the kernels.  The min-plus pass stages its line in an LDS tile of 256 entries, so the
lines of 300 are the ones longer than the tile; a row of 130 is two ballot words plus a ragged third; 70 and 67 are lines longer
than one wave along H and along D."""
import functools

import numpy as np
import torch

from arco_amd.utils import metrics

GUARD = 64                                   # sentinel words behind the histogram and behind the workspace
SENT32 = 0x5A5A5A5A
SENT64 = 0x5A5A5A5A5A5A5A5A
BRUTE_MAX_VOXELS = 4000                      # the brute force builds an |border A| x |border B| table


def nbins(shape):
    return int(sum((int(s) - 1) ** 2 for s in shape)) + 1


# ---- label maps ------------------------------------------------------------------------------------------------------------------------
def _grow(x):
    pad = np.pad(x, 1)
    g = x.copy()
    for ax in range(x.ndim):
        for sh in (-1, 1):
            sl = [slice(1, -1)] * x.ndim
            sl[ax] = slice(1 + sh, x.shape[ax] + 1 + sh)
            g |= pad[tuple(sl)]
    return g


def label_map(rng, shape, n_cls=4, absent=()):
    """Classes 0..n_cls-1: blobs grown from random seeds (one seed of class 1 in the first corner and one of the last class in the
    opposite corner, so objects touch the array faces), 3 % pinholes (interior borders).  Every class outside `absent` has a voxel."""
    lab = np.zeros(shape, dtype=np.int64)
    present = [c for c in range(1, n_cls) if c not in absent]
    for c in present:
        x = rng.random(shape) < 0.08
        if c == present[0]:
            x[(0,) * len(shape)] = True
        if c == present[-1]:
            x[(-1,) * len(shape)] = True
        for _ in range(2):
            x = _grow(x)
        lab[x] = c
    lab[rng.random(shape) < 0.03] = 0
    flat = lab.reshape(-1)
    for c in present:                        # a class that the later ones painted over gets one voxel back
        if not (flat == c).any():
            counts = np.bincount(flat, minlength=n_cls)
            donors = np.flatnonzero(counts[flat] > 1)
            flat[donors[rng.integers(len(donors))]] = c
    return lab


def _random_case(seed, shape, classes=(1, 2, 3), absent_gt=()):
    rng = np.random.default_rng(seed)
    return dict(pred=label_map(rng, shape), gt=label_map(rng, shape, absent=absent_gt), classes=list(classes), empty=list(absent_gt))


def _two_voxels(shape, p, q):
    pred, gt = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    pred[p] = 1
    gt[q] = 1
    return dict(pred=pred, gt=gt, classes=[1], empty=[])


def _identical(seed, shape):
    lab = label_map(np.random.default_rng(seed), shape)
    return dict(pred=lab, gt=lab.copy(), classes=[1, 2, 3], empty=[])


def _full(seed, shape):
    rng = np.random.default_rng(seed)
    return dict(pred=np.ones(shape, dtype=np.int64), gt=(label_map(rng, shape) > 0).astype(np.int64), classes=[1], empty=[])


_BUILDERS = {
    "2d_24x20": lambda: _random_case(0, (24, 20)),
    "2d_1x7": lambda: _random_case(1, (1, 7)),
    "2d_two_voxels": lambda: _two_voxels((9, 9), (1, 1), (4, 5)),                  # one count in bin 3^2 + 4^2 = 25
    "3d_14x12x10": lambda: _random_case(2, (14, 12, 10)),
    "3d_9x16x11": lambda: _random_case(3, (9, 16, 11)),
    "3d_3x5x130": lambda: _random_case(4, (3, 5, 130)),                            # a row of two ballot words and a ragged third
    "3d_5x70x9": lambda: _random_case(5, (5, 70, 9)),                              # a line longer than one wave along H
    "3d_67x4x6": lambda: _random_case(6, (67, 4, 6)),                              # ... and along D
    "3d_2x3x300": lambda: _random_case(7, (2, 3, 300)),                            # a row of five ballot words
    "3d_2x300x3": lambda: _random_case(8, (2, 300, 3)),                            # a line longer than the LDS tile along H
    "3d_300x3x2": lambda: _random_case(9, (300, 3, 2)),                            # ... and along D
    "3d_corners": lambda: _two_voxels((6, 7, 8), (0, 0, 0), (5, 6, 7)),            # the only count lands in the LAST bin
    "3d_identical": lambda: _identical(10, (14, 12, 10)),                          # everything in bin 0
    "3d_full": lambda: _full(11, (7, 6, 9)),                                       # the border is the array's shell
    "3d_absent": lambda: _random_case(12, (9, 16, 11), absent_gt=(2,)),            # class 2 missing from gt: two empty rows
    "3d_from_class_2": lambda: _random_case(13, (14, 12, 10), classes=(2, 3)),     # a class range that starts at 2
}
CASES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case with its scipy reference (computed once; treat as read-only)."""
    c = _BUILDERS[name]()
    c["name"], c["shape"], c["ndim"] = name, c["pred"].shape, c["pred"].ndim
    c["nbins"] = nbins(c["shape"])
    c["ref"] = np.stack([scipy_hist(c["pred"] == k, c["gt"] == k, c["nbins"]) for k in c["classes"]])
    for a in (c["pred"], c["gt"], c["ref"]):
        a.setflags(write=False)
    return c


# ---- references: [2][nbins] int64 for one pair of boolean masks ----------------------------------------------------------------------------
def scipy_hist(a, b, nb):
    out = np.zeros((2, nb), dtype=np.int64)
    if a.any() and b.any():
        for d, (x, y) in enumerate(((a, b), (b, a))):
            dist = metrics.binary._surface_distances(x, y)
            out[d] = np.bincount(np.rint(dist ** 2).astype(np.int64), minlength=nb)
    return out


def _brute_border(x):
    pad = np.pad(x, 1, constant_values=False)
    core = np.ones_like(x)
    for ax in range(x.ndim):
        for sh in (-1, 1):
            sl = [slice(1, -1)] * x.ndim
            sl[ax] = slice(1 + sh, x.shape[ax] + 1 + sh)
            core &= pad[tuple(sl)]
    return x & ~core


def brute_hist(a, b, nb):
    out = np.zeros((2, nb), dtype=np.int64)
    pa, pb = np.argwhere(_brute_border(a)).astype(np.int64), np.argwhere(_brute_border(b)).astype(np.int64)
    if len(pa) and len(pb):
        d2 = ((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)
        out[0] = np.bincount(d2.min(axis=1), minlength=nb)
        out[1] = np.bincount(d2.min(axis=0), minlength=nb)
    return out


# ---- checkers -----------------------------------------------------------------------------------------------------------------------------
def exact(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = np.asarray(ref)
    return got.shape == ref.shape and got.dtype == np.int64 and bool(np.array_equal(got, ref))


def guarded(n, dtype):
    """A buffer of n words plus GUARD sentinel words; the kernels get n."""
    return torch.full((n + GUARD,), SENT32 if dtype == torch.int32 else SENT64, dtype=dtype)


def guards_intact(buf, n):
    sent = SENT32 if buf.dtype == torch.int32 else SENT64
    return buf.numel() == n + GUARD and bool((buf[n:] == sent).all().item())


def device_maps(c):
    return torch.tensor(c["pred"]).cuda(), torch.tensor(c["gt"]).cuda()


def run_guarded(L, c):
    """The entry point itself on exactly-sized buffers with sentinels behind them: (hist [nc][2][nbins] on the host, hist buffer,
    its size, workspace buffer, its size)."""
    D, H, W = (1, *c["shape"]) if c["ndim"] == 2 else c["shape"]
    nc = len(c["classes"])
    ws_bytes = L.query("arco_surface_ws_bytes", D, H, W, nc)
    assert ws_bytes == nc * 2 * 2 * D * H * W * 4
    n_hist = nc * 2 * c["nbins"]
    ws, hist = guarded(ws_bytes // 4, torch.int32).cuda(), guarded(n_hist, torch.int64).cuda()
    p, g = device_maps(c)
    L.call("arco_surface_hist", L.ptr(p), L.ptr(g), D, H, W, c["ndim"], c["classes"][0], c["classes"][-1], L.ptr(ws), ws_bytes,
           L.ptr(hist), n_hist * 8)
    torch.cuda.synchronize()
    return hist[:n_hist].view(nc, 2, c["nbins"]).cpu(), hist.cpu(), n_hist, ws.cpu(), ws_bytes // 4
