"""numpy restatements of csrc/patch_pool.hip (arco_patch_pool_fwd / arco_patch_pool_bwd), shared by tests/test_patch_pool_cpu.py and
tests/test_patch_pool_gpu.py.  No torch op on the pooled path.

  windows(patch, pool)          the cells' [lo, hi) local ranges: floor(i * patch / pool), ceil((i + 1) * patch / pool)
  patch_pool_fwd_ref64 / patch_pool_bwd_ref64     the map and its adjoint in float64
  patch_pool_fwd_f32 / patch_pool_bwd_f32         the kernels' fp32 operations, element by element, in the kernels' order

x is [B, C, n...], y and gy are [P, B, C, pool...], the patch number first, the first spatial axis outermost in it."""
import itertools

import numpy as np

# (n, patch, pool, B, C)
CASES = [
    ((14, 12, 10), 5, 2, 2, 3),     # odd patch: three covering patches, overlapping windows, an uncovered tail voxel on axis 0
    ((30, 30, 20), 20, 8, 1, 2),    # the 3-D default geometry in miniature, one patch on the last axis
    ((9, 8, 8), 4, 8, 2, 1),        # pool > patch
    ((32, 32, 32), 10, 4, 2, 2),    # 125 patches
    ((16, 16, 16), 16, 1, 3, 2),    # a single patch, global mean
    ((12, 12, 12), 4, 4, 1, 4),     # identity windows
    ((32, 32, 32), 16, 2, 2, 2),    # divisible, the existing tests' configuration
    ((37, 50), 10, 4, 2, 4),        # 2-D
    ((64, 64), 16, 4, 4, 4),        # 2-D
    ((21, 16), 7, 3, 1, 1),         # 2-D
]
CASE_IDS = ["x".join(map(str, c[0])) + f"-p{c[1]}-o{c[2]}" for c in CASES]


def case_input(case, seed=0):
    """x and gy of a case, fp32, seeded; values of both signs with a spread of magnitudes."""
    n, patch, pool, B, C = case
    rs = np.random.RandomState(1000 + seed)
    x = (rs.standard_normal((B, C) + tuple(n)) * np.exp(rs.uniform(-2, 2, (B, C) + tuple(n)))).astype(np.float32)
    P = int(np.prod([len(starts(s, patch)) for s in n]))
    shp = (P, B, C) + (pool,) * len(n)
    gy = (rs.standard_normal(shp) * np.exp(rs.uniform(-2, 2, shp))).astype(np.float32)
    return x, gy


def windows(patch, pool):
    return [((i * patch) // pool, -((-(i + 1) * patch) // pool)) for i in range(pool)]


def starts(n, patch):
    return list(range(0, n - patch + 1, patch // 2))


def _patch_origins(n, patch):
    return list(itertools.product(*[starts(s, patch) for s in n]))


def _cells(patch, pool, nd):
    return list(itertools.product(*[list(enumerate(windows(patch, pool)))] * nd))


def patch_pool_fwd_ref64(x, patch, pool):
    x = np.asarray(x, np.float64)
    n = x.shape[2:]
    out = []
    for org in _patch_origins(n, patch):
        y = np.empty(x.shape[:2] + (pool,) * len(n))
        for cell in _cells(patch, pool, len(n)):
            idx = tuple(i for i, _ in cell)
            sl = tuple(slice(o + lo, o + hi) for o, (_, (lo, hi)) in zip(org, cell))
            y[(slice(None), slice(None)) + idx] = x[(slice(None), slice(None)) + sl].mean(axis=tuple(range(2, 2 + len(n))))
        out.append(y)
    return np.stack(out)


def patch_pool_bwd_ref64(gy, n, patch, pool):
    gy = np.asarray(gy, np.float64)
    gx = np.zeros(gy.shape[1:3] + tuple(n))
    for p, org in enumerate(_patch_origins(n, patch)):
        for cell in _cells(patch, pool, len(n)):
            idx = tuple(i for i, _ in cell)
            sl = tuple(slice(o + lo, o + hi) for o, (_, (lo, hi)) in zip(org, cell))
            cnt = np.prod([hi - lo for _, (lo, hi) in cell])
            gx[(slice(None), slice(None)) + sl] += (gy[(p, slice(None), slice(None)) + idx] / cnt).reshape(gy.shape[1:3] + (1,) * len(n))
    return gx


def patch_pool_fwd_f32(x, patch, pool):
    """Per output element: acc = 0.f; acc += x[...] over the window, axis 0 outermost, every axis ascending; acc / (float)count.
    The loop over the window's offsets is the kernel's; every patch, batch and channel takes the same steps, so they go as arrays."""
    x = np.asarray(x, np.float32)
    n = x.shape[2:]
    nd = len(n)
    orgs = _patch_origins(n, patch)
    xp = np.stack([x[(slice(None), slice(None)) + tuple(slice(o, o + patch) for o in org)] for org in orgs])     # [P, B, C, patch...]
    y = np.empty(xp.shape[:3] + (pool,) * nd, np.float32)
    for cell in _cells(patch, pool, nd):
        idx = tuple(i for i, _ in cell)
        acc = np.zeros(xp.shape[:3], np.float32)
        for off in itertools.product(*[range(lo, hi) for _, (lo, hi) in cell]):
            acc = acc + xp[(slice(None),) * 3 + off]
        cnt = np.float32(int(np.prod([hi - lo for _, (lo, hi) in cell])))
        y[(slice(None),) * 3 + idx] = acc / cnt
    return y


def _axis_slots(n, patch, pool):
    """Per coordinate v of an axis, in the kernel's order (patches ascending, inside a patch its covering cells ascending): the list of
    (patch index, cell, window length).  As arrays [slots, n] with a validity mask, padded to the longest list."""
    step, win = patch // 2, windows(patch, pool)
    n_p = len(starts(n, patch))
    per_v = []
    for v in range(n):
        p_lo = 0 if v < patch else (v - patch) // step + 1
        p_hi = min(v // step, n_p - 1)
        lst = []
        for p in range(p_lo, p_hi + 1):
            l = v - p * step
            i_lo, i_hi = (l * pool) // patch, min(((l + 1) * pool - 1) // patch, pool - 1)
            for i in range(i_lo, i_hi + 1):
                assert win[i][0] <= l < win[i][1]
                lst.append((p, i, win[i][1] - win[i][0]))
        # the computed ranges are ALL the covering tuples
        assert len(lst) == sum(1 for p in range(n_p) for (lo, hi) in win if lo <= v - p * step < hi)
        per_v.append(lst)
    S = max(1, max(len(l) for l in per_v))
    arr = np.zeros((3, S, n), np.int64)
    ok = np.zeros((S, n), bool)
    for v, lst in enumerate(per_v):
        for s, t in enumerate(lst):
            arr[:, s, v] = t
            ok[s, v] = True
    return arr[0], arr[1], arr[2], ok, n_p


def patch_pool_bwd_f32(gy, n, patch, pool):
    """Per input voxel: acc = 0.f; acc += gy[p, b, c, cell] / (float)count(cell) over the covering (patch, cell) tuples, nested loops
    p0, i0, p1, i1(, p2, i2) from the outermost, all ascending.  Returns (gx, sum of |term| in float64, number of terms) per voxel.
    Slot k of an axis is the k-th (patch, cell) tuple of the coordinate in that order; a voxel without a k-th tuple adds nothing."""
    gy = np.asarray(gy, np.float32)
    nd = len(n)
    B, C = gy.shape[1:3]
    ax = [_axis_slots(n[d], patch, pool) for d in range(nd)]
    n_p = [a[4] for a in ax]
    gx = np.zeros((B, C) + tuple(n), np.float32)
    mag = np.zeros((B, C) + tuple(n), np.float64)
    terms = np.zeros(tuple(n), np.int64)
    grids = np.meshgrid(*[np.arange(s) for s in n], indexing="ij")
    for slot in itertools.product(*[range(a[3].shape[0]) for a in ax]):
        p = np.zeros(tuple(n), np.int64)
        cnt = np.ones(tuple(n), np.int64)
        ok = np.ones(tuple(n), bool)
        cell = []
        for d in range(nd):
            pd, idd, ld, okd, _ = ax[d]
            p = p * n_p[d] + pd[slot[d]][grids[d]]
            cnt = cnt * ld[slot[d]][grids[d]]
            ok &= okd[slot[d]][grids[d]]
            cell.append(idd[slot[d]][grids[d]])
        if not ok.any():
            continue
        g = gy[(p, slice(None), slice(None)) + tuple(cell)]                 # [n..., B, C]
        g = np.moveaxis(g, (-2, -1), (0, 1))                                # [B, C, n...]
        term = g / np.maximum(cnt, 1).astype(np.float32)
        gx = np.where(ok, gx + term, gx).astype(np.float32)
        mag += np.where(ok, np.abs(term.astype(np.float64)), 0.0)
        terms += ok
    return gx, mag, terms
