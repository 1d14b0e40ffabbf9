"""numpy restatements of csrc/patch_head.hip (arco_patch_head_fwd / arco_patch_head_bwd / arco_patch_head_wgrad_finish), shared by
tests/test_patch_head_cpu.py and tests/test_patch_head_kernels_gpu.py.  No torch op on the path.  The geometry and the pooled values
are tests/patch_pool_refs.py's.

  head_fwd_f32(x, patch, pool, layers)        (pooled [P, B, C, pool...], y [P * B, C_L, pool...]), fp32 steps rounded one by one
  head_bwd(pooled, gy, layers)                d_0 [P, B, C, pool...] in the kernel's fp32 steps, and per layer the float64 parameter sums
                                              with the sums of their terms' magnitudes

layers is a list of (W [c_k, c_{k-1}] fp32, b [c_k] fp32 or None).  A POSITION is one (patch, batch, cell) triple."""
import numpy as np

import patch_pool_refs as PR

# (n, patch, pool, B, widths c_0 .. c_L, layers without a bias)
CASES = [
    ((11, 13), 4, 3, 2, (3, 6, 3, 3, 3), ()),          # 2-D, four layers: overlapping windows (0,2) (1,3) (2,4), an uncovered tail on both axes
    ((9, 8, 11), 5, 2, 2, (2, 4, 2), ()),              # 3-D, the teacher's shape: two layers
    ((5, 6), 2, 3, 1, (2, 4, 2), ()),                  # pool > patch: repeated windows
    ((8, 9), 4, 2, 1, (9, 18, 9), ()),                 # the top width tier (17 .. 32)
    ((10, 9), 4, 2, 2, (5, 10, 5, 5), ()),             # the middle tier (9 .. 16)
    ((11, 13), 4, 3, 2, (3, 6, 3, 3), (1,)),           # the second layer without a bias
    ((8, 9), 4, 2, 1, (5, 20, 32, 7, 17), (0, 2)),     # the top tier with four layers, two of them without a bias, the cap of 32
    ((7, 6, 5), 4, 2, 1, (4, 4), ()),                  # a single layer
    # 11^3 patches x 4 x 27 cells = 143 748 positions, above the 131 072 = 512 blocks (PH_BWD_MAX_BLOCKS) x 256 threads (the bottom tier's
    # block) that one pass of the backward's capped grid covers: its stride loop runs twice in the first blocks, and 512 slabs are summed
    ((24, 24, 24), 4, 3, 4, (2, 4, 2), ()),
]
CASE_IDS = ["x".join(map(str, c[0])) + f"-p{c[1]}-o{c[2]}-w" + "_".join(map(str, c[4])) + ("-nobias" if c[5] else "") for c in CASES]
BWD_MAX_BLOCKS, BWD_THREADS_TIER8 = 512, 256


def positions(case):
    n, patch, pool, B = case[:4]
    return int(np.prod([len(PR.starts(s, patch)) for s in n])) * B * pool ** len(n)


def case_input(case, seed=0):
    """x, the layers and gy of a case, fp32, seeded; values of both signs with a spread of magnitudes."""
    n, patch, pool, B, widths, nobias = case
    rs = np.random.RandomState(2000 + seed)
    shp = (B, widths[0]) + tuple(n)
    x = (rs.standard_normal(shp) * np.exp(rs.uniform(-2, 2, shp))).astype(np.float32)
    layers = []
    for k in range(len(widths) - 1):
        W = (rs.standard_normal((widths[k + 1], widths[k])) / np.sqrt(widths[k])).astype(np.float32)
        b = None if k in nobias else (0.5 * rs.standard_normal(widths[k + 1])).astype(np.float32)
        layers.append((W, b))
    P = int(np.prod([len(PR.starts(s, patch)) for s in n]))
    shp = (P * B, widths[-1]) + (pool,) * len(n)
    gy = (rs.standard_normal(shp) * np.exp(rs.uniform(-2, 2, shp))).astype(np.float32)
    return x, layers, gy


def _layer_fwd(a, W, b):
    """a: list of fp32 arrays, one per input channel.  out[j] = b[j] (0.f without a bias); out[j] = out[j] + W[j, i] * a[i], i ascending."""
    out = []
    for j in range(W.shape[0]):
        acc = np.full(a[0].shape, np.float32(0.0) if b is None else b[j], np.float32)
        for i in range(W.shape[1]):
            prod = W[j, i] * a[i]                    # fp32 x fp32, rounded
            acc = acc + prod                         # rounded on its own
        assert acc.dtype == np.float32
        out.append(acc)
    return out


def _channels(t):
    """[P, B, C, cells...] -> list of C arrays [P, B, cells...]"""
    return [np.ascontiguousarray(t[:, :, c]) for c in range(t.shape[2])]


def head_fwd_f32(x, patch, pool, layers):
    pooled = PR.patch_pool_fwd_f32(x, patch, pool)
    a = _channels(pooled)
    for W, b in layers:
        a = _layer_fwd(a, W, b)
    y = np.stack(a, axis=2)                          # [P, B, C_L, cells...]
    return pooled, y.reshape((-1,) + y.shape[2:])


def head_bwd(pooled, gy, layers):
    """Returns (d0 fp32 [P, B, C, cells...], grads): grads[k] = dict(w, w_abs, b, b_abs) of layer k (from 0), the parameter sums over all
    positions of the EXACT products (double)d[j] * (double)a[i] (and of (double)d[j]) taken in extended precision, and the sums of the
    terms' magnitudes, as float64 arrays.  b / b_abs are there for a layer without a bias too (the kernel does not write them)."""
    pooled = np.asarray(pooled, np.float32)
    P, B = pooled.shape[:2]
    acts = [_channels(pooled)]
    for W, b in layers[:-1]:
        acts.append(_layer_fwd(acts[-1], W, b))
    g = np.asarray(gy, np.float32).reshape((P, B) + gy.shape[1:])
    d = _channels(g)
    grads = [None] * len(layers)
    wide = np.longdouble
    for k in range(len(layers) - 1, -1, -1):
        W, _ = layers[k]
        a = acts[k]
        gw, gw_abs = np.zeros(W.shape), np.zeros(W.shape)
        gb, gb_abs = np.zeros(W.shape[0]), np.zeros(W.shape[0])
        for j in range(W.shape[0]):
            dj = d[j].astype(np.float64)
            gb[j], gb_abs[j] = float(dj.astype(wide).sum()), float(np.abs(dj).astype(wide).sum())
            for i in range(W.shape[1]):
                term = dj * a[i].astype(np.float64)                  # exact: 24 x 24 bits
                gw[j, i], gw_abs[j, i] = float(term.astype(wide).sum()), float(np.abs(term).astype(wide).sum())
        grads[k] = dict(w=gw, w_abs=gw_abs, b=gb, b_abs=gb_abs)
        prev = []
        for i in range(W.shape[1]):
            acc = np.zeros(d[0].shape, np.float32)
            for j in range(W.shape[0]):
                prod = W[j, i] * d[j]
                acc = acc + prod
            assert acc.dtype == np.float32
            prev.append(acc)
        d = prev
    return np.stack(d, axis=2), grads
