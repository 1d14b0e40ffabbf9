"""References and cases for the zoom kernels (arco_amd/csrc/zoom.hip, arco_amd/utils/zoom_gpu.py).

ref_zoom restates scipy.ndimage.zoom(order=0, mode='constant') as the index rule the kernels implement: output index o of an axis of
n_in points resampled to n_out points reads input index floor(cc + 0.5), cc = o * z, z = (n_in - 1) / (n_out - 1), all in float64
with the product and the sum rounded separately (numpy does not fuse them), and is 0 where !(0 <= cc <= n_in - 1).
tests/test_zoom_kernels_cpu.py holds it to scipy on every case below, in both directions.

A case is (patch, (x, y)): the forward zoom takes [S, x, y] slices to the patch, the way back takes a [S, *patch] map to (x, y)."""
import numpy as np
import torch

CASES = [
    ((48, 64), (28, 47)),      # forward zeroes the last image row; the way back zeroes the last label column
    ((48, 48), (55, 58)),      # downsampling forward; zeroed last row and column forward
    ((64, 48), (127, 24)),     # 63 exact .5 ties of floor(cc + 0.5) on the way back; zeroed last column on the way back
    ((64, 64), (43, 78)),      # one axis up, one down; 21 ties
    ((32, 32), (16, 31)),      # last row and column both zeroed on the way back
    ((64, 64), (2, 3)),        # smallest legal axes
    ((64, 64), (64, 64)),      # identity
    ((24, 37), (19, 53)),      # three slices, fastest axes 37 and 53: the tail of the 16-byte stores and the slice stride
]
RAGGED = CASES[-1]
IDS = ["%dx%d_%dx%d" % (p + s) for p, s in CASES]


def slices(case):
    return 3 if case == RAGGED else 2


def axis_map(n_in, n_out):
    """(idx int64 [n_out], ok bool [n_out], ties): the input index every output index reads, whether it reads at all (else the
    constant 0), and how many of the reading ones sit on an exact .5 tie of floor(cc + 0.5)."""
    z = (n_in - 1) / (n_out - 1)
    cc = np.arange(n_out, dtype=np.float64) * z
    ok = (cc >= 0) & (cc <= n_in - 1)
    idx = np.where(ok, np.floor(cc + 0.5), 0).astype(np.int64)
    ties = int(np.sum(ok & (cc - np.floor(cc) == 0.5)))
    return idx, ok, ties


def ref_zoom(a, out_size):
    """zoom(order=0) of the last two axes of `a` to out_size, any leading axes; the dtype of `a`."""
    a = np.asarray(a)
    i0, ok0, _ = axis_map(a.shape[-2], out_size[0])
    i1, ok1, _ = axis_map(a.shape[-1], out_size[1])
    out = a[..., i0[:, None], i1[None, :]]
    return np.where(ok0[:, None] & ok1[None, :], out, np.zeros((), dtype=a.dtype)).astype(a.dtype)


def image(case, direction, seed=0):
    """float32 [S, n0, n1], nowhere 0 (a zeroed edge shows); direction 'fwd' has the slices' shape, 'back' the patch's."""
    patch, xy = case
    shape = (slices(case),) + (xy if direction == "fwd" else patch)
    rng = np.random.default_rng(seed + 17 * shape[1] + shape[2])
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def labels(case, direction, seed=0):
    """int64 [S, n0, n1] in 1..3."""
    patch, xy = case
    shape = (slices(case),) + (xy if direction == "fwd" else patch)
    return np.random.default_rng(seed + 31 * shape[1] + shape[2]).integers(1, 4, size=shape, dtype=np.int64)


def target(case, direction):
    patch, xy = case
    return patch if direction == "fwd" else xy


# ---- canary margins around an output ---------------------------------------------------------------------------------------------------
GUARD = 64                                   # sentinel elements before and after the output
SENT = {torch.float32: -12345.5, torch.int64: 0x5A5A5A5A5A5A5A5A}


def guarded(n, dtype, device):
    """(buffer of GUARD + n + GUARD sentinel elements, its middle n as a view): the kernels get the view."""
    buf = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    s = SENT[buf.dtype]
    return buf.numel() == n + 2 * GUARD and bool((buf[:GUARD] == s).all().item()) and bool((buf[GUARD + n:] == s).all().item())
