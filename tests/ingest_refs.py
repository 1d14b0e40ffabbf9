"""Pure-numpy reference of the GPU ingest (arco_amd/csrc/ingest.hip) and the cases its CPU and GPU tests share.

`apply_slice_descriptor` / `apply_volume_descriptor` implement the coordinate rule the kernels are held to, in float64 numpy
(element-wise ufuncs: every product and sum rounded on its own, no fused multiply-add):

  zoom, per axis:  cc = j * z with z = (n_in - 1) / (n_out - 1);  the constant 0 when cc < 0 or cc > n_in - 1, else floor(cc + 0.5)
  rotate:          cc_h = (off[h] + i * m[h][0]) + j * m[h][1], same range rule, same floor(cc + 0.5)

tests/test_gpu_ingest_cpu.py holds them to the real host transforms (scipy), tests/test_gpu_ingest_gpu.py holds the kernels to them."""
import functools

import numpy as np

import fixture_inputs as fx

SLICE_SOURCES = [(40, 36), (33, 47), (5, 256), (216, 256)]
SLICE_PATCHES = [(32, 32), (256, 256)]
ANGLES = list(range(-20, 20))                         # every value np.random.randint(-20, 20) can draw
ROT_FLIPS = [(k, axis) for k in range(4) for axis in range(2)]
CROP_PATCHES = [(300, 320), (200, 180), (32, 32), (200, 300), (258, 100)]   # zoomed shapes above, below and astride random_crop's 256
VOLUME_SOURCES = [(40, 38, 36), (30, 40, 36)]         # at patch 32^3 the second takes RandomCrop's pad path (30 <= 32)
VOLUME_PATCH = (32, 32, 32)


def _nearest(cc, n):
    ok = (cc >= 0.0) & (cc <= float(n - 1))
    return ok, np.where(ok, np.floor(cc + 0.5), 0.0).astype(np.int64)


def _unrotflip(k, axis, R, N, r, c):
    """Source position (u, v) in an array of shape N of element (r, c) of flip(rot90(a, k), axis), whose shape is R."""
    if axis == 0:
        r = R[0] - 1 - r
    else:
        c = R[1] - 1 - c
    k = k % 4
    if k == 0:
        return r, c
    if k == 1:
        return c, N[1] - 1 - r
    if k == 2:
        return N[0] - 1 - r, N[1] - 1 - c
    return N[0] - 1 - c, r


def apply_slice_descriptor(image, label, d, out_shape):
    """(image float32 [H, W], label int64 [H, W]) of the float64 descriptor row `d` on the stored slice (image, label)."""
    H, W = out_shape
    n0, n1 = image.shape
    op, Z0, Z1, z0, z1 = int(d[1]), int(d[2]), int(d[3]), d[4], d[5]
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok = np.ones((H, W), dtype=bool)
    u, v = i, j
    if op == 1:
        u, v = _unrotflip(int(d[6]), int(d[7]), (H, W), (Z0, Z1), i, j)
    elif op == 2:
        fi, fj = i.astype(np.float64), j.astype(np.float64)
        ok0, u = _nearest((d[12] + fi * d[8]) + fj * d[9], Z0)
        ok1, v = _nearest((d[13] + fi * d[10]) + fj * d[11], Z1)
        ok = ok0 & ok1
    elif op == 3:
        u, v = i + int(d[6]), j + int(d[7])
    ok = ok & (u >= 0) & (u < Z0) & (v >= 0) & (v < Z1)
    ok0, su = _nearest(u.astype(np.float64) * z0, n0)
    ok1, sv = _nearest(v.astype(np.float64) * z1, n1)
    ok = ok & ok0 & ok1
    su, sv = np.where(ok, su, 0), np.where(ok, sv, 0)
    img = np.where(ok, image.astype(np.float32)[su, sv], np.float32(0))
    lab = np.where(ok, label.astype(np.uint8)[su, sv], 0).astype(np.int64)
    return img.astype(np.float32), lab


def apply_volume_descriptor(image, label, d, patch):
    """(image float32 [X, Y, Z], label int64 [X, Y, Z]) of the int64 descriptor row `d` on the stored volume."""
    n = image.shape
    k, axis = int(d[1]), int(d[2])
    R = (n[1], n[0]) if k % 2 else (n[0], n[1])
    x, y, z = np.meshgrid(*(np.arange(p) for p in patch), indexing="ij")
    r, c, zz = x + int(d[3]), y + int(d[4]), z + int(d[5])
    ok = (r >= 0) & (r < R[0]) & (c >= 0) & (c < R[1]) & (zz >= 0) & (zz < n[2])
    u, v = _unrotflip(k, axis, R, n[:2], r, c)
    u, v, zz = np.where(ok, u, 0), np.where(ok, v, 0), np.where(ok, zz, 0)
    img = np.where(ok, image.astype(np.float32)[u, v, zz], np.float32(0)).astype(np.float32)
    lab = np.where(ok, label.astype(np.uint8)[u, v, zz], 0).astype(np.int64)
    return img, lab


@functools.lru_cache(maxsize=None)
def slice_sources():
    return [fx.ingest_slice(700 + s, shape) for s, shape in enumerate(SLICE_SOURCES)]


@functools.lru_cache(maxsize=None)
def volume_sources():
    return [fx.ingest_volume(70 + s, shape) for s, shape in enumerate(VOLUME_SOURCES)]


def slice_cases(patch):
    """Every (source, op, draws) of the 2-D checks at `patch`: dicts {src, op, draws} - no op, the 8 (k, axis), the 40 angles,
    the crop.  On a non-square patch an odd k would not collate; the patches here are square."""
    cases = []
    for src in range(len(SLICE_SOURCES)):
        cases.append(dict(src=src, op=0, draws={}))
        cases += [dict(src=src, op=1, draws=dict(k=k, axis=axis)) for k, axis in ROT_FLIPS]
        cases += [dict(src=src, op=2, draws=dict(angle=a)) for a in ANGLES]
        if tuple(patch) == (256, 256):                 # random_crop returns 256 x 256 whatever the patch
            cases.append(dict(src=src, op=3, draws={}))
    return cases


def crop_cases():
    """random_crop on zoomed shapes other than 256 x 256: always a 256 x 256 output (no batch of another patch size could hold it)."""
    return [dict(src=src, op=3, draws={}, patch=p) for src in range(len(SLICE_SOURCES)) for p in CROP_PATCHES]


def volume_cases():
    """(source, k, axis, crop window start): the 8 (k, axis) on both sources with the windows at both ends and inside."""
    from arco_amd.dataloaders.gpu_ingest import padded_shape
    rs = np.random.RandomState(11)
    cases = []
    for src, shape in enumerate(VOLUME_SOURCES):
        for k, axis in ROT_FLIPS:
            pads, padded = padded_shape(shape, VOLUME_PATCH, k)
            hi = [padded[a] - VOLUME_PATCH[a] for a in range(3)]              # randint(0, hi): 0 .. hi - 1
            for start in ((0, 0, 0), tuple(h - 1 for h in hi), tuple(int(rs.randint(0, h)) for h in hi)):
                cases.append(dict(src=src, k=k, axis=axis, start=start, pads=pads))
    return cases


@functools.lru_cache(maxsize=None)
def slice_batch(kind):
    """(float64 descriptor rows [B, 16], reference images [B, 1, H, W], reference labels [B, H, W]) of one launch: kind 32 / 256 =
    slice_cases at that patch (256 mixes all four branches), kind 'crop' = crop_cases (H = W = 256).  Computed once, read-only."""
    from arco_amd.dataloaders.gpu_ingest import slice_row
    cases = crop_cases() if kind == "crop" else slice_cases((kind, kind))
    rows, imgs, labs = [], [], []
    for c in cases:
        patch = c.get("patch", (kind, kind))
        d, out = slice_row(c["src"], SLICE_SOURCES[c["src"]], patch, c["op"], **c["draws"])
        img, lab = apply_slice_descriptor(*slice_sources()[c["src"]], d, out)
        rows.append(d); imgs.append(img[None]); labs.append(lab)
    out = np.stack(rows), np.stack(imgs), np.stack(labs)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def volume_batch():
    """(int64 descriptor rows [B, 8], reference images [B, 1, 32, 32, 32], reference labels [B, 32, 32, 32]) of volume_cases."""
    from arco_amd.dataloaders.gpu_ingest import volume_row
    rows, imgs, labs = [], [], []
    for c in volume_cases():
        d = volume_row(c["src"], c["pads"], c["k"], c["axis"], c["start"])
        img, lab = apply_volume_descriptor(*volume_sources()[c["src"]], d, VOLUME_PATCH)
        rows.append(d); imgs.append(img[None]); labs.append(lab)
    out = np.stack(rows), np.stack(imgs), np.stack(labs)
    for a in out:
        a.setflags(write=False)
    return out


class ForcedDraws:
    """Stand-ins for `random.random` and `np.random.randint` that hand out the given values in order (randint checks its bounds), so
    that a host transform takes a chosen branch with chosen parameters."""

    def __init__(self, randoms=(), ints=()):
        self.randoms, self.ints = list(randoms), list(ints)

    def random(self):
        return self.randoms.pop(0)

    def randint(self, lo, hi):
        v = self.ints.pop(0)
        assert lo <= v < hi, (lo, v, hi)
        return v

    def install(self, monkeypatch):
        import random
        monkeypatch.setattr(random, "random", self.random)
        monkeypatch.setattr(np.random, "randint", self.randint)
        return self


def slice_draws(op, draws):
    """The draws that send RandomGenerator down branch `op` with the parameters `draws`."""
    randoms = [0.75 if cand == op else 0.25 for cand in (1, 2, 3)][:op if op else 3]
    return ForcedDraws(randoms, [draws[k] for k in ("k", "axis", "angle") if k in draws])


def write_slice_dataset(tmp_path, n=30, shape=(40, 36)):
    """The ACDC-shaped tree of tests/test_ingest_gpu.py: n npz slices (patients_to_slices('ACDC', 1) = 23 of them labeled)."""
    import os
    root = tmp_path / "ACDC"
    os.makedirs(root / "data" / "slices")
    names = [f"patient{i:03d}_slice_{i}" for i in range(n)]
    for i, name in enumerate(names):
        img, lab = fx.ingest_slice(300 + i, shape)
        np.savez(root / "data" / "slices" / (name + ".npz"), image=img, label=lab)
    (root / "train_slices.list").write_text("\n".join(names) + "\n")
    return root


def write_volume_dataset(tmp_path, n=5, shape=(40, 38, 36)):
    """The LA-shaped tree of tests/test_ingest_gpu.py: n npz volumes."""
    import os
    base = tmp_path / "LA" / "2018LA_Seg_Training Set"
    cases = [f"case{i}" for i in range(n)]
    for i, c in enumerate(cases):
        os.makedirs(base / c)
        vol, lab = fx.ingest_volume(i, shape)
        np.savez(base / c / "mri_norm2.npz", image=vol, label=lab)
    (tmp_path / "LA" / "train.list").write_text("\n".join(cases) + "\n")
    return base
