"""Data ingest from a GPU-resident dataset (both trainers' --gpu_ingest 1; csrc/ingest.hip).

The host path of --synthetic 0 reads every sample from disk and runs scipy on it, one host thread, per step.  Every transform on
it is nearest-neighbour or an index map, and none of its random draws looks at pixel data.  So:

  * `GpuBank` holds a whole dataset in device memory - one packed fp32 buffer of images, one packed uint8 buffer of labels, an
    int64 table {offset, n0, n1, n2} per case - read once, with the dataset's transform switched off;
  * `SliceDescriptors` / `VolumeDescriptors` are twins of the dataset objects of `build_loaders`: their `__getitem__` consumes
    python's `random` and numpy's global RandomState exactly as `RandomGenerator` / `RandomRotFlip` + `RandomCrop` do (same
    calls, same order) and returns the case index plus the drawn parameters, a row of 16 float64 / 8 int64;
  * `stepper.paired_loaders` wraps them as it wraps the host datasets (the samplers, the loaders' base-seed draws and the doubling
    of the labeled set are the same code), and `GpuBank.slices` / `.volumes` turn a collated batch of rows into the batch the host path would
    have produced, bit for bit, with one kernel launch;
  * `bank_loader` does the same for the pre-trainers' single loader over a TwoStreamBatchSampler (pretrain_2D / pretrain_3D).

Casting at upload changes nothing: nearest resampling and zero fill commute with astype(float32) / astype(uint8)."""
import random

import numpy as np
import torch
from scipy import special
from torch.utils.data import ConcatDataset, Dataset

from .. import _lib
from . import Compose
from .dataset import RandomGenerator
from .la_heart import RandomCrop, RandomRotFlip, ToTensor

SLICE_DESC, VOLUME_DESC, TABLE = 16, 8, 4          # csrc/ingest.hip: INGEST_SLICE_DESC, INGEST_VOLUME_DESC, INGEST_TABLE
OP_NONE, OP_ROT_FLIP, OP_ROTATE, OP_CROP = 0, 1, 2, 3
CROP = 256                                          # dataset.random_crop's hard-wired output size


def zoomed_size(n_in, patch):
    """Length scipy.ndimage.zoom(a, patch / n_in) gives an axis of n_in points, and its coordinate step (n_in - 1) / (n_out - 1)."""
    n_out = int(round(n_in * (patch / n_in)))
    if n_out < 2:
        raise ValueError(f"gpu ingest: a zoomed axis of {n_out} point(s) is not supported")
    return n_out, (n_in - 1) / (n_out - 1)


def rotate_params(angle, shape):
    """The matrix and the offset scipy.ndimage.rotate(a, angle, reshape=False) hands to affine_transform for an `a` of `shape`: the
    same calls on the same values (scipy/ndimage/_interpolation.py), so the same float64 bits."""
    c, s = special.cosdg(angle), special.sindg(angle)
    m = np.array([[c, s], [-s, c]])
    plane = np.asarray(shape)
    out_center = m @ ((plane - 1) / 2)
    in_center = (plane - 1) / 2
    return m, in_center - out_center


def crop_window(zoomed):
    """dataset.random_crop on an array of shape `zoomed`: ((row shift, column shift), output shape) with shift = window start
    minus pad, so that out[i, j] = a[i + shift0, j + shift1] inside `a` and 0 outside."""
    Z0, Z1 = zoomed
    p0 = p1 = 0
    if Z0 <= CROP or Z1 <= CROP:
        p0, p1 = max((CROP - Z0) // 2 + 3, 0), max((CROP - Z1) // 2 + 3, 0)
    w, h = Z0 + 2 * p0, Z1 + 2 * p1
    w1, h1 = int(round((w - CROP) / 2.)), int(round((h - CROP) / 2.))
    return (w1 - p0, h1 - p1), (min(CROP, w - w1), min(CROP, h - h1))


def slice_row(idx, shape, patch_size, op, k=0, axis=0, angle=0):
    """(the float64 row of csrc/ingest.hip's SliceDesc, the shape of the transformed sample) for case `idx` of `shape` zoomed to
    `patch_size` and then put through `op` with the drawn k / axis (OP_ROT_FLIP) or angle (OP_ROTATE)."""
    (Z0, z0), (Z1, z1) = zoomed_size(shape[0], patch_size[0]), zoomed_size(shape[1], patch_size[1])
    d = np.zeros(SLICE_DESC, dtype=np.float64)
    d[:6] = idx, op, Z0, Z1, z0, z1
    out = (Z0, Z1)
    if op == OP_ROT_FLIP:
        d[6:8] = k, axis
        out = (Z1, Z0) if k % 2 else (Z0, Z1)
    elif op == OP_ROTATE:
        m, off = rotate_params(angle, (Z0, Z1))
        d[8:12], d[12:14] = m.ravel(), off
    elif op == OP_CROP:
        d[6:8], out = crop_window((Z0, Z1))
    return d, out


class SliceDescriptors(Dataset):
    """Twin of a slice dataset whose transform is Compose([RandomGenerator(patch)]): draws what RandomGenerator draws, returns
    {'idx', 'desc'} with desc the row of `slice_row`."""

    def __init__(self, shapes, patch_size):
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.patch_size = (int(patch_size[0]), int(patch_size[1]))

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, idx):
        op, draws = OP_NONE, {}
        for cand in (OP_ROT_FLIP, OP_ROTATE, OP_CROP):        # RandomGenerator.__call__'s cascade
            if random.random() > 0.5:
                op = cand
                if op == OP_ROT_FLIP:                           # random_rot_flip
                    draws = dict(k=np.random.randint(0, 4), axis=np.random.randint(0, 2))
                elif op == OP_ROTATE:                           # random_rotate (random_crop draws nothing: a centre crop)
                    draws = dict(angle=np.random.randint(-20, 20))
                break
        d, out = slice_row(idx, self.shapes[idx], self.patch_size, op, **draws)
        if out != self.patch_size:
            # the host path hands such a sample to a collate that cannot stack it with the others (odd k on a non-square patch, the
            # 256-hard-wired crop at another patch size)
            raise RuntimeError(f"gpu ingest: a sample of shape {out} cannot be collated into a batch of patch {self.patch_size} "
                               f"(op {op}); the host path fails on it as well")
        return {'idx': idx, 'desc': torch.from_numpy(d)}


def padded_shape(shape, patch_size, k):
    """(pads, shape after RandomRotFlip's k quarter turns and RandomCrop's zero pad) of a volume of `shape`."""
    r = (shape[1], shape[0], shape[2]) if k % 2 else tuple(shape)
    pads = (0, 0, 0)
    if any(r[a] <= patch_size[a] for a in range(3)):
        pads = tuple(max((patch_size[a] - r[a]) // 2 + 3, 0) for a in range(3))
    return pads, tuple(r[a] + 2 * pads[a] for a in range(3))


def volume_row(idx, pads, k, axis, start):
    """The int64 row {case, k, axis, s0, s1, s2, 0, 0} of csrc/ingest.hip: s = crop window start minus pad."""
    return np.array([idx, k, axis] + [start[a] - pads[a] for a in range(3)] + [0, 0], dtype=np.int64)


class VolumeDescriptors(Dataset):
    """Twin of a volume dataset whose transform is Compose([RandomRotFlip(), RandomCrop(patch), ToTensor()]): the same five
    np.random.randint draws; returns {'idx', 'desc'} with desc the row of `volume_row`."""

    def __init__(self, shapes, patch_size):
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.patch_size = tuple(int(v) for v in patch_size)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, idx):
        o = self.patch_size
        k = np.random.randint(0, 4)                             # RandomRotFlip
        axis = np.random.randint(0, 2)
        pads, (w, h, d) = padded_shape(self.shapes[idx], o, k)  # RandomCrop
        w1 = np.random.randint(0, w - o[0])
        h1 = np.random.randint(0, h - o[1])
        d1 = np.random.randint(0, d - o[2])
        return {'idx': idx, 'desc': torch.from_numpy(volume_row(idx, pads, k, axis, (w1, h1, d1)))}


class GpuBank:
    """A dataset's cases packed in device memory: `img` fp32 and `lab` uint8 (one element per pixel / voxel, case after case), `table`
    int64 [n_cases, 4] = {offset in elements, n0, n1, n2 (1 for slices)} on the host, `table_dev` its device copy."""

    def __init__(self, images, labels, device):
        images, labels = list(images), list(labels)
        if not images or len(images) != len(labels):
            raise ValueError("gpu ingest: a bank needs at least one case, and one label array per image")
        ranks = {np.ndim(a) for a in images} | {np.ndim(a) for a in labels}
        if len(ranks) != 1 or ranks.pop() not in (2, 3):
            raise ValueError("gpu ingest: the cases of one dataset must all be 2-D slices or all be 3-D volumes")
        self.rank = np.ndim(images[0])
        table = np.ones((len(images), TABLE), dtype=np.int64)
        off = 0
        for i, (im, lb) in enumerate(zip(images, labels)):
            if np.shape(im) != np.shape(lb) or min(np.shape(im)) < 1:
                raise ValueError(f"gpu ingest: case {i}: image {np.shape(im)} and label {np.shape(lb)} must have one non-empty shape")
            lb = np.asarray(lb)
            if lb.size and (lb.min() < 0 or lb.max() > 255):
                raise ValueError(f"gpu ingest: case {i}: label values {lb.min()} .. {lb.max()} do not fit the bank's uint8 labels (0 .. 255)")
            table[i, 0], table[i, 1:1 + self.rank] = off, np.shape(im)
            off += int(np.prod(np.shape(im)))
        self.table = table
        self.n_cases, self.elems = len(images), off
        self.shapes = [tuple(int(v) for v in row[1:1 + self.rank]) for row in table]
        self.device = torch.device(device)
        self.img = torch.from_numpy(np.concatenate([np.asarray(a).astype(np.float32).ravel() for a in images])).to(self.device)
        self.lab = torch.from_numpy(np.concatenate([np.asarray(a).astype(np.uint8).ravel() for a in labels])).to(self.device)
        self.table_dev = torch.from_numpy(table).to(self.device)
        _lib.require_gpu(self.img, self.lab, self.table_dev)

    @classmethod
    def from_dataset(cls, ds, device):
        """Read every case of `ds` once, untransformed (only `__len__` and `__getitem__` are used)."""
        transform, ds.transform = ds.transform, None
        try:
            samples = [ds[i] for i in range(len(ds))]
        finally:
            ds.transform = transform
        return cls([s['image'] for s in samples], [s['label'] for s in samples], device)

    @property
    def nbytes(self):
        return self.elems * 5 + self.table.nbytes

    def descriptors(self, transform):
        """The descriptor twin of a dataset of this bank's cases whose transform is `transform`; a transform that has no twin is an
        error (no silent change of augmentation)."""
        ts = transform.transforms if isinstance(transform, Compose) else [transform]
        kinds = [type(t) for t in ts]
        if self.rank == 2 and kinds == [RandomGenerator]:
            return SliceDescriptors(self.shapes, ts[0].output_size)
        if self.rank == 3 and kinds == [RandomRotFlip, RandomCrop, ToTensor]:
            return VolumeDescriptors(self.shapes, ts[1].output_size)
        raise ValueError(f"gpu ingest: no descriptor twin for the transform {[k.__name__ for k in kinds]} on rank-{self.rank} cases")

    def _check(self, desc, width, dtype):
        if desc.dim() != 2 or desc.shape[1] != width or desc.dtype != dtype or desc.shape[0] < 1:
            raise ValueError(f"gpu ingest: descriptors must be [B, {width}] {dtype}, got {tuple(desc.shape)} {desc.dtype}")
        cases = desc[:, 0]
        if not desc.is_cuda and (cases.min() < 0 or cases.max() >= self.n_cases):
            raise ValueError("gpu ingest: a descriptor names a case outside the bank")
        return desc.to(self.device, non_blocking=True).contiguous()

    def slices(self, desc, patch_size, labels=True):
        """image fp32 [B, 1, H, W], label int64 [B, H, W] (None with labels=False) for the [B, 16] float64 descriptors `desc`."""
        if self.rank != 2:
            raise ValueError("gpu ingest: slices() needs a bank of 2-D cases")
        d = self._check(desc, SLICE_DESC, torch.float64)
        B, (H, W) = int(d.shape[0]), (int(v) for v in patch_size)
        img = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        lab = torch.empty((B, H, W), dtype=torch.int64, device=self.device) if labels else None
        _lib.call("arco_ingest_slices", _lib.ptr(self.img), _lib.ptr(self.lab), self.elems, _lib.ptr(self.table_dev), self.n_cases,
                  _lib.ptr(d), B, H, W, _lib.ptr(img), _lib.ptr(lab))
        return img, lab

    def volumes(self, desc, patch_size, labels=True):
        """image fp32 [B, 1, X, Y, Z], label int64 [B, X, Y, Z] (None with labels=False) for the [B, 8] int64 descriptors `desc`."""
        if self.rank != 3:
            raise ValueError("gpu ingest: volumes() needs a bank of 3-D cases")
        d = self._check(desc, VOLUME_DESC, torch.int64)
        B, (X, Y, Z) = int(d.shape[0]), (int(v) for v in patch_size)
        img = torch.empty((B, 1, X, Y, Z), dtype=torch.float32, device=self.device)
        lab = torch.empty((B, X, Y, Z), dtype=torch.int64, device=self.device) if labels else None
        _lib.call("arco_ingest_volumes", _lib.ptr(self.img), _lib.ptr(self.lab), self.elems, _lib.ptr(self.table_dev), self.n_cases,
                  _lib.ptr(d), B, X, Y, Z, _lib.ptr(img), _lib.ptr(lab))
        return img, lab


class BankLoader:
    """A descriptor DataLoader with its bank: iterating yields {'image', 'label', 'idx'} batches on the device, one launch each."""

    def __init__(self, loader, bank, patch_size, labels=True):
        self.loader, self.bank, self.patch_size, self.labels = loader, bank, tuple(int(v) for v in patch_size), labels
        self.dataset = loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        return self._batches(iter(self.loader))     # the loader's iterator is made HERE, as the host path's is: it draws the base seed

    def _batches(self, it):
        make = self.bank.slices if self.bank.rank == 2 else self.bank.volumes
        for batch in it:
            img, lab = make(batch['desc'], self.patch_size, self.labels)
            yield {'image': img, 'label': lab, 'idx': batch['idx']}


def _base(ds):
    while isinstance(ds, ConcatDataset):            # paired_loaders doubles the labeled set: ConcatDataset([ds, ds]), nested
        ds = ds.datasets[0]
    return ds


def bank_loaders(host_loaders, paired_loaders, batch_size, device, generator=None, unlabeled_labels=False):
    """The two loaders of --gpu_ingest 1 from the two host loaders `build_loaders` made: a bank per stream from each loader's
    dataset, the descriptor twins of those datasets, and `paired_loaders` around the twins as it is around the originals.  The
    unlabeled stream's labels are never read by a step, so its batches carry none unless asked for.  Returns the (labeled,
    unlabeled) BankLoaders."""
    sets = [_base(ld.dataset) for ld in host_loaders]
    banks = [GpuBank.from_dataset(ds, device) for ds in sets]
    twins = [bank.descriptors(ds.transform) for bank, ds in zip(banks, sets)]
    loaders = paired_loaders(*twins, batch_size, generator)
    return tuple(BankLoader(ld, bank, tw.patch_size, labels=lab) for ld, bank, tw, lab in zip(loaders, banks, twins, (True, unlabeled_labels)))


def bank_loader(host_loader, device):
    """The loader of --gpu_ingest 1 for the pre-trainers' shape - ONE host loader over the whole list with
    batch_sampler=TwoStreamBatchSampler: a bank of the loader's dataset, the descriptor twin of that dataset and the SAME sampler object
    around the twin.  Every sample of a batch may be a labeled one, so the batches always carry labels."""
    from torch.utils.data import DataLoader
    ds = host_loader.dataset
    bank = GpuBank.from_dataset(ds, device)
    twin = bank.descriptors(ds.transform)
    loader = DataLoader(twin, batch_sampler=host_loader.batch_sampler, num_workers=0, pin_memory=host_loader.pin_memory)
    return BankLoader(loader, bank, twin.patch_size, labels=True)
