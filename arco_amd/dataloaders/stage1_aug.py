"""The student transform of stage-1 pre-training on the GPU (pretrain_2D / pretrain_3D --gpu_ingest 1; csrc/stage1_aug.hip).

The host classes - dataset_withAug.RandomColorJitter / RandomNoise (2-D) and la_heart.RandomColorJitter / RandomNoise (3-D) - run one
`jitter_gray_` per image (3-D: per X-Y slice of every volume, a `.mean()` and three or four elementwise launches each) and blur through
`augment.jitter_blur` (3-D: two permuted copies of every volume around it).  The twins here draw exactly what those classes draw, in
the same order - the numpy gate, per plane `_jitter_params` on the torch CPU generator, python's `random.uniform` for sigma - then upload
the per-plane records once and launch once (the in-place blur: twice).  They keep the aliasing of the host classes:

  GrayJitter            edits the shared image tensor in place and returns a new dict around it (student and teacher both see it)
  Noise, 2-D            returns a new dict with a NEW [B, H, W] tensor, byte / 255
  Noise, 3-D            edits the volume in place - the byte values 0 .. 255, the reference drops the /255 here - new dict, same tensor

`gray_jitter_planes` / `blur_planes` are the launches; a plane is image[j, 0] of [B, C, H, W] or image[j, 0, :, :, t] of [B, C, X, Y, Z]."""
import random

import numpy as np
import torch

from .. import _lib
from . import Compose
from . import dataset_withAug as A2
from . import la_heart as A3
from .dataset_withAug import _jitter_params

JIT_RECORD = np.dtype([("order", "<i4", 4), ("fb", "<f4"), ("fc", "<f4")])      # csrc/stage1_aug.hip: JitRecord


def jitter_records(params):
    """The record array of a list of `_jitter_params` results (order, factors), one per plane."""
    recs = np.zeros(len(params), dtype=JIT_RECORD)
    recs["order"] = [order for order, _ in params]
    recs["fb"], recs["fc"] = [fac[0] for _, fac in params], [fac[1] for _, fac in params]
    return recs


def _planes(image):
    """(elements from the tensor's first one to the end of its storage, B, T, H, W, strides s_img, s_t, s_row, s_col) of the planes of
    channel 0 of an fp32 device tensor [B, C, H, W] or [B, C, X, Y, Z]."""
    _lib.require_gpu(image)
    if image.dtype != torch.float32 or image.dim() not in (4, 5):
        raise ValueError(f"stage-1 transform on the GPU: images must be fp32 [B, C, H, W] or [B, C, X, Y, Z], got {image.dtype} {tuple(image.shape)}")
    st = image.stride()
    n_elems = image.untyped_storage().nbytes() // 4 - image.storage_offset()
    B, H, W = (int(image.shape[a]) for a in (0, 2, 3))
    T, s_t = (int(image.shape[4]), st[4]) if image.dim() == 5 else (1, 0)
    return n_elems, B, T, H, W, (st[0], s_t, st[2], st[3])


def gray_jitter_planes(image, recs):
    """jitter_gray_ on every plane of `image`, in place, one launch: recs = jitter_records(...) in plane order (j, t)."""
    n_elems, B, T, H, W, strides = _planes(image)
    if image.shape[1] != 1:
        raise ValueError(f"stage-1 transform on the GPU: the jitter is that of one-channel images, got {tuple(image.shape)}")
    assert recs.dtype == JIT_RECORD and len(recs) == B * T and _lib.query("arco_jit_record_bytes") == JIT_RECORD.itemsize
    dev = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(image.device)
    _lib.call("arco_gray_jitter_planes", _lib.ptr(image), n_elems, B * T, T, H, W, *strides, _lib.ptr(dev))
    return image


def blur_planes(image, sigma, inplace):
    """Pillow's GaussianBlur(sigma) of the 8-bit quantisation of every plane of `image`: a new [B * T, H, W] tensor of byte / 255
    (inplace=False), or the byte values stored back into `image` (inplace=True)."""
    from ..augment import _gaussian_blur_radius
    n_elems, B, T, H, W, strides = _planes(image)
    radius = _gaussian_blur_radius(sigma)
    if inplace:
        ws = torch.empty(_lib.query("arco_blur_planes_ws_bytes", B * T, T, H, W), dtype=torch.uint8, device=image.device)
        _lib.call("arco_blur_planes", _lib.ptr(image), n_elems, B * T, T, H, W, *strides, radius, None, _lib.ptr(ws))
        return image
    out = torch.empty((B * T, H, W), dtype=torch.float32, device=image.device)
    _lib.call("arco_blur_planes", _lib.ptr(image), n_elems, B * T, T, H, W, *strides, radius, _lib.ptr(out), None)
    return out


class GrayJitter(object):
    """Twin of RandomColorJitter, 2-D and 3-D: one `_jitter_params` draw per plane in the order (j, t), one launch."""

    def __init__(self, color, p):
        self.color, self.p = color, p

    def __call__(self, sample):
        if np.random.uniform(low=0, high=1, size=1) > self.p:
            return sample
        image, label = sample['image'], sample['label']
        n = int(image.shape[0]) * (int(image.shape[-1]) if image.dim() == 5 else 1)
        gray_jitter_planes(image, jitter_records([_jitter_params(self.color) for _ in range(n)]))
        return {'image': image, 'label': label}


class Noise(object):
    """Twin of RandomNoise: one sigma per call.  2-D (inplace=False): a new [B, H, W] tensor; 3-D (inplace=True): the volume itself."""

    def __init__(self, p, inplace):
        self.p, self.inplace = p, inplace

    def __call__(self, sample):
        if np.random.uniform(low=0, high=1, size=1) > self.p:
            return sample
        image, label = sample['image'], sample['label']
        sigma = random.uniform(0.15, 1.15)
        return {'image': blur_planes(image, sigma, self.inplace), 'label': label}


def device_transform(transform):
    """The device twin of a student transform (`make_transform_student` of either pre-trainer); a transform that has no twin is an
    error (no silent change of augmentation)."""
    ts = transform.transforms if isinstance(transform, Compose) else [transform]
    twins = []
    for t in ts:
        if type(t) in (A2.RandomColorJitter, A3.RandomColorJitter):
            twins.append(GrayJitter(t.color, t.p))
        elif type(t) in (A2.RandomNoise, A3.RandomNoise):
            twins.append(Noise(t.p, inplace=type(t) is A3.RandomNoise))
        else:
            raise ValueError(f"gpu ingest: no device twin for the student transform {type(t).__name__}")
    return Compose(twins)
