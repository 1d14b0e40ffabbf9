"""Numpy restatements of the two kernels of arco_amd/csrc/stage1_aug.hip and the cases their CPU and GPU tests share.

  jitter:  torchvision's tensor-mode ColorJitter on a one-channel fp32 plane, every operation rounded to fp32 on its own:
             op 0   x = clamp(fl32(x * fb), 0, 1)
             op 1   x = clamp(fl32(fl32(x * fc) + s), 0, 1),  s = fl32(fl32(1 - fc) * mean), 1 - fc taken in double and rounded once,
                    mean = np.float32(np.sum(plane, dtype=np.float64) / n) of the plane as it stands when the op runs
             op 2, 3  nothing
  blur:    arco_oracle.gaussian_blur_u8(arco_oracle.q8(plane), sigma) - Pillow's integer arithmetic, held to Pillow itself by
           tests/test_pretrain_ingest_cpu.py

The kernel sums a plane in float64 in an order of its own (a fixed one).  `plane_mean` therefore ASSERTS that the plane's float64 sum
taken forward, taken over the sorted values and taken pairwise (np.sum) rounds to the same fp32 mean: a condition on the test inputs,
not a tolerance - with it any summation order gives the restatement's bits."""
import functools
import itertools

import numpy as np

import arco_oracle as orc

F = np.float32
SIGMAS = (0.15, 0.5, 0.7, 1.15)                                      # the ends of random.uniform(0.15, 1.15) and two sigmas inside
ORDERS = [list(p) for p in itertools.permutations(range(4))]         # the 24 results of torch.randperm(4)
FACTOR_SETS = {"fb_one": (1.0, 0.85), "fc_one": (1.15, 1.0), "both": (0.9, 1.1)}
SHAPES_2D = [(3, 1, 40, 36), (2, 1, 33, 47), (1, 1, 256, 256)]
SHAPES_3D = [(2, 1, 24, 20, 5), (1, 1, 32, 32, 33)]                  # T = 33: no lane grouping divides it
BLUR_PLANES = [(33, 47), (70, 36), (40, 38)]                         # larger than one tile either way: tile borders inside the image
BLUR_T = (5, 17)


def plane_mean(plane):
    v = np.asarray(plane, F).ravel().astype(np.float64)
    n = v.size
    mean = F(np.sum(v) / n)
    forward, ascending = F(np.cumsum(v)[-1] / n), F(np.cumsum(np.sort(v))[-1] / n)
    assert mean == forward == ascending, "test input: the fp32 mean of this plane depends on the order of the float64 sum"
    return mean


def jitter_plane(plane, order, fb, fc, mean_fn=plane_mean):
    """The jitter of one plane; returns a new fp32 array."""
    x = np.asarray(plane, F).copy()
    fb, fc = F(fb), F(fc)
    for op in order:
        if op == 0:
            x = np.clip(x * fb, F(0), F(1))
        elif op == 1:
            s = F(F(1.0 - float(fc)) * mean_fn(x))
            x = np.clip((x * fc).astype(F) + s, F(0), F(1))
    assert x.dtype == F
    return x


def plane_views(image):
    """The planes of channel 0 of an array [B, C, H, W] or [B, C, X, Y, Z] in record order (j, t), as views."""
    if image.ndim == 4:
        return [image[j, 0] for j in range(image.shape[0])]
    return [image[j, 0, :, :, t] for j in range(image.shape[0]) for t in range(image.shape[4])]


def jitter_image(image, params):
    """jitter_plane on every plane of a copy of `image`; params: one (order, (fb, fc, ...)) per plane, `_jitter_params`' result."""
    out = np.array(image, dtype=F, copy=True)
    views = plane_views(out)
    assert len(views) == len(params)
    for v, (order, fac) in zip(views, params):
        v[...] = jitter_plane(v, order, fac[0], fac[1])
    return out


def blur_planes(planes, sigma):
    """uint8 [N, H, W]: the blurred 8-bit quantisation of fp32 planes [N, H, W]."""
    return orc.gaussian_blur_u8(orc.q8(np.asarray(planes, F)), sigma)


def blur_image(image, sigma):
    """uint8 [B * T, H, W] in record order: the blur of every plane of `image`."""
    return blur_planes(np.stack(plane_views(np.asarray(image, F))), sigma)


def jitter_input(shape, seed):
    """fp32 `shape`, uniform in [-0.1, 1.2): values inside and outside [0, 1]."""
    rs = np.random.RandomState(seed)
    return (rs.rand(*shape) * 1.3 - 0.1).astype(F)


def spread_params(n_planes, factors, start=0):
    """(order, (fb, fc, 1, 0)) per plane: the 24 orders dealt round over the planes, from order `start` on."""
    return [(ORDERS[(start + p) % 24], (factors[0], factors[1], 1.0, 0.0)) for p in range(n_planes)]


def n_planes(shape):
    return shape[0] * (shape[4] if len(shape) == 5 else 1)


def case_starts(shape):
    """The launches of one (shape, factor set): as many as it takes to deal all 24 orders over the shape's planes."""
    return list(range(0, 24, n_planes(shape)))


@functools.lru_cache(maxsize=None)
def jitter_case(shape, kind, start):
    """(input, params, expected) of one launch, computed once and read-only."""
    x = jitter_input(shape, sum(shape) + start)
    params = spread_params(n_planes(shape), FACTOR_SETS[kind], start)
    want = jitter_image(x, params)
    for a in (x, want):
        a.setflags(write=False)
    return x, params, want


def seed_all(s):
    import random
    import torch
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def rng_states():
    import random
    import torch
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def assert_same_states(a, b):
    import torch
    assert a[0] == b[0]
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]
    assert torch.equal(a[2], b[2])
