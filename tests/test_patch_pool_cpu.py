"""The numpy restatements of the patch-pooling kernels (tests/patch_pool_refs.py) against the tensor library's adaptive pooling and
its autograd at float64, in stage1.patch_heads' own patch order; the fp32 statements against the float64 ones within derived bounds;
the --patch_heads flag and the ISD / ISD_3d constructor keyword.  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import patch_pool_refs as R        # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32


def _torch_patches(x, patch, pool):
    """The fallback body of stage1.patch_heads without the pointwise layers: one adaptive pooling per patch, its loop order."""
    nd = x.dim() - 2
    fn = F.adaptive_avg_pool2d if nd == 2 else F.adaptive_avg_pool3d
    starts = [range(0, x.shape[2 + d] - patch + 1, patch // 2) for d in range(nd)]
    return torch.stack([fn(x[(slice(None), slice(None)) + tuple(slice(o, o + patch) for o in org)], pool)
                        for org in itertools.product(*starts)])


@pytest.mark.parametrize("patch,pool", [(20, 8), (5, 2), (4, 8), (10, 4), (16, 1), (4, 4), (16, 2), (7, 3), (64, 8), (3, 7)])
def test_windows_are_the_tensor_librarys(patch, pool):
    """A ramp and its squares pooled by adaptive_avg_pool1d: the two means fix a window's two ends."""
    win = R.windows(patch, pool)
    ramp = torch.arange(patch, dtype=torch.float64).reshape(1, 1, patch)
    m1 = F.adaptive_avg_pool1d(ramp, pool).reshape(-1).numpy()
    m2 = F.adaptive_avg_pool1d(ramp * ramp, pool).reshape(-1).numpy()
    for i, (lo, hi) in enumerate(win):
        assert 0 <= lo < hi <= patch
        r = np.arange(lo, hi, dtype=np.float64)
        np.testing.assert_allclose([m1[i], m2[i]], [r.mean(), (r * r).mean()], rtol=1e-13)
    if (patch, pool) == (20, 8):
        assert win == [(0, 3), (2, 5), (5, 8), (7, 10), (10, 13), (12, 15), (15, 18), (17, 20)]


@pytest.fixture(scope="module", params=list(range(len(R.CASES))), ids=R.CASE_IDS)
def case(request):
    c = R.CASES[request.param]
    x, gy = R.case_input(c)
    n, patch, pool = c[:3]
    return dict(c=c, x=x, gy=gy, fwd64=R.patch_pool_fwd_ref64(x, patch, pool), bwd64=R.patch_pool_bwd_ref64(gy, n, patch, pool))


def test_fwd_ref64_is_the_torch_patch_loop(case):
    n, patch, pool, B, C = case["c"]
    want = _torch_patches(torch.from_numpy(case["x"]).double(), patch, pool).numpy()
    assert case["fwd64"].shape == want.shape == case["gy"].shape
    np.testing.assert_allclose(case["fwd64"], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_fwd_f32_within_bound_of_ref64(case):
    """A sequential fp32 sum of m terms and one division: |error| <= (m + 1) * 2^-24 * mean|x| over the window."""
    n, patch, pool, B, C = case["c"]
    got = R.patch_pool_fwd_f32(case["x"], patch, pool)
    assert got.dtype == np.float32
    mean_abs = R.patch_pool_fwd_ref64(np.abs(case["x"]), patch, pool)
    lens = np.array([hi - lo for lo, hi in R.windows(patch, pool)])
    m = lens
    for _ in range(len(n) - 1):
        m = np.multiply.outer(m, lens)
    err = np.abs(got.astype(np.float64) - case["fwd64"])
    bound = (m + 1) * U * mean_abs
    print("fwd f32 error / bound, max:", float((err / bound).max()))
    assert (err <= bound).all()


def test_bwd_ref64_is_float64_autograd(case):
    n, patch, pool, B, C = case["c"]
    x = torch.from_numpy(case["x"]).double().requires_grad_(True)
    (_torch_patches(x, patch, pool) * torch.from_numpy(case["gy"]).double()).sum().backward()
    want = x.grad.numpy()
    np.testing.assert_allclose(case["bwd64"], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_bwd_f32_within_bound_of_ref64_and_zero_where_uncovered(case):
    """t divisions and t - 1 additions per voxel: |error| <= (t + 1) * 2^-24 * sum|term|.  No covering patch: exactly 0."""
    n, patch, pool, B, C = case["c"]
    got, mag, terms = R.patch_pool_bwd_f32(case["gy"], n, patch, pool)
    assert got.dtype == np.float32 and got.shape == case["x"].shape
    err = np.abs(got.astype(np.float64) - case["bwd64"])
    bound = (terms + 1) * U * mag
    print("bwd f32 error / bound, max:", float((err[:, :, terms > 0] / bound[:, :, terms > 0]).max()), "terms up to", int(terms.max()))
    assert (err <= bound).all()
    covered = np.zeros(tuple(n), bool)
    for org in itertools.product(*[R.starts(s, patch) for s in n]):
        covered[tuple(slice(o, o + patch) for o in org)] = True
    assert ((terms > 0) == covered).all()
    assert (got[:, :, ~covered] == 0).all() and (case["bwd64"][:, :, ~covered] == 0).all()
    if n == (14, 12, 10):
        assert not covered[13].any() and covered[:13, :11, :9].all()         # the tail behind the last patch, here on every axis
        assert terms.max() == 64             # three patches per axis meet at coordinate 4: cells 1 / 0, 1 / 0 of them, 4 tuples an axis


def test_patch_heads_flag():
    from arco_amd import pretrain_2D as P2, pretrain_3D as P3
    for mod in (P2, P3):
        assert mod.build_parser().parse_args([]).patch_heads == "torch"
        assert mod.build_parser().parse_args(["--patch_heads", "gpu"]).patch_heads == "gpu"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--patch_heads", "hip"])


def test_patch_heads_constructor_keyword():
    from arco_amd.model_2D import ISD
    from arco_amd.model_3D import ISD_3d
    for cls in (ISD, ISD_3d):
        with pytest.raises(ValueError, match="patch_heads"):
            cls(K=4, num_classes=2, patch_heads="hip")
