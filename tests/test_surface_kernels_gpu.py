"""Surface-distance kernels (arco_amd/csrc/surface.hip) on the GPU against the scipy reference of tests/surface_kernel_refs.py (which
tests/test_surface_kernels_cpu.py holds to the brute-force restatement): the histograms are integer counts, so every check is exact;
hd95 finished from them equals the host route's (==), asd to rtol 1e-12 (the order of one float64 sum)."""
import numpy as np
import pytest
import torch

import surface_kernel_refs as R
from arco_amd.utils import metrics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


@pytest.mark.parametrize("name", R.CASES)
def test_histograms_exact_and_guards_intact(L, name):
    from arco_amd.utils import surface_gpu
    c = R.case(name)
    got, hist_buf, n_hist, ws_buf, n_ws = R.run_guarded(L, c)
    assert R.guards_intact(hist_buf, n_hist) and R.guards_intact(ws_buf, n_ws)
    assert R.exact(got, c["ref"])
    p, g = R.device_maps(c)
    first = surface_gpu.surface_histograms(p, g, c["classes"])
    assert first.is_cuda and first.dtype == torch.int64 and tuple(first.shape) == c["ref"].shape
    assert R.exact(first, c["ref"])
    assert torch.equal(surface_gpu.surface_histograms(p, g, c["classes"]), first)      # a second call: the identical tensor
    assert torch.equal(surface_gpu.surface_histograms(p.to(torch.int32), g.to(torch.uint8), c["classes"]), first)


@pytest.mark.parametrize("name", R.CASES)
def test_surface_metrics_match_host(name):
    from arco_amd.utils import surface_gpu
    c = R.case(name)
    p, g = R.device_maps(c)
    got = surface_gpu.surface_metrics(p, g, c["classes"])
    assert len(got) == len(c["classes"])
    for k, m in zip(c["classes"], got):
        if k in c["empty"]:
            assert m is None
            continue
        hd, asd = m
        assert hd == metrics.binary.hd95(c["pred"] == k, c["gt"] == k)
        np.testing.assert_allclose(asd, metrics.binary.asd(c["pred"] == k, c["gt"] == k), rtol=1e-12, atol=0)


def test_ndim_says_which_axes_have_neighbours():
    from arco_amd.utils import surface_gpu
    c = R.case("2d_24x20")
    p, g = R.device_maps(c)
    # a [1, H, W] tensor with ndim = 2 is the 2-D map: the z neighbours do not exist
    got = surface_gpu.surface_histograms(p[None], g[None], c["classes"], ndim=2)
    assert R.exact(got, c["ref"])
    # an [H, W] tensor with ndim = 3 is the one-slice volume: the z neighbours are outside, every voxel is a border voxel
    ref3 = np.stack([R.scipy_hist(c["pred"][None] == k, c["gt"][None] == k, c["nbins"]) for k in c["classes"]])
    assert not np.array_equal(ref3, c["ref"])
    assert R.exact(surface_gpu.surface_histograms(p, g, c["classes"], ndim=3), ref3)
    assert R.exact(surface_gpu.surface_histograms(p[None], g[None], c["classes"]), ref3)


def test_single_pair_functions():
    from arco_amd.utils import surface_gpu
    c = R.case("3d_9x16x11")
    a, b = c["pred"] == 1, c["gt"] == 1
    assert surface_gpu.hd95(a, b) == metrics.binary.hd95(a, b)
    np.testing.assert_allclose(surface_gpu.asd(a, b), metrics.binary.asd(a, b), rtol=1e-12, atol=0)
    np.testing.assert_allclose(surface_gpu.asd(b, a), metrics.binary.asd(b, a), rtol=1e-12, atol=0)
    # label maps count as `> 0`, tensors on the device are taken as they are
    lab_p, lab_g = R.device_maps(c)
    assert surface_gpu.hd95(lab_p, lab_g) == metrics.binary.hd95(c["pred"] > 0, c["gt"] > 0)
    two = R.case("2d_two_voxels")
    assert surface_gpu.hd95(two["pred"], two["gt"]) == 5.0 and surface_gpu.asd(two["pred"], two["gt"]) == 5.0
    empty = np.zeros_like(a)
    for fn in (surface_gpu.hd95, surface_gpu.asd):
        with pytest.raises(RuntimeError, match="first supplied array does not contain any binary object"):
            fn(empty, b)
        with pytest.raises(RuntimeError, match="second supplied array does not contain any binary object"):
            fn(a, empty)
    with pytest.raises(RuntimeError, match="first supplied"):
        metrics.binary.hd95(empty, b)                                    # the host route's message is the same
