"""Connected-component kernels (arco_amd/csrc/cc.hip) on the GPU against the scipy reference of tests/cc_kernel_refs.py (which
tests/test_cc_kernels_cpu.py holds to a scipy-free flood fill and to test_util.getLargestCC).  Labels, the largest component and the
counts are integers with one canonical value each, so every check is equality."""
import numpy as np
import pytest
import torch

import cc_kernel_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


@pytest.mark.parametrize("name,conn", R.RUNS)
def test_components_exact_and_guards_intact(L, name, conn):
    from arco_amd.utils import cc_gpu
    x, ndim = R.case(name)
    exp = R.ref(name, conn)
    rc, got, bufs = R.run_guarded(L, x, ndim, conn)
    assert rc == 0
    for buf, n in bufs:
        assert R.guards_intact(buf, n)
    assert R.same(got, exp)
    xd = torch.tensor(x).cuda()
    first = cc_gpu.components(xd, connectivity=conn, ndim=ndim)
    assert all(t.is_cuda for t in first) and R.same(first, exp)
    again = cc_gpu.components(xd, connectivity=conn, ndim=ndim)                          # a second call: the identical tensors
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_default_connectivity_is_full():
    from arco_amd.utils import cc_gpu
    for name in ("diagonal_3d", "diagonal_2d", "map_as_3d"):
        x, ndim = R.case(name)
        assert R.same(cc_gpu.components(torch.tensor(x).cuda(), ndim=ndim), R.ref(name, ndim))


def test_short_workspace_is_refused_and_nothing_written(L):
    x, ndim = R.case("random_small")
    rc, _, bufs = R.run_guarded(L, x, ndim, 3, ws_short=4)                               # one word short
    assert rc == -1
    for buf, _ in bufs:
        assert R.untouched(buf)
    with pytest.raises(RuntimeError, match="arco_cc_largest"):                           # through L.call: the library's usual error
        xd = torch.tensor(x).cuda()
        out = torch.empty(x.size, dtype=torch.int32, device="cuda")
        L.call("arco_cc_largest", L.ptr(xd), *x.shape, 3, 3, L.ptr(out), 8, L.ptr(out), x.size * 4, L.ptr(out), x.size, L.ptr(out), 24)


@pytest.mark.parametrize("name", ["classes_1_to_3", "random_2d_0.3", "w130"])
def test_dtypes_and_views(name):
    from arco_amd.utils import cc_gpu
    x, ndim = R.case(name)
    exp = R.ref(name, ndim)
    xd = torch.tensor(x).cuda()
    for dtype in (torch.int64, torch.int32, torch.uint8):
        assert R.same(cc_gpu.components(xd.to(dtype)), exp), dtype
    # a non-contiguous view: every second column of a volume twice as wide, and a transposed view of the transposed copy
    wide = torch.zeros((*x.shape[:-1], 2 * x.shape[-1]), dtype=torch.int64, device="cuda")
    wide[..., ::2] = xd
    wide[..., 1::2] = 1 - xd.clamp(0, 1)
    view = wide[..., ::2]
    assert not view.is_contiguous() and R.same(cc_gpu.components(view), exp)
    tr = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not tr.is_contiguous() and R.same(cc_gpu.components(tr), exp)


@pytest.mark.parametrize("name", ["random_0.3", "serpentine_3d", "tie_three", "tie_two", "negative_labels", "classes_1_to_3"])
def test_largest_cc_equals_getLargestCC(name):
    from arco_amd.test_util import getLargestCC
    from arco_amd.utils import cc_gpu
    x, _ = R.case(name)
    host = getLargestCC(x)
    for arg in (x, x != 0, torch.tensor(x).cuda(), torch.tensor(x != 0).cuda(), torch.tensor(x)):
        got = cc_gpu.largest_cc(arg)
        assert got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == x.shape
        assert np.array_equal(got.cpu().numpy(), host)
    assert cc_gpu.largest_cc(x, device="cuda:0").device == torch.device("cuda:0")


def test_no_foreground():
    from arco_amd.utils import cc_gpu
    for name in R.EMPTY:
        x, ndim = R.case(name)
        labels, largest, info = cc_gpu.components(torch.tensor(x).cuda())
        assert info.cpu().tolist() == [0, -1, 0] and not labels.any() and not largest.any()
        with pytest.raises(AssertionError):
            cc_gpu.largest_cc(x)
        with pytest.raises(AssertionError):
            cc_gpu.largest_cc(torch.tensor(x).cuda())
