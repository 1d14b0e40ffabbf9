"""Connected components by value (arco_amd/csrc/cc.hip) on the GPU against the scipy reference of tests/cc_value_kernel_refs.py
(which tests/test_cc_value_kernels_cpu.py holds to a scipy-free flood fill and to the host functions of arco_amd/utils/cc_host.py).  Labels, the kept
components and the counts are integers with one canonical value each, so every check is equality."""
import numpy as np
import pytest
import torch

import cc_kernel_refs as B
import cc_value_kernel_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


@pytest.mark.parametrize("name,conn", R.RUNS)
def test_components_exact_and_guards_intact(L, name, conn):
    from arco_amd.utils import cc_gpu
    x, ndim, classes = R.case(name)
    exp = R.ref(name, conn)
    rc, got, bufs = R.run_guarded(L, x, ndim, conn, classes)
    assert rc == 0
    for buf, n in bufs:
        assert R.guards_intact(buf, n)
    assert R.same(got, exp)
    rc, again, _ = R.run_guarded(L, x, ndim, conn, classes)                              # a second run: the identical bytes
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(got, again))
    xd = torch.tensor(x).cuda()
    first = cc_gpu.components_by_value(xd, classes, connectivity=conn, ndim=ndim)
    assert all(t.is_cuda for t in first) and R.same(first, exp)
    second = cc_gpu.components_by_value(xd, classes, connectivity=conn, ndim=ndim)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("name,conn", [(n, c) for n, c in B.RUNS if n in R.BINARY_OF_B])
def test_binary_map_equals_arco_cc_largest(L, name, conn):
    """classes = 2 on a 0 / 1 map: labels, keep and rows 0 and 1 of info are what the binary kernels return."""
    x, ndim = B.case(name)
    rc_b, (labels_b, largest_b, info_b), _ = B.run_guarded(L, x, ndim, conn)
    rc, (labels, keep, info), bufs = R.run_guarded(L, x, ndim, conn, 2)
    assert rc_b == 0 and rc == 0
    for buf, n in bufs:
        assert R.guards_intact(buf, n)
    assert labels.dtype == labels_b.dtype and torch.equal(labels, labels_b)
    assert keep.dtype == largest_b.dtype and torch.equal(keep, largest_b)
    assert torch.equal(info[0], info_b) and torch.equal(info[1], info_b) and info[2].tolist() == [0, -1, 0]


def test_default_connectivity_is_full():
    from arco_amd.utils import cc_gpu
    for name in ("diagonal_3d", "diagonal_2d", "map_as_3d"):
        x, ndim, classes = R.case(name)
        assert R.same(cc_gpu.components_by_value(torch.tensor(x).cuda(), classes, ndim=ndim), R.ref(name, ndim))


BAD = [dict(ws_short=8), dict(ws_short=4), dict(passed=dict(classes=1)), dict(passed=dict(classes=257)), dict(passed=dict(classes=0)),
       dict(passed=dict(classes=4)),                                                     # more classes than ws and info are sized for
       dict(passed=dict(ndim=2)), dict(passed=dict(ndim=4)), dict(passed=dict(connectivity=0)), dict(passed=dict(connectivity=4))]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_bad_argument_is_refused_and_nothing_written(L, bad):
    x, ndim, classes = R.case("absent_class")                                            # [6, 7, 70]: D > 1, so ndim = 2 is an error
    assert x.shape[0] > 1 and classes == 4
    rc, _, bufs = R.run_guarded(L, x, ndim, 3, 3, **bad)                                 # (sized for 3 classes)
    assert rc == -1
    for buf, _ in bufs:
        assert R.untouched(buf)


def test_bad_argument_through_the_library_call(L):
    x, _, classes = R.case("absent_class")
    with pytest.raises(RuntimeError, match="arco_cc_value_largest"):                     # through L.call: the library's usual error
        xd = torch.tensor(x).cuda()
        out = torch.empty(x.size, dtype=torch.int32, device="cuda")
        L.call("arco_cc_value_largest", L.ptr(xd), *x.shape, 3, 3, classes, L.ptr(out), 8, L.ptr(out), x.size * 4, L.ptr(out), x.size,
               L.ptr(out), 24 * (classes + 1))


@pytest.mark.parametrize("name", ["random_3d_0.3_v3", "random_2d_0.3_v8", "w130"])
def test_dtypes_and_views(name):
    from arco_amd.utils import cc_gpu
    x, ndim, classes = R.case(name)
    exp = R.ref(name, ndim)
    xd = torch.tensor(x).cuda()
    for dtype in (torch.int64, torch.int32, torch.uint8):
        assert R.same(cc_gpu.components_by_value(xd.to(dtype), classes), exp), dtype
    wide = torch.zeros((*x.shape[:-1], 2 * x.shape[-1]), dtype=torch.int64, device="cuda")        # every second column of a wider volume
    wide[..., ::2] = xd
    wide[..., 1::2] = 1
    view = wide[..., ::2]
    assert not view.is_contiguous() and R.same(cc_gpu.components_by_value(view, classes), exp)
    tr = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not tr.is_contiguous() and R.same(cc_gpu.components_by_value(tr, classes), exp)


HOST_CASES = ["random_3d_0.3_v3", "random_3d_0.6_v8", "random_2d_0.1_v3", "serpentine_3d", "nest_3d", "tie_three", "tie_two_classes",
              "tie_same_class", "absent_class", "classes_256", "classes_2", "checkerboard"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_wrappers_equal_the_host_functions(name):
    from arco_amd.utils.cc_host import getLargestCC_by_value, keep_largest_per_class
    from arco_amd.utils import cc_gpu
    x, _, classes = R.case(name)
    per_class, by_value = keep_largest_per_class(x), getLargestCC_by_value(x)
    assert (per_class != 0).sum() >= by_value.sum() > 0
    for arg in (x, torch.tensor(x).cuda(), torch.tensor(x), x.astype(np.int32), torch.tensor(x).cuda().to(torch.int16)):
        got = cc_gpu.largest_per_class(arg, classes)
        assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == x.shape
        assert np.array_equal(got.cpu().numpy(), per_class)
        got = cc_gpu.largest_cc_by_value(arg, classes)
        assert got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == x.shape
        assert np.array_equal(got.cpu().numpy(), by_value)
    assert cc_gpu.largest_per_class(x, classes, device="cuda:0").device == torch.device("cuda:0")
    if classes == 2:                                                                     # a bool map is the two-class label map
        assert np.array_equal(cc_gpu.largest_per_class(x != 0, 2).cpu().numpy(), per_class)
        assert np.array_equal(cc_gpu.largest_cc_by_value(torch.tensor(x != 0).cuda(), 2).cpu().numpy(), by_value)


@pytest.mark.parametrize("name", ["out_of_range", "out_of_range_2d", "only_out_of_range", "classes_256_out"])
def test_out_of_range_value_is_a_value_error(name):
    from arco_amd.utils import cc_gpu
    x, _, classes = R.case(name)
    first = int(np.flatnonzero((x.reshape(-1) < 0) | (x.reshape(-1) >= classes))[0])
    for arg in (x, torch.tensor(x).cuda()):
        with pytest.raises(ValueError, match=f"linear index {first}$"):
            cc_gpu.largest_per_class(arg, classes)
        with pytest.raises(ValueError, match=f"linear index {first}$"):
            cc_gpu.largest_cc_by_value(arg, classes)
    valid = np.where((x >= 1) & (x <= classes - 1), x, 0)                                # the same map without them is taken
    assert np.array_equal(cc_gpu.largest_per_class(valid, classes).cpu().numpy() != 0, R.ref(name, x.ndim)[1] != 0)


def test_no_foreground():
    from arco_amd.utils import cc_gpu
    for name in ("all_zeros", "all_zeros_2d"):
        x, ndim, classes = R.case(name)
        labels, keep, info = cc_gpu.components_by_value(torch.tensor(x).cuda(), classes)
        assert info.cpu().tolist() == [[0, -1, 0]] * (classes + 1) and not labels.any() and not keep.any()
        assert not cc_gpu.largest_per_class(x, classes).any()
        with pytest.raises(AssertionError):
            cc_gpu.largest_cc_by_value(x, classes)
        with pytest.raises(AssertionError):
            cc_gpu.largest_cc_by_value(torch.tensor(x).cuda(), classes)
