"""Connected components by value (arco_amd/csrc/cc.hip, arco_amd/utils/cc_gpu.py, arco_amd/utils/cc_host.py), the part that needs no
GPU:
  references    scipy_ref and the scipy-free flood fill of tests/cc_value_kernel_refs.py agree on every small case at every connectivity;
                on a binary map scipy_ref is cc_kernel_refs.scipy_ref and getLargestCC_by_value is getLargestCC
  host route    cc_host.keep_largest_per_class is scipy_ref's `keep` applied to the map; getLargestCC_by_value is the component of row 0
  cases         what each case is there for actually holds (1 2 1 stays apart, each value of a checkerboard is one component, ...)
  checkers      `same` rejects one label off, the second of two equal blobs kept, a merged 1 2 1, a wrong row-0 winner
  C ABI         the two entry points are exported; the workspace query; ARCO_ERR_ARG on the host
  rejections    the wrappers' TypeError / ValueError and the new keywords of eval_surface - all raised before any GPU call (there is no
                GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

import cc_kernel_refs as B
import cc_value_kernel_refs as R


@pytest.mark.parametrize("name,conn", R.SMALL_RUNS)
def test_references_agree(name, conn):
    x, ndim, classes = R.case(name)
    assert x.size <= R.FLOOD_MAX_VOXELS
    assert R.same(R.flood_ref(x, conn, ndim, classes), R.ref(name, conn))


@pytest.mark.parametrize("name,conn", [(n, c) for n, c in B.RUNS if n in R.BINARY_OF_B])
def test_binary_map_is_the_binary_reference(name, conn):
    x, ndim = B.case(name)
    assert set(np.unique(x)) <= {0, 1}
    labels, keep, info = R.scipy_ref(x, conn, ndim, 2)
    exp = B.ref(name, conn)
    assert R.same((labels, keep, info[0]), exp) and np.array_equal(info[1], exp[2]) and info[2].tolist() == [0, -1, 0]


@pytest.mark.parametrize("name", R.CASES)
def test_host_functions_are_the_reference(name):
    from arco_amd.test_util import getLargestCC
    from arco_amd.utils.cc_host import getLargestCC_by_value, keep_largest_per_class
    x, ndim, classes = R.case(name)
    a = R._as_ndim(x, ndim)
    labels, keep, info = (t.reshape(a.shape) if i < 2 else t for i, t in enumerate(R.ref(name, ndim)))
    assert labels.dtype == np.int32 and keep.dtype == np.uint8 and info.dtype == np.int64 and info.shape == (classes + 1, 3)
    valid = np.where((a >= 1) & (a <= classes - 1), a, 0)                    # the host functions take every non-zero value as a class
    got = keep_largest_per_class(valid)
    assert got.dtype == valid.dtype and np.array_equal(got, valid * keep)
    if info[0, 0] == 0:
        assert name in R.EMPTY and not labels.any() and not keep.any() and info[:classes].tolist() == [[0, -1, 0]] * classes
        with pytest.raises(AssertionError):
            getLargestCC_by_value(valid)
        return
    assert name not in R.EMPTY
    host = getLargestCC_by_value(valid)
    assert host.dtype == np.bool_ and np.array_equal(host, labels == info[0, 1] + 1) and host.sum() == info[0, 2]
    if classes == 2:
        assert np.array_equal(host, getLargestCC(valid)) and np.array_equal(got != 0, host)
    # info is consistent with the maps
    assert np.array_equal(labels > 0, valid != 0) and info[0, 0] == info[1:classes, 0].sum() == len(np.unique(labels[labels > 0]))
    assert info[0, 2] == info[1:classes, 2].max() and info[classes, 0] == ((a < 0) | (a >= classes)).sum()
    for c in range(1, classes):
        n, first, size = info[c]
        assert (n == 0) == (not (valid == c).any())
        if n:
            assert valid.reshape(-1)[first] == c and keep.reshape(-1)[first] == 1 and (keep.astype(bool) & (valid == c)).sum() == size


@pytest.mark.parametrize("name", R.BINARY_OF_B)
def test_by_value_is_getLargestCC_on_a_binary_map(name):
    from arco_amd.test_util import getLargestCC
    from arco_amd.utils.cc_host import getLargestCC_by_value, keep_largest_per_class
    x, ndim = B.case(name)
    a = R._as_ndim(x, ndim)
    if name in B.EMPTY:
        with pytest.raises(AssertionError):
            getLargestCC_by_value(a)
        assert not keep_largest_per_class(a).any()
        return
    assert np.array_equal(getLargestCC_by_value(a), getLargestCC(a))
    assert np.array_equal(keep_largest_per_class(a), getLargestCC(a).astype(a.dtype))


def _n(name, conn, row=0):
    return int(R.ref(name, conn)[2][row, 0])


def test_cases_are_what_they_are_for():
    assert len(R.SMALL) >= 40 and {"random_3d_0.3_v3", "random_2d_0.3_v8"}.isdisjoint(R.SMALL)
    assert sorted({R.case(n)[0].shape[-1] for n in ("w1", "w63", "w64", "w65", "w130")}) == [1, 63, 64, 65, 130]
    row = R.case("w130")[0][0]
    assert (row[0] == 1).all() and row[1, :4].tolist() == [1, 2, 1, 2] and row[2, :5].tolist() == [1, 1, 2, 2, 1]
    assert row[3, 61:67].tolist() == [1, 1, 2, 1, 2, 2] and row[4, :3].tolist() == [1, 2, 1] and row[4, 62:66].tolist() == [3, 1, 2, 1]
    assert row[6, 62:66].tolist() == [1, 1, 2, 2]
    # 1 2 1: three components, the two 1s apart; the first 1 wins its class and row 0
    labels, keep, info = R.ref("one_two_one", 2)
    assert labels.tolist() == [[1, 2, 3]] and keep.tolist() == [[1, 1, 0]] and info.tolist() == [[3, 0, 1], [2, 0, 1], [1, 1, 1], [0, -1, 0]]
    assert R.ref("one_two_one_rows", 1)[2][:3].tolist() == [[5, 1, 5], [4, 0, 1], [1, 1, 5]]
    assert R.ref("one_two_one_rows", 2)[2][:3].tolist() == [[5, 1, 5], [4, 0, 1], [1, 1, 5]]         # not even by the diagonal
    # different values in vertical and diagonal contact: one component per row / plane / colour
    assert [_n("stacked_rows", c) for c in (1, 2)] == [7, 7] and [_n("stacked_planes", c) for c in (1, 2, 3)] == [5, 5, 5]
    cb = R.case("checkerboard")[0]
    assert cb.shape == (9, 10, 11) and set(np.unique(cb)) == {1, 2}
    assert [_n("checkerboard", c) for c in (1, 2, 3)] == [cb.size, 2, 2]
    assert R.ref("checkerboard", 3)[2][:3].tolist() == [[2, 0, 495], [1, 0, 495], [1, 1, 495]]
    assert R.ref("checkerboard", 1)[2][:3].tolist() == [[990, 0, 1], [495, 0, 1], [495, 1, 1]]
    assert [_n("checkerboard_2d", c) for c in (1, 2)] == [9 * 67, 2]
    # nesting: two components of class 1 around and inside the one of class 2
    for name in ("nest_2d", "nest_3d"):
        nd = R.case(name)[1]
        assert all(R.ref(name, c)[2][:3, 0].tolist() == [3, 2, 1] for c in range(1, nd + 1)), name
        keep = R.ref(name, nd)[1]
        assert 0 < keep.sum() < (R.case(name)[0] != 0).sum()                                          # the inner blob goes
    # the same value joined by the diagonal only
    assert [_n("diagonal_2d", c, 2) for c in (1, 2)] == [12, 1]
    assert [_n("diagonal_3d", c, 2) for c in (1, 2, 3)] == [10, 10, 1] and [_n("diagonal_3d_alone", c, 2) for c in (1, 2, 3)] == [10, 10, 1]
    assert [_n("anti_diagonal", c, 2) for c in (1, 2, 3)] == [8, 8, 1]
    assert [_n("diagonal_zy", c, 2) for c in (1, 2, 3)] == [8, 1, 1] and [_n("diagonal_zx", c, 2) for c in (1, 2, 3)] == [8, 1, 1]
    # long walks: the winding shape is one component of class 1 by faces alone
    for name in ("serpentine", "serpentine_3d", "comb", "comb_3d"):
        assert _n(name, 1, 1) == (2 if name == "comb_3d" else 1) and _n(name, 1, 2) >= 1, name
    assert _n("serpentine", 1, 2) == 16 and _n("comb", 1, 2) == 32                          # the gaps: a second value, many components
    # ties
    assert R.ref("tie_same_class", 2)[2].tolist() == [[2, 31, 9], [2, 31, 9], [0, -1, 0], [0, -1, 0]]
    assert R.ref("tie_same_class_later_larger", 2)[2][:2].tolist() == [[2, 200, 10], [2, 200, 10]]
    assert R.ref("tie_two_classes", 2)[2].tolist() == [[2, 31, 9], [1, 200, 9], [1, 31, 9], [0, -1, 0]]
    assert R.ref("tie_two_classes_later_larger", 2)[2][:3].tolist() == [[2, 200, 10], [1, 200, 10], [1, 31, 9]]
    assert R.ref("tie_three", 3)[2][:3].tolist() == [[3, 331, 27], [2, 340, 27], [1, 331, 27]]
    assert R.ref("tie_three_later_larger", 3)[2][:3].tolist() == [[3, 500, 28], [2, 500, 28], [1, 331, 27]]
    # absent classes and the class count
    info = R.ref("absent_class", 3)[2]
    assert info[2].tolist() == [0, -1, 0] and info[1, 0] > 0 and info[3, 0] > 0
    info = R.ref("classes_above_values", 3)[2]
    assert info.shape == (10, 3) and info[3:9].tolist() == [[0, -1, 0]] * 6 and info[9].tolist() == [0, -1, 0]
    corner = R.case("last_corner")[0]
    assert R.ref("last_corner", 3)[2].tolist() == [[1, corner.size - 1, 1], [0, -1, 0], [1, corner.size - 1, 1], [0, -1, 0]]
    assert R.ref("all_one_value", 1)[2][:3].tolist() == [[1, 0, 4 * 5 * 66], [0, -1, 0], [1, 0, 4 * 5 * 66]]
    # values out of range are background and are counted
    for name in ("out_of_range", "out_of_range_2d", "only_out_of_range", "classes_256_out"):
        x, nd, C = R.case(name)
        bad = (x < 0) | (x >= C)
        labels, keep, info = R.ref(name, nd)
        assert (x < 0).any() or name == "classes_256_out"
        assert (x >= C).any() and not labels[bad].any() and not keep[bad].any() and info[C].tolist() == [bad.sum(), np.flatnonzero(bad)[0], 0]
    assert R.case("classes_2")[2] == 2 and R.case("classes_256")[2] == 256 and R.ref("classes_256", 3)[2][255, 0] > 0
    # [1, H, W]: ndim 2 has connectivities 1..2, ndim 3 has 1..3; the same array and the same components in the plane
    assert ("slice_as_2d", 3) not in R.RUNS and ("slice_as_3d", 3) in R.RUNS and ("map_as_3d", 3) in R.RUNS
    assert np.array_equal(R.ref("slice_as_2d", 2)[0], R.ref("slice_as_3d", 3)[0])
    assert not np.array_equal(R.ref("slice_as_2d", 1)[0], R.ref("slice_as_2d", 2)[0])
    randoms = [n for n in R.CASES if n.startswith("random_")]
    assert len(randoms) == 12
    for name in randoms:
        x, nd, C = R.case(name)
        assert x.shape in ((20, 33, 70), (40, 130)) and set(np.unique(x)) == set(range(C)) and _n(name, 1) > _n(name, nd) >= C - 1


def test_checkers_reject_planted_errors():
    exp = R.ref("tie_same_class", 2)
    assert R.same(tuple(a.copy() for a in exp), exp) and R.same(tuple(torch.tensor(a) for a in exp), exp)
    for i in range(3):                                                                 # one element off in each output
        moved = [a.copy() for a in exp]
        moved[i].reshape(-1)[-1] += 1
        assert not R.same(moved, exp), i
    x = R.case("tie_same_class")[0]
    second = [a.copy() for a in exp]                                                   # the second of two equal blobs kept
    second[1] = (exp[0] == 201).astype(np.uint8)
    assert second[1].sum() == exp[1].sum() == 9 and x[second[1] == 1].tolist() == [1] * 9 and not R.same(second, exp)
    exp = R.ref("one_two_one", 2)                                                      # a merged 1 2 1
    merged = [a.copy() for a in exp]
    merged[0][0, 2] = 1
    assert not R.same(merged, exp)
    merged[1][0, 2] = 1
    merged[2][0], merged[2][1] = (2, 0, 2), (1, 0, 2)
    assert not R.same(merged, exp)
    exp = R.ref("tie_two_classes", 2)                                                  # a wrong row-0 winner: the later blob of equal size
    wrong = [a.copy() for a in exp]
    wrong[2][0, 1] = 200
    assert not R.same(wrong, exp)
    assert not R.same((exp[0].astype(np.int64), exp[1], exp[2]), exp)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_workspace_query():
    import arco_amd._lib as L
    lib = L.load()
    assert "arco_cc_value_largest" in L.EXPORTS and "arco_cc_value_ws_bytes" in L.EXPORTS
    assert hasattr(lib, "arco_cc_value_largest") and hasattr(lib, "arco_cc_value_ws_bytes")
    last = 0
    for shape in ((1, 1, 1), (1, 1, 64), (1, 1, 65), (1, 2, 65), (3, 4, 65), (20, 33, 70), (112, 112, 80), (192, 160, 88), (1, 4096, 4096)):
        b = L.query("arco_cc_value_ws_bytes", *shape, 4)
        assert b > last and b % 8 == 0 and b >= 9 * int(np.prod(shape)), shape             # parent, count: 4 bytes per voxel; class: 1
        assert L.query("arco_cc_value_ws_bytes", *shape, 2) <= b <= L.query("arco_cc_value_ws_bytes", *shape, 256)
        last = b
    assert L.query("arco_cc_value_ws_bytes", 2047, 1024, 1024, 3) > 9 * 2047 * 1024 * 1024     # no 32-bit overflow
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (2, 3, 4097), (4097, 1, 1), (2048, 1024, 1024)):
        assert L.query("arco_cc_value_ws_bytes", *shape, 3) == -1, shape
    for classes in (-1, 0, 1, 257, 1 << 16):
        assert L.query("arco_cc_value_ws_bytes", 2, 3, 4, classes) == -1, classes


def test_workspace_sizes_are_exact():
    """The layout of CcvWs: a header of 12 bytes per class plus 8 (padded to 8), two sets of row words of 8 bytes, parent and count
    (4 bytes per voxel each, padded to 8) and the class bytes (padded to 8)."""
    import arco_amd._lib as L
    assert L.query("arco_cc_value_ws_bytes", 3, 4, 65, 3) == 48 + 2 * 12 * 2 * 8 + 2 * 780 * 4 + 784 == 7456
    assert L.query("arco_cc_value_ws_bytes", 1, 1, 9, 2) == 32 + 2 * 1 * 8 + 2 * 10 * 4 + 16 == 144


def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced."""
    import arco_amd._lib as L
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    D, H, W, C = 2, 3, 4, 3
    ws = lib.arco_cc_value_ws_bytes(D, H, W, C)
    # x, D, H, W, ndim, connectivity, classes, ws, ws_bytes, labels, labels_bytes, keep, keep_bytes, info, info_bytes
    ok = [p, D, H, W, 3, 3, C, p, ws, p, 96, p, 24, p, 96]
    rejected = [(0, None), (7, None), (9, None), (11, None), (13, None),                         # a null pointer
                (1, 0), (2, 0), (3, 0), (1, 4097), (2, 4097), (3, 4097),                         # a dim < 1 or > 4096
                (4, 1), (4, 4), (4, 2),                                                          # ndim not 2 or 3; ndim 2 with D != 1
                (5, 0), (5, 4),                                                                  # connectivity outside 1..ndim
                (6, 1), (6, 0), (6, -3), (6, 257),                                               # classes outside 2..256
                (6, 4),                                                                          # ... or more than info and ws hold
                (8, ws - 4), (8, 0), (10, 95), (12, 23), (14, 95)]                               # a buffer smaller than required
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_cc_value_largest(*args, None) == -1, (pos, val)
    big = 1 << 40
    assert lib.arco_cc_value_largest(p, 1, H, W, 2, 3, C, p, 1 << 20, p, 1 << 20, p, 1 << 20, p, 96, None) == -1      # connectivity 3 in 2-D
    assert lib.arco_cc_value_largest(p, 2048, 1024, 1024, 3, 3, C, p, big, p, big, p, big, p, 96, None) == -1        # 2^31 voxels
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    assert lib.arco_cc_value_largest(p, D, H, W, 3, 3, C, odd, ws, p, 96, p, 24, p, 96, None) == -1                   # ws not 8-byte aligned
    assert (buf == 0).all()


# ---- Python level ------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_any_gpu_call():
    from arco_amd.utils import cc_gpu
    t = torch.zeros((2, 5, 6), dtype=torch.int64)
    f = cc_gpu.components_by_value
    with pytest.raises(TypeError):
        f(t.numpy(), 3)
    with pytest.raises(TypeError):
        f(t.float(), 3)
    with pytest.raises(TypeError):
        f(t.bool(), 3)
    for bad in (2.0, "3", None, True):
        with pytest.raises(TypeError, match="classes"):
            f(t, bad)
    for bad in (1, 0, -2, 257):
        with pytest.raises(ValueError, match="classes"):
            f(t, bad)
        with pytest.raises(ValueError, match="classes"):
            cc_gpu.largest_per_class(t, bad)
        with pytest.raises(ValueError, match="classes"):
            cc_gpu.largest_cc_by_value(t.numpy(), bad)
    for shape in ((7,), (2, 3, 4, 5)):                                                     # rank 1 and rank 4
        with pytest.raises(ValueError, match="2-D or 3-D"):
            f(torch.zeros(shape, dtype=torch.int64), 3)
        with pytest.raises(ValueError, match="2-D or 3-D"):
            cc_gpu.largest_per_class(np.zeros(shape, dtype=np.int64), 3)
    with pytest.raises(ValueError, match="4096"):
        f(torch.zeros((1, 4097), dtype=torch.uint8), 3)
    big = torch.zeros(1, dtype=torch.int32).expand(2048, 1024, 1024)                       # 2^31 voxels by shape only: one element
    with pytest.raises(ValueError, match="voxels"):
        f(big, 3)
    for nd, conns in ((None, (0, 4, -1)), (3, (0, 4))):
        for c in conns:
            with pytest.raises(ValueError, match="connectivity"):
                f(t, 3, connectivity=c, ndim=nd)
    for c in (0, 3):
        with pytest.raises(ValueError, match="connectivity"):
            f(t[0], 3, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            f(t[:1], 3, connectivity=c, ndim=2)
    with pytest.raises(ValueError, match="ndim"):
        f(t, 3, ndim=2)                                                                    # ndim 2 for a [2, H, W] tensor
    for nd in (1, 4):
        with pytest.raises(ValueError, match="ndim"):
            f(t, 3, ndim=nd)
    with pytest.raises(RuntimeError, match="GPU"):
        f(t, 3)                                                                            # a valid request for a CPU tensor: no CPU fallback
    for g in (cc_gpu.largest_per_class, cc_gpu.largest_cc_by_value):
        with pytest.raises(TypeError):
            g(t.float(), 3)
        with pytest.raises(TypeError):
            g(t.numpy().astype(np.float32), 3)


def test_route_keywords():
    from arco_amd import eval_surface
    assert eval_surface.NMS_MODES == ("foreground", "value", "per_class")
    for bad in ("class", "VALUE", None, 1):
        for kw in (dict(surface="gpu", cc="gpu"), dict(surface="gpu"), dict()):
            with pytest.raises(ValueError, match="nms_mode"):
                eval_surface.test_all_case(None, [], 3, nms=1, nms_mode=bad, **kw)         # before the model is touched
    for mode in eval_surface.NMS_MODES:
        with pytest.raises(ValueError, match="surface"):
            eval_surface.test_all_case(None, [], 3, nms=1, nms_mode=mode, cc="gpu")        # cc="gpu" still needs surface="gpu"
    image = np.zeros((2, 8, 8), dtype=np.float32)
    for nms in (0, 1):
        with pytest.raises(ValueError, match="surface"):
            eval_surface.test_single_volume(image, image, None, 4, nms=nms, cc="gpu", surface="host")
        with pytest.raises(ValueError, match="surface"):
            eval_surface.test_single_volume(image, image, None, 4, nms=nms, cc="gpu")      # the default surface is the host route
        with pytest.raises(ValueError, match="cc"):
            eval_surface.test_single_volume(image, image, None, 4, nms=nms, cc="cuda", surface="gpu")
