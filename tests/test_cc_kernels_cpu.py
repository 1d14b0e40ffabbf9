"""Connected-component kernels (arco_amd/csrc/cc.hip, arco_amd/utils/cc_gpu.py), the part that needs no GPU:
  references    scipy_ref and the scipy-free flood fill of tests/cc_kernel_refs.py agree on every small case at every connectivity;
                scipy_ref's `largest` is test_util.getLargestCC at full connectivity
  cases         what each case is there for actually holds (one component, all ties, joined by the diagonal only, ...)
  checkers      `same` and the guard check reject a planted error
  C ABI         the two entry points are exported; arco_cc_ws_bytes is positive and monotone; ARCO_ERR_ARG on the host
  rejections    cc_gpu.components' TypeError / ValueError, check_cc and test_all_case(cc="gpu", surface="host") - all raised before any
                GPU call (there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

import cc_kernel_refs as R


@pytest.mark.parametrize("name,conn", R.SMALL_RUNS)
def test_references_agree(name, conn):
    x, ndim = R.case(name)
    assert x.size <= R.FLOOD_MAX_VOXELS
    assert R.same(R.flood_ref(x, conn, ndim), R.ref(name, conn))


@pytest.mark.parametrize("name", R.CASES)
def test_largest_is_getLargestCC(name):
    from arco_amd.test_util import getLargestCC
    x, ndim = R.case(name)
    labels, largest, info = R.ref(name, ndim)
    assert labels.dtype == np.int32 and largest.dtype == np.uint8 and info.dtype == np.int64 and info.shape == (3,)
    assert labels.shape == largest.shape == x.shape
    if name in R.EMPTY:
        assert info.tolist() == [0, -1, 0] and not largest.any() and not labels.any()
        with pytest.raises(AssertionError):
            getLargestCC(x)
        return
    host = getLargestCC(R._as_ndim(x, ndim))
    assert host.dtype == np.bool_ and np.array_equal(host.reshape(x.shape), largest.astype(bool))
    # info is consistent with the two maps
    assert info[0] == len(np.unique(labels[labels > 0])) and info[2] == largest.sum() > 0
    assert largest.reshape(-1)[info[1]] == 1 and labels.reshape(-1)[info[1]] == info[1] + 1
    assert np.array_equal(labels > 0, x != 0)


def _n(name, conn):
    return int(R.ref(name, conn)[2][0])


def test_cases_are_what_they_are_for():
    assert len(R.SMALL) >= 30 and {"random_0.3", "random_2d_0.3"}.isdisjoint(R.SMALL)
    assert sorted({R.case(n)[0].shape[-1] for n in ("w1", "w63", "w64", "w65", "w130")}) == [1, 63, 64, 65, 130]
    row = R.case("w130")[0][0]
    assert row[0].all() and not row[1].any() and row[2, 63] and row[2, 64] and row[2, 127] and row[2, 128]      # runs across the words
    for name in ("serpentine", "serpentine_3d", "comb", "comb_3d"):                    # one winding component, faces suffice
        x, ndim = R.case(name)
        assert _n(name, 1) == (2 if name == "comb_3d" else 1), name
    x, _ = R.case("comb")
    assert _n("comb", 1) == 1 and R.scipy_ref(x[:-1], 1)[2][0] == 33                   # the prongs meet in the last row only
    cb, _ = R.case("checkerboard")
    assert cb.shape == (9, 10, 11) and _n("checkerboard", 3) == 1 and _n("checkerboard", 2) == 1
    labels, largest, info = R.ref("checkerboard", 1)                                   # every voxel alone: all sizes tie, the first wins
    assert info.tolist() == [int(cb.sum()), 0, 1] and largest.sum() == 1 and largest.reshape(-1)[0] == 1
    assert np.array_equal(labels.reshape(-1)[cb.reshape(-1) != 0], np.flatnonzero(cb.reshape(-1)) + 1)
    assert (_n("diagonal_2d", 1), _n("diagonal_2d", 2)) == (12, 1)
    assert [_n("diagonal_3d", c) for c in (1, 2, 3)] == [10, 10, 1]
    assert [_n("anti_diagonal", c) for c in (1, 2, 3)] == [8, 8, 1]
    assert [_n("diagonal_zy", c) for c in (1, 2, 3)] == [8, 1, 1] and [_n("diagonal_zx", c) for c in (1, 2, 3)] == [8, 1, 1]
    # ties: the first blob in memory wins; one more voxel on the last one and that one wins
    assert R.ref("tie_two", 2)[2].tolist() == [2, 1 * 30 + 1, 9] and R.ref("tie_two_later_larger", 2)[2].tolist() == [2, 6 * 30 + 20, 10]
    assert R.ref("tie_three", 3)[2].tolist() == [3, 300 + 30 + 1, 27]
    assert R.ref("tie_three_later_larger", 3)[2].tolist() == [3, 300 + 6 * 30 + 20, 28]
    ones, _ = R.case("all_ones")
    assert R.ref("all_ones", 1)[2].tolist() == [1, 0, ones.size]
    corner, _ = R.case("last_corner")
    assert R.ref("last_corner", 3)[2].tolist() == [1, corner.size - 1, 1]
    assert (R.case("negative_labels")[0] < 0).any() and set(np.unique(R.case("classes_1_to_3")[0])) == {0, 1, 2, 3}
    # [1, H, W]: ndim 2 has connectivities 1..2, ndim 3 has 1..3; the same array and the same components in the plane
    assert ("slice_as_2d", 3) not in R.RUNS and ("slice_as_3d", 3) in R.RUNS and ("map_as_3d", 3) in R.RUNS
    assert np.array_equal(R.ref("slice_as_2d", 2)[0], R.ref("slice_as_3d", 3)[0])
    assert not np.array_equal(R.ref("slice_as_2d", 1)[0], R.ref("slice_as_2d", 2)[0])
    for name in ("random_0.1", "random_0.3", "random_0.6", "random_2d_0.1", "random_2d_0.3", "random_2d_0.6"):
        assert R.case(name)[0].shape in ((20, 33, 70), (40, 130)) and _n(name, 1) > _n(name, R.case(name)[1]) >= 1


def test_checkers_reject_planted_errors():
    exp = R.ref("random_small", 3)
    assert R.same(tuple(a.copy() for a in exp), exp) and R.same(tuple(torch.tensor(a) for a in exp), exp)
    for i in range(3):
        moved = [a.copy() for a in exp]
        moved[i].reshape(-1)[-1] += 1
        assert not R.same(moved, exp), i
    assert not R.same((exp[0].astype(np.int64), exp[1], exp[2]), exp)
    for dtype in (torch.uint8, torch.int32, torch.int64):
        buf = R.guarded(100, dtype)
        assert R.untouched(buf)
        buf[:100] = 7
        assert R.guards_intact(buf, 100) and not R.untouched(buf)
        buf[100 + R.GUARD - 1] = 0
        assert not R.guards_intact(buf, 100)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_exports_and_workspace_query():
    import arco_amd._lib as L
    lib = L.load()
    assert "arco_cc_largest" in L.EXPORTS and "arco_cc_ws_bytes" in L.EXPORTS
    assert hasattr(lib, "arco_cc_largest") and hasattr(lib, "arco_cc_ws_bytes")
    last = 0
    for shape in ((1, 1, 1), (1, 1, 64), (1, 1, 65), (1, 2, 65), (3, 4, 65), (20, 33, 70), (112, 112, 80), (192, 160, 88), (1, 4096, 4096)):
        b = L.query("arco_cc_ws_bytes", *shape)
        assert b > last and b % 4 == 0 and b >= 8 * int(np.prod(shape)), shape             # parent and count: 4 bytes per voxel each
        last = b
    assert L.query("arco_cc_ws_bytes", 2047, 1024, 1024) > 8 * 2047 * 1024 * 1024          # no 32-bit overflow
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (2, 3, 4097), (4097, 1, 1), (2048, 1024, 1024)):
        assert L.query("arco_cc_ws_bytes", *shape) == -1, shape


def test_workspace_sizes_are_exact():
    """The layout of CcWs: a 16-byte header, 8 bytes per row word, parent (4 bytes per voxel, padded to 8) and count (4 per voxel)."""
    import arco_amd._lib as L
    assert L.query("arco_cc_ws_bytes", 3, 4, 65) == 16 + 12 * 2 * 8 + 780 * 4 + 780 * 4 == 6448
    assert L.query("arco_cc_ws_bytes", 1, 1, 9) == 16 + 1 * 8 + 10 * 4 + 9 * 4 == 100


def test_argument_checks_reject_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced."""
    import arco_amd._lib as L
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    D, H, W = 2, 3, 4
    ws = lib.arco_cc_ws_bytes(D, H, W)
    # x, D, H, W, ndim, connectivity, ws, ws_bytes, labels, labels_bytes, largest, largest_bytes, info, info_bytes
    ok = [p, D, H, W, 3, 3, p, ws, p, 96, p, 24, p, 24]
    rejected = [(0, None), (6, None), (8, None), (10, None), (12, None),                         # a null pointer
                (1, 0), (2, 0), (3, 0), (1, 4097), (2, 4097), (3, 4097),                         # a dim < 1 or > 4096
                (4, 1), (4, 4), (4, 2),                                                          # ndim not 2 or 3; ndim 2 with D != 1
                (5, 0), (5, 4),                                                                  # connectivity outside 1..ndim
                (7, ws - 4), (7, 0), (9, 95), (11, 23), (13, 23)]                                # a buffer smaller than required
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_cc_largest(*args, None) == -1, (pos, val)
    assert lib.arco_cc_largest(p, 1, H, W, 2, 3, p, 1 << 20, p, 1 << 20, p, 1 << 20, p, 24, None) == -1      # connectivity 3 in 2-D
    assert lib.arco_cc_largest(p, 2048, 1024, 1024, 3, 3, p, 1 << 40, p, 1 << 40, p, 1 << 40, p, 24, None) == -1   # 2^31 voxels
    assert (buf == 0).all()


# ---- Python level ------------------------------------------------------------------------------------------------------------------------
def test_components_refuses_before_any_gpu_call():
    from arco_amd.utils import cc_gpu
    t = torch.zeros((2, 5, 6), dtype=torch.int64)
    with pytest.raises(TypeError):
        cc_gpu.components(t.numpy())
    with pytest.raises(TypeError):
        cc_gpu.components(t.float())
    with pytest.raises(TypeError):
        cc_gpu.components(t.bool())
    for shape in ((7,), (2, 3, 4, 5)):                                                     # rank 1 and rank 4
        with pytest.raises(ValueError, match="2-D or 3-D"):
            cc_gpu.components(torch.zeros(shape, dtype=torch.int64))
    with pytest.raises(ValueError, match="4096"):
        cc_gpu.components(torch.zeros((1, 4097), dtype=torch.uint8))
    big = torch.zeros(1, dtype=torch.int32).expand(2048, 1024, 1024)                       # 2^31 voxels by shape only: one element
    assert big.numel() == 1 << 31
    with pytest.raises(ValueError, match="voxels"):
        cc_gpu.components(big)
    for nd, conns in ((None, (0, 4, -1)), (3, (0, 4))):
        for c in conns:
            with pytest.raises(ValueError, match="connectivity"):
                cc_gpu.components(t, connectivity=c, ndim=nd)
    for c in (0, 3):
        with pytest.raises(ValueError, match="connectivity"):
            cc_gpu.components(t[0], connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            cc_gpu.components(t[:1], connectivity=c, ndim=2)
    with pytest.raises(ValueError, match="ndim"):
        cc_gpu.components(t, ndim=2)                                                       # ndim 2 for a [2, H, W] tensor
    for nd in (1, 4):
        with pytest.raises(ValueError, match="ndim"):
            cc_gpu.components(t, ndim=nd)
    with pytest.raises(RuntimeError, match="GPU"):
        cc_gpu.components(t)                                                               # a valid request for a CPU tensor: no CPU fallback


def test_route_keywords():
    from arco_amd import eval_surface
    from arco_amd.utils import cc_gpu
    assert cc_gpu.check_cc("host") == "host" and cc_gpu.check_cc("gpu") == "gpu"
    for bad in ("cuda", "GPU", None, 1):
        with pytest.raises(ValueError, match="cc"):
            cc_gpu.check_cc(bad)
        with pytest.raises(ValueError, match="cc"):
            eval_surface.test_all_case(None, [], 2, surface="gpu", cc=bad)
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_all_case(None, [], 2, cc="gpu", surface="host")                  # before the model is touched
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_all_case(None, [], 2, cc="gpu")                                  # the default surface is the host route
    with pytest.raises(ValueError, match="surface"):
        eval_surface.test_all_case(None, [], 2, cc="gpu", surface="cuda")
