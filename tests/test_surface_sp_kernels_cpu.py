"""Surface-distance kernels with a voxel spacing and a connectivity (arco_amd/csrc/surface.hip), the part that needs no GPU:
  border        the O(n^2) border of tests/surface_sp_kernel_refs.py equals X ^ binary_erosion(X, generate_binary_structure(ndim, c))
  references    sqrt of the brute force is within REL_SCIPY (4 * 2^-52, derived in the refs module) of scipy on every case, spacing and
                connectivity, and array_equal to it with spacing (1, 1, 1)
  planted       the voxel nearest by index is not the nearest in millimetres; the border grows with the connectivity
  finish        hd95 / asd finished from the REFERENCE records equal metrics.binary to rtol 1e-12 (per-distance REL_SCIPY; then one
                pairwise float64 sum and one linear interpolation over at most a few thousand values)
  checkers      `exact` rejects one record off by 8 ulp and one record dropped
  rejections    ARCO_ERR_ARG of arco_surface_sp_dist on the host, arco_surface_sp_ws_bytes, and the Python-level ValueErrors - raised
                before any GPU call (there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import binary_erosion, generate_binary_structure

import surface_sp_kernel_refs as S
from arco_amd.utils import metrics

COMBOS = S.combos()


@pytest.mark.parametrize("name", S.CASES)
def test_brute_border_equals_erosion(name):
    c = S.case(name)
    for conn in range(1, c["ndim"] + 1):
        fp = generate_binary_structure(c["ndim"], conn)
        assert len(S.offsets(c["ndim"], conn)) == int(fp.sum()) - 1
        for k in c["classes"]:
            for which in ("pred", "gt"):
                x = c[which] == k
                got = np.zeros_like(x)
                got[tuple(S.border_points(name, which, k, conn).T)] = True
                assert np.array_equal(got, x ^ binary_erosion(x, structure=fp, iterations=1)), (k, which, conn)
                assert np.array_equal(got, S.brute_border(x, conn))


@pytest.mark.parametrize("name,sp,conn", COMBOS)
def test_brute_force_within_bound_of_scipy(name, sp, conn):
    c = S.case(name)
    vs = S.spacing_for(sp, c["ndim"])
    ref = S.brute_records(name, sp, conn)
    for i, k in enumerate(c["classes"]):
        d0, d1 = S.scipy_distances(c["pred"] == k, c["gt"] == k, vs, conn)
        if k in c["empty"]:
            assert d0.size == d1.size == ref[(i, 0)].size == ref[(i, 1)].size == 0
            continue
        assert ref[(i, 0)].size > 0 and ref[(i, 1)].size > 0
        for got, exp in ((np.sqrt(ref[(i, 0)]), d0), (np.sqrt(ref[(i, 1)]), d1)):
            err = float((np.abs(got - exp) / np.where(exp > 0, exp, 1.0)).max()) if got.shape == exp.shape else np.inf
            print(f"{name} {sp} conn {conn} class {k}: {got.size} distances, worst relative difference {err / 2.0 ** -52:.3f} * 2^-52")
            assert S.within(got, exp, S.REL_SCIPY)
            if sp == "unit":
                assert np.array_equal(got, exp)


def test_cases_and_planted_answers():
    assert S.TILE < 300 and {"3d_2x300x3", "3d_300x3x2"} <= set(S.CASES)           # lines longer than the float64 LDS tile
    assert len(COMBOS) == 2 * 5 * 2 + (len(S.CASES) - 2) * 5 * 3
    for name in S.CASES:
        assert int(np.prod(S.case(name)["shape"])) <= S.BRUTE_MAX_VOXELS
    # nearest by index (one voxel along z) is 10 mm away, the voxel three along x only 3 mm: 9.0, not 100.0
    c = S.case("nearest_by_index")
    for conn in (1, 2, 3):
        pa, pb = S.border_points("nearest_by_index", "pred", 1, conn), S.border_points("nearest_by_index", "gt", 1, conn)
        assert S._brute_d2(pa, pb, (10.0, 1.0, 1.0)).tolist() == [9.0]
        assert sorted(S._brute_d2(pb, pa, (10.0, 1.0, 1.0)).tolist()) == [9.0, 100.0]
        assert S._brute_d2(pa, pb, (1.0, 1.0, 1.0)).tolist() == [1.0]
    assert metrics.binary.hd95(c["pred"], c["gt"], voxelspacing=(10, 1, 1)) == pytest.approx(np.percentile([3.0, 3.0, 10.0], 95))
    assert S.brute_records("nearest_by_index", "10_1.25_1.25", 1)[(0, 0)].tolist() == [(1.25 * 3) * (1.25 * 3)]
    # the border of the block with two diagonal holes grows with the connectivity
    n = [len(S.border_points("diagonal_holes", "pred", 1, conn)) for conn in (1, 2, 3)]
    assert n[0] < n[1] < n[2]
    # a class absent from gt gives empty groups on both sides; the class range may start above 1
    absent = S.brute_records("3d_absent", "unit", 1)
    assert S.case("3d_absent")["empty"] == [2] and absent[(1, 0)].size == absent[(1, 1)].size == 0 and absent[(0, 0)].size > 0
    assert S.case("3d_from_class_2")["classes"] == [2, 3]


@pytest.mark.parametrize("name,sp,conn", [t for t in COMBOS if t[2] in (1, 3) or t[1] == "unit"])
def test_finish_from_reference_records_equals_host(name, sp, conn):
    from arco_amd.utils import surface_gpu
    c = S.case(name)
    vs = S.spacing_for(sp, c["ndim"])
    ref = S.brute_records(name, sp, conn)
    for i, k in enumerate(c["classes"]):
        got = surface_gpu.finish_distances(np.sqrt(ref[(i, 0)]), np.sqrt(ref[(i, 1)]))
        if k in c["empty"]:
            assert got is None
            continue
        np.testing.assert_allclose(got[0], metrics.binary.hd95(c["pred"] == k, c["gt"] == k, vs, conn), rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[1], metrics.binary.asd(c["pred"] == k, c["gt"] == k, vs, conn), rtol=1e-12, atol=0)


def test_checkers_reject_planted_errors():
    ref = S.brute_records("3d_14x12x10", "2.9_0.7_1.3", 2)
    copy = {k: v.copy() for k, v in ref.items()}
    assert S.exact(copy, ref)
    val = np.concatenate([ref[k] for k in sorted(ref)])
    tag = np.concatenate([np.full(ref[k].size, 2 * k[0] + k[1], dtype=np.int32) for k in sorted(ref)])
    perm = np.random.default_rng(0).permutation(val.size)
    assert S.exact(S.group(val[perm], tag[perm], 3), ref)                          # the order of arrival does not matter
    assert S.exact(S.group(torch.tensor(val[perm]), torch.tensor(tag[perm]), 3), ref)
    off = {k: v.copy() for k, v in ref.items()}
    j = off[(1, 0)].size // 2
    off[(1, 0)][j:j + 1] = (off[(1, 0)][j:j + 1].view(np.int64) + 8).view(np.float64)      # one record off by 8 ulp
    assert off[(1, 0)][j] != ref[(1, 0)][j] and abs(off[(1, 0)][j] / ref[(1, 0)][j] - 1) < 1e-14
    assert not S.exact(off, ref)
    dropped = {k: v.copy() for k, v in ref.items()}
    dropped[(2, 1)] = dropped[(2, 1)][:-1]
    assert not S.exact(dropped, ref)
    assert not S.exact(S.group(np.delete(val, 5), np.delete(tag, 5), 3), ref)
    assert not S.exact({k: v.astype(np.float32) for k, v in ref.items()}, ref)
    a = np.array([1.0, 2.0])
    assert S.within(a * (1 + 2.0 ** -51), a, S.REL_SCIPY) and not S.within(a * (1 + 2.0 ** -49), a, S.REL_SCIPY)
    assert not S.within(a[:1], a, S.REL_SCIPY)


# ---- argument checks (host side) ---------------------------------------------------------------------------------------------------------
def test_c_abi_rejects_bad_arguments_on_the_host():
    """ARCO_ERR_ARG (-1) is returned before anything is launched, so this needs no GPU; the pointers are host addresses (or null) that
    are never dereferenced."""
    import arco_amd._lib as L
    lib = L.load()
    assert "arco_surface_sp_dist" in L.EXPORTS and "arco_surface_sp_ws_bytes" in L.EXPORTS
    buf = torch.zeros(64, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    bad = -1
    D, H, W, nc = 2, 3, 4, 2
    ws = nc * 2 * 2 * D * H * W * 8
    assert lib.arco_surface_sp_ws_bytes(D, H, W, nc) == ws == 1536
    assert lib.arco_surface_sp_ws_bytes(192, 160, 88, 1) == 2 * 2 * 192 * 160 * 88 * 8
    assert lib.arco_surface_sp_ws_bytes(4096, 4096, 4096, 32) == 32 * 2 * 2 * 4096 ** 3 * 8        # no 32-bit overflow
    for args in ((0, 3, 4, 1), (2, 0, 4, 1), (2, 3, 4097, 1), (2, 3, 4, 0), (2, 3, 4, 33)):
        assert lib.arco_surface_sp_ws_bytes(*args) == bad, args
    inf, nan = float("inf"), float("nan")
    # surface_sp_dist: 0 pred, 1 gt, 2 D, 3 H, 4 W, 5 ndim, 6 connectivity, 7 sz, 8 sy, 9 sx, 10 c_lo, 11 c_hi, 12 ws, 13 ws_bytes,
    #                  14 val, 15 tag, 16 cap, 17 count
    ok = [p, p, D, H, W, 3, 1, 10.0, 1.25, 1.25, 1, 2, p, ws, p, p, 2 * D * H * W, p]
    rejected = [(0, None), (1, None), (12, None), (14, None), (15, None), (17, None),                # a null pointer
                (2, 0), (3, 0), (4, 0), (2, -1), (2, 4097), (3, 4097), (4, 4097),                    # a dim < 1 or > 4096
                (5, 1), (5, 4), (5, 0),                                                              # ndim not in {2, 3}
                (5, 2),                                                                              # ndim 2 with D != 1
                (6, 0), (6, 4), (6, -1),                                                             # connectivity outside 1..ndim
                (7, 0.0), (7, -1.0), (7, inf), (7, nan), (8, 0.0), (8, -2.5), (8, inf), (8, nan),    # a spacing not finite and > 0
                (9, 0.0), (9, -1e-3), (9, -inf), (9, nan),
                (11, 0),                                                                             # c_hi < c_lo
                (11, 33),                                                                            # 33 classes
                (13, ws - 1), (13, 0),                                                               # a short workspace
                (16, 0), (16, -5)]                                                                   # cap < 1
    for pos, val in rejected:
        args = list(ok)
        args[pos] = val
        assert lib.arco_surface_sp_dist(*args, None) == bad, (pos, val)
    # 33 classes with a workspace that would be large enough: it is the class count that is rejected
    assert lib.arco_surface_sp_dist(p, p, D, H, W, 3, 1, 1.0, 1.0, 1.0, 0, 32, p, 1 << 40, p, p, 48, p, None) == bad
    # ndim 2: D must be 1, connectivity 3 is outside 1..ndim, and sz is ignored - with a bad sz it is the short workspace that is seen
    ws2 = 2 * 2 * H * W * 8
    assert lib.arco_surface_sp_dist(p, p, 1, H, W, 2, 3, 1.0, 1.0, 1.0, 1, 1, p, ws2, p, p, 24, p, None) == bad
    assert lib.arco_surface_sp_dist(p, p, 1, H, W, 2, 2, nan, 1.0, 1.0, 1, 1, p, ws2 - 1, p, p, 24, p, None) == bad


def test_python_level_errors_come_before_any_gpu_call():
    from arco_amd import eval_surface
    from arco_amd.utils import surface_gpu
    a = np.zeros((4, 5, 6), dtype=np.int64)
    a[1:3, 1:3, 1:3] = 1
    t = torch.from_numpy(a)
    bad_spacings = ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0),
                    (1.0, float("inf"), 1.0), 0.0, -2.0, float("inf"))
    for vs in bad_spacings:
        for fn in (surface_gpu.spaced_hd95, surface_gpu.spaced_asd, surface_gpu.spaced_pair_metrics):
            with pytest.raises(ValueError, match="voxelspacing"):
                fn(a, a, voxelspacing=vs)
        with pytest.raises(ValueError, match="voxelspacing"):
            surface_gpu.spaced_distances(t, t, (1,), voxelspacing=vs)
        with pytest.raises(ValueError, match="voxelspacing"):
            surface_gpu.spaced_metrics(t, t, (1,), voxelspacing=vs)
        for surface in ("host", "gpu"):
            with pytest.raises(ValueError, match="voxelspacing"):
                eval_surface.calculate_metric_percase_3d(a, a, surface=surface, voxelspacing=vs)
            with pytest.raises(ValueError, match="voxelspacing"):
                eval_surface.test_single_volume(a.astype(np.float32), a, None, 2, surface=surface, voxelspacing=vs)
            with pytest.raises(ValueError, match="voxelspacing"):
                eval_surface.test_all_case(None, [(a, a)], 2, surface=surface, voxelspacing=vs)
    for conn in (0, 4, -1, 1.5, None):
        with pytest.raises(ValueError, match="connectivity"):
            surface_gpu.spaced_hd95(a, a, connectivity=conn)
        with pytest.raises(ValueError, match="connectivity"):
            surface_gpu.spaced_metrics(t, t, (1,), connectivity=conn)
        for surface in ("host", "gpu"):
            with pytest.raises(ValueError, match="connectivity"):
                eval_surface.calculate_metric_percase_3d(a, a, surface=surface, connectivity=conn)
            with pytest.raises(ValueError, match="connectivity"):
                eval_surface.test_single_volume(a.astype(np.float32), a, None, 2, surface=surface, connectivity=conn)
            with pytest.raises(ValueError, match="connectivity"):
                eval_surface.test_all_case(None, [(a, a)], 2, surface=surface, connectivity=conn)
    # a 2-D map has two axes: two spacings, connectivity at most 2
    with pytest.raises(ValueError, match="voxelspacing"):
        surface_gpu.spaced_hd95(a[0], a[0], voxelspacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="connectivity"):
        surface_gpu.spaced_hd95(a[0], a[0], connectivity=3)
    for surface in ("host", "gpu"):
        with pytest.raises(ValueError, match="voxelspacing"):
            eval_surface.calculate_metric_percase_2d(a[1], a[1], surface=surface, voxelspacing=(1.0, 1.0, 1.0))
        with pytest.raises(ValueError, match="connectivity"):
            eval_surface.calculate_metric_percase_2d(a[1], a[1], surface=surface, connectivity=3)
    with pytest.raises(ValueError, match="voxelspacing"):
        surface_gpu.spaced_distances(t[:1], t[:1], (1,), voxelspacing=(1.0, 1.0, 1.0), ndim=2)
    for classes in ((1, 3), (2, 1), ()):
        with pytest.raises(ValueError, match="contiguous"):
            surface_gpu.spaced_metrics(t, t, classes, voxelspacing=2.0)
    with pytest.raises(ValueError, match="cap"):
        surface_gpu.spaced_records(t, t, (1,), cap=0)
    # the unit-spacing functions keep refusing both arguments
    with pytest.raises(ValueError, match="metrics.binary"):
        surface_gpu.hd95(a, a, voxelspacing=(1.0, 1.0, 2.5))
    with pytest.raises(ValueError, match="metrics.binary"):
        surface_gpu.asd(a, a, connectivity=2)
    # surface="host" with the two arguments is metrics.binary with them: no GPU needed
    b = np.roll(a, 1, 0)
    vs = (10.0, 1.25, 1.25)
    exp = (metrics.binary.dc(a, b), metrics.binary.jc(a, b), metrics.binary.hd95(a, b, vs, 2), metrics.binary.asd(a, b, vs, 2))
    assert eval_surface.calculate_metric_percase_3d(a, b, voxelspacing=vs, connectivity=2) == exp
    assert eval_surface.calculate_metric_percase_2d(a, b, voxelspacing=vs, connectivity=2) == exp
    assert eval_surface.calculate_metric_percase_3d(a, b) == eval_surface.calculate_metric_percase_3d(a, b, voxelspacing=None, connectivity=1)
    assert exp[2] != metrics.binary.hd95(a, b)
