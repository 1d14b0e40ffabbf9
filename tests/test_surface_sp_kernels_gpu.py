"""Surface-distance kernels with a voxel spacing and a connectivity (arco_amd/csrc/surface.hip) on the GPU against the brute force of
tests/surface_sp_kernel_refs.py, which restates the kernels' operation order: the records, grouped by tag and sorted, are array_equal
as float64 squared distances (tests/test_surface_sp_kernels_cpu.py holds that brute force to scipy).  hd95 / asd finished from them are
held to metrics.binary with the same arguments at rtol 1e-12: per distance the two differ by at most REL_SCIPY = 4 * 2^-52 (derived
in the refs module); the mean and the percentile are one numpy pairwise sum and one linear interpolation over at most a few thousand
such values."""
import numpy as np
import pytest
import torch

import surface_sp_kernel_refs as S
from arco_amd.utils import metrics

pytestmark = pytest.mark.gpu

COMBOS = S.combos()


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def _maps(c):
    return torch.tensor(c["pred"]).cuda(), torch.tensor(c["gt"]).cuda()


@pytest.mark.parametrize("name,sp,conn", COMBOS)
def test_records_exact_and_guards_intact(L, name, sp, conn):
    c = S.case(name)
    nc = len(c["classes"])
    ref = S.brute_records(name, sp, conn)
    total = sum(v.size for v in ref.values())
    n, val, tag, bufs = S.run_guarded(L, name, sp, conn)
    for buf, size in bufs:
        assert S.guards_intact(buf, size)
    assert n == total == val.size == tag.size
    first = S.group(val, tag, nc)
    assert S.exact(first, ref)
    n2, val2, tag2, _ = S.run_guarded(L, name, sp, conn)                 # a second call: the identical sorted records
    assert n2 == n and S.exact(S.group(val2, tag2, nc), first)


@pytest.mark.parametrize("name,sp,conn", [("3d_14x12x10", "2.9_0.7_1.3", 2), ("nearest_by_index", "10_1.25_1.25", 1)])
def test_cap_smaller_than_needed(L, name, sp, conn):
    from arco_amd.utils import surface_gpu
    c = S.case(name)
    ref = S.brute_records(name, sp, conn)
    total = sum(v.size for v in ref.values())
    cap = max(total // 2, 1)
    assert 1 <= cap < total
    n, val, tag, bufs = S.run_guarded(L, name, sp, conn, cap=cap)
    assert n == total                                                    # the true count
    for buf, size in bufs:
        assert S.guards_intact(buf, size)                                # nothing written past cap
    assert val.size == tag.size == cap
    # what was written is a sub-multiset of the reference's records
    every = {k: v.tolist() for k, v in ref.items()}
    for v, t in zip(val.tolist(), tag.tolist()):
        every[(t // 2, t % 2)].remove(v)
    p, g = _maps(c)
    vs = S.spacing_for(sp, c["ndim"])
    with pytest.raises(RuntimeError, match="do not fit"):
        surface_gpu.spaced_records(p, g, c["classes"], vs, conn, cap=cap)
    v_all, t_all = surface_gpu.spaced_records(p, g, c["classes"], vs, conn, cap=total)      # exactly enough is enough
    assert S.exact(S.group(v_all, t_all, len(c["classes"])), ref)


@pytest.mark.parametrize("name,sp,conn", COMBOS)
def test_spaced_metrics_match_host(name, sp, conn):
    from arco_amd.utils import surface_gpu
    c = S.case(name)
    p, g = _maps(c)
    vs = S.spacing_for(sp, c["ndim"])
    ref = S.brute_records(name, sp, conn)
    dist = surface_gpu.spaced_distances(p, g, c["classes"], vs, conn)
    got = surface_gpu.spaced_metrics(p, g, c["classes"], vs, conn)
    assert len(got) == len(dist) == len(c["classes"])
    for i, (k, m) in enumerate(zip(c["classes"], got)):
        d0, d1 = dist[i]
        assert d0.dtype == d1.dtype == np.float64
        assert np.array_equal(d0, np.sqrt(ref[(i, 0)])) and np.array_equal(d1, np.sqrt(ref[(i, 1)]))
        if k in c["empty"]:
            assert m is None and d0.size == d1.size == 0                 # a class absent from either map
            continue
        hd, asd = m
        assert hd == float(np.percentile(np.hstack((d0, d1)), 95)) and asd == float(d0.mean())
        np.testing.assert_allclose(hd, metrics.binary.hd95(c["pred"] == k, c["gt"] == k, vs, conn), rtol=1e-12, atol=0)
        np.testing.assert_allclose(asd, metrics.binary.asd(c["pred"] == k, c["gt"] == k, vs, conn), rtol=1e-12, atol=0)
    assert surface_gpu.spaced_metrics(p, g, c["classes"], vs, conn) == got                    # repeated calls are bit-identical


@pytest.mark.parametrize("name", S.CASES)
def test_unit_spacing_agrees_with_the_integer_route(name):
    from arco_amd.utils import surface_gpu
    c = S.case(name)
    p, g = _maps(c)
    ints = surface_gpu.surface_metrics(p, g, c["classes"])
    for vs in (None, 1.0, (1.0,) * c["ndim"]):
        got = surface_gpu.spaced_metrics(p, g, c["classes"], vs, 1)
        for k, a, b in zip(c["classes"], got, ints):
            if k in c["empty"]:
                assert a is None and b is None
                continue
            assert a[0] == b[0]                                          # hd95: the same multiset of sqrt(integer)
            np.testing.assert_allclose(a[1], b[1], rtol=1e-12, atol=0)


def test_planted_answers():
    from arco_amd.utils import surface_gpu
    c = S.case("nearest_by_index")
    p, g = _maps(c)
    (d0, d1), = surface_gpu.spaced_distances(p, g, (1,), (10.0, 1.0, 1.0), 1)
    assert d0.tolist() == [3.0] and d1.tolist() == [3.0, 10.0]           # 3 mm along x, not the 10 mm of the voxel next along z
    c = S.case("diagonal_holes")
    p, g = _maps(c)
    sizes = [surface_gpu.spaced_distances(p, g, (1,), None, conn)[0][0].size for conn in (1, 2, 3)]
    assert sizes == [len(S.border_points("diagonal_holes", "pred", 1, conn)) for conn in (1, 2, 3)] and sizes[0] < sizes[1] < sizes[2]


def test_ndim_says_which_axes_have_neighbours():
    from arco_amd.utils import surface_gpu
    c = S.case("2d_24x20")
    p, g = _maps(c)
    vs = (2.9, 0.7)
    flat = surface_gpu.spaced_distances(p, g, c["classes"], vs, 2)
    lifted = surface_gpu.spaced_distances(p[None], g[None], c["classes"], vs, 2, ndim=2)      # [1, H, W] with ndim 2 is the 2-D map
    for a, b in zip(flat, lifted):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # as a one-slice volume every voxel is a border voxel (its z neighbours lie outside): metrics.binary on the 3-D array
    vol = surface_gpu.spaced_metrics(p[None], g[None], c["classes"], (5.0, 2.9, 0.7), 1)
    for k, m in zip(c["classes"], vol):
        np.testing.assert_allclose(m[0], metrics.binary.hd95(c["pred"][None] == k, c["gt"][None] == k, (5.0, 2.9, 0.7), 1), rtol=1e-12)
        np.testing.assert_allclose(m[1], metrics.binary.asd(c["pred"][None] == k, c["gt"][None] == k, (5.0, 2.9, 0.7), 1), rtol=1e-12)


def test_single_pair_functions():
    from arco_amd.utils import surface_gpu
    c = S.case("3d_14x12x10")
    a, b = c["pred"] == 1, c["gt"] == 1
    vs = (10.0, 1.25, 1.25)
    np.testing.assert_allclose(surface_gpu.spaced_hd95(a, b, vs, 3), metrics.binary.hd95(a, b, vs, 3), rtol=1e-12, atol=0)
    np.testing.assert_allclose(surface_gpu.spaced_asd(a, b, vs, 3), metrics.binary.asd(a, b, vs, 3), rtol=1e-12, atol=0)
    np.testing.assert_allclose(surface_gpu.spaced_asd(b, a, 2.0), metrics.binary.asd(b, a, 2.0), rtol=1e-12, atol=0)
    lab_p, lab_g = _maps(c)                                              # label maps count as `> 0`; device tensors are taken as they are
    np.testing.assert_allclose(surface_gpu.spaced_pair_metrics(lab_p, lab_g, vs, 2),
                               (metrics.binary.hd95(c["pred"] > 0, c["gt"] > 0, vs, 2), metrics.binary.asd(c["pred"] > 0, c["gt"] > 0, vs, 2)),
                               rtol=1e-12, atol=0)
    empty = np.zeros_like(a)
    for fn in (surface_gpu.spaced_hd95, surface_gpu.spaced_asd):
        with pytest.raises(RuntimeError, match="first supplied array does not contain any binary object"):
            fn(empty, b, vs)
        with pytest.raises(RuntimeError, match="second supplied array does not contain any binary object"):
            fn(a, empty, vs)
