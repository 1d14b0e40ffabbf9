"""CPU companion of tests/test_row2d_kernels_gpu.py: what makes that file trustworthy on a machine without a GPU.
  * the toleranced comparisons: the kernels' formulas emulated in fp32 (numpy float32 index arithmetic, torch fp32 values; once with
    every operation rounded and once with every product-sum fused, the two extremes the compiler may choose between) stay inside the
    SAME per-element bound against the SAME float64 reference of tests/row2d_kernel_refs.py; the worst ratios are printed, and the
    largest per kernel is recorded in the GPU file's docstring;
  * the case tables cover the listed edges and the inputs hold the conditions the GPU file relies on;
  * the comparisons reject planted errors: corner rows swapped, ly and lx swapped, an inf let through the saturating cast, a tie
    rounded away from even, a row zeroed that no index names, the diagonal's 1 dropped from the fold, a term dropped from the sum.
The host-side rejections of these entry points are in tests/test_side_kernels_cpu.py::test_argument_checks_reject_on_the_host."""
import math

import numpy as np
import pytest
import torch

import row2d_kernel_refs as R2
import side_kernel_refs as R
from loss_kernel_refs import exact, worst


def report(name, ratio):
    print(f"emulated {name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("i", range(len(R2.ROW2D_CASES)))
def test_row2d_bound_holds_for_the_emulation(i):
    c = R2.row2d_case(i)
    if c["Clo"]:
        for fused in (False, True):
            report(f"row2d blend case {i} fused {fused}", worst(R2.emu_rows2d(c, fused), c["ref_lo"], c["tol_lo"]))
        if c["lo"] == c["hi"]:                                                # the identity: weights 0 / 1, bit for bit
            assert exact(R2.emu_rows2d(c, False), c["LO2"][c["pix"]])
    assert exact(c["hi16_rows"], c["HI162"][c["pix"]].float())
    # the corner rows and (ly, lx) ARE what arco_up_neighbors is held to (tests/test_side_kernels_gpu.py::test_up_neighbors)
    r_coord, r_sum, inside = R.corner_property(c["cn"]["idx"], c["cn"]["w"], c["cn"])
    assert inside and r_coord <= 1.0 and r_sum <= 1.0


def test_case_tables_cover_the_listed_edges():
    t = R2.ROW2D_CASES
    assert {c[1] for c in t} == {0, 4, 12, 260} and {c[2] for c in t} == {0, 4, 8, 12}
    assert {c[0] for c in t} == set(range(len(R.RATIOS_2D))) and {c[3] % 4 for c in t} == {0, 1, 2, 3} and 1 in {c[3] for c in t}
    assert {c[4] for c in t} == {0, 8} and {c[5] for c in t} == {0, 4} and all(c[5] <= c[4] for c in t)
    for i, cs in enumerate(t):
        c = R2.row2d_case(i)
        pix, hi = c["pix"], c["hi"]
        vol = hi[0] * hi[1]
        assert int(pix.min()) >= 0 and int(pix.max()) < R.NV * vol and pix.numel() == cs[3]
        if cs[3] > 2:                                                         # every border pixel of every image, and duplicates
            assert {img * vol + p for img in range(R.NV) for p in R2.border_pixels(hi)} <= set(pix.tolist())
            assert int(torch.bincount(pix).max()) >= 64
    u = R2.UTIL_CASES
    assert {c[1] for c in u} == {4, 12, 260} and {c[3] for c in u} >= {0, 1} and any(c[2] for c in u)
    assert any(c[3] * (c[1] // 4) == 4096 * 256 + 1 for c in u)
    for i, cs in enumerate(u):
        idx = R2.util_idx(i)
        assert idx.numel() == cs[3] and (cs[3] == 0 or (int(idx.min()) >= 0 and int(idx.max()) < cs[0]))
        assert idx.unique().numel() < cs[0]                                   # at least one row stays unnamed
        assert cs[3] < 4 or idx.unique().numel() < idx.numel()                # duplicates
    assert R2.CAST_SCALES == (1.0, 1024.0, 65536.0)
    assert {c[0] for c in R2.FOLD_CASES} == {2, 3, 17, 1025} and all((n, 1) in R2.FOLD_CASES and (n, n - 1) in R2.FOLD_CASES for n in (2, 3, 17, 1025))
    assert 1025 * 1025 > 4096 * 256 >= 1024 * 1024
    assert R2.COMBINE_N == tuple(range(1, 9))


@pytest.mark.parametrize("scale", R2.CAST_SCALES)
def test_cast_inputs_hold_their_conditions(scale):
    c = R2.cast_case(2, scale)
    y = c["ref"][c["named"]].float()
    x = c["X"][c["named"]]
    fin = y[torch.isfinite(y)]
    assert float(fin.abs().max()) == 65504.0 and bool(torch.isnan(y).any()) and not bool(torch.isinf(y).any())
    assert bool(torch.isinf(x).any()) and bool(((y != 0) & (y.abs() < 2.0 ** -14)).any())                     # inf in, subnormals out
    assert bool((torch.signbit(y) & (y == 0)).any())                                                          # -0.0 stays -0.0
    s = R2.cast_specials(scale)
    out = (s * scale).clamp(-65504.0, 65504.0).half().float()
    want = {2.0 ** -25: 0.0, 3 * 2.0 ** -25: 2.0 ** -23, 1 + 2.0 ** -11: 1.0, 1 + 3 * 2.0 ** -11: 1 + 2.0 ** -9, 2049.0: 2048.0, -2051.0: -2052.0,
            65519.996: 65504.0, 65520.0: 65504.0}
    for v, w in want.items():                                                 # round to nearest even at the ties, saturation above
        k = int((s * scale == torch.tensor(v, dtype=torch.float32)).nonzero()[0])
        assert float(out[k]) == w, (v, float(out[k]), w)
    assert bool((~c["named"]).any()) and bool((c["ref"][~c["named"]] == R.SENTINEL).all())


def test_fold_and_combine_references():
    for i in range(len(R2.FOLD_CASES)):
        c = R2.fold_case(i)
        n, k = c["n"], c["c"]
        full = torch.cat((c["lo"], c["hi"]), 1)
        off = ~torch.eye(n, dtype=torch.bool)                                 # a copy off the diagonal, one rounding of w + 1 on it
        assert exact(full[off], c["W"][off])
        d64 = c["W"].diagonal().double() + 1.0
        assert worst(full.diagonal(), d64, 2.0 ** -24 * d64.abs() + 1e-300) <= 1.0
        assert exact(c["dW"][:, :k], c["dlo"]) and exact(c["dW_nolo"][:, k:], c["dhi"]) and bool((c["dW_nolo"][:, :k] == 0).all())
    for n in R2.COMBINE_N:
        c = R2.combine_case(n)
        for fused in (False, True):
            report(f"combine_terms n {n} fused {fused}", worst(R2.emu_combine(c, fused), c["ref"], c["tol"]))
        assert worst(c["grads"], c["grads64"], 2.0 ** -24 * c["grads64"].abs() + 1e-300) <= 1.0
        assert bool((c["w"] < 0).any()) == (n >= 3)
        if n >= 2:
            assert float(c["w"][0] * c["t"][0] + c["w"][1] * c["t"][1]) == 0.0


def test_comparisons_reject_planted_errors():
    c = R2.row2d_case(2)                                                      # non-integer upsampling, 12 channels
    n, Clo = c["n"], c["Clo"]
    good = R2.emu_rows2d(c, False)
    assert worst(good, c["ref_lo"], c["tol_lo"]) <= 1.0
    bad = dict(c)
    bad["V"] = c["V"].view(n, 4, Clo)[:, [0, 2, 1, 3]].reshape(4 * n, Clo)    # corner rows 01 and 10 swapped
    assert worst(R2.emu_rows2d(bad, False), c["ref_lo"], c["tol_lo"]) > 1e3
    ax = c["cn"]["ax"]
    bad = dict(c)
    bad["cn"] = dict(c["cn"], ax=[ax[1], ax[0]])                              # ly and lx swapped
    assert worst(R2.emu_rows2d(bad, False), c["ref_lo"], c["tol_lo"]) > 1e3
    one = good.clone()
    one[n // 2, Clo - 1] += 1e-4
    assert worst(one, c["ref_lo"], c["tol_lo"]) > 1.0 and not R.bits_equal(one, good)
    cs = R2.cast_case(2, 1024.0)
    wrong = cs["ref"].clone()
    r, k = (torch.isinf(cs["X"]) & cs["named"].view(-1, 1)).nonzero()[0].tolist()
    wrong[r, k] = math.inf                                                    # an inf let through instead of +-65504
    assert R.same_or_nan(cs["ref"].clone(), cs["ref"]) and not R.same_or_nan(wrong, cs["ref"])
    wrong = cs["ref"].clone()
    tie = ((cs["X"] * 1024.0 == 1 + 2.0 ** -11) & cs["named"].view(-1, 1)).nonzero()
    assert tie.numel()
    wrong[tie[0, 0], tie[0, 1]] = 1 + 2.0 ** -10                              # the tie rounded away from even
    assert not R.same_or_nan(wrong, cs["ref"])
    z = R2.zero_case(2, False)
    wrong = z["ref"].clone()
    unnamed = [r for r in range(z["M"]) if r not in set(z["idx"].tolist())][0]
    wrong[unnamed] = 0                                                        # a row zeroed that no index names
    assert not exact(wrong, z["ref"])
    f = R2.fold_case(3)
    assert not exact(f["W"][:, :f["c"]].contiguous(), f["lo"])                # the diagonal's 1 dropped
    cc = dict(R2.combine_case(5))
    assert worst(R2.emu_combine(cc, False), cc["ref"], cc["tol"]) <= 1.0
    cc["n"] = 4                                                               # the last term dropped
    assert worst(R2.emu_combine(cc, False), cc["ref"], cc["tol"]) > 1e3
