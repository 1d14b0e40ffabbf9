"""Every entry point of csrc/loss_front.hip called DIRECTLY (arco_amd._lib), one kernel at a time, against a plain float64 / int64
reference on the CPU computed from the same input values (tests/loss_kernel_refs.py) - not through the loss chain, not against
another HIP route, not against golden files - at the edges the chain's random inputs never reach:

  exact (torch.equal)
  * arco_mask_codes (mask_codes_kernel + scan_counts_kernel), arco_compact_rows, arco_lv_weights: C 1 / 2 / 4 / 19 / 21, labeled
    and unlabeled images present or absent, n_pix 1 / 255 / 256 / 257 / 65 836 (258 blocks: the scan takes two blocks per thread and
    half its threads have an empty range), probabilities from four values (ties in > 20 % of the pixels, a pixel with all C equal,
    p == delta_p and p == delta_n), masks from {0, 0.5, 1}, low_rank / high_rank at 0, C and equal, every counter column zero in one
    case and nonzero in another, a block whose waves hold 0 / 1 / 63 / 64 bits, lists prefilled with a sentinel, Cp > C;
  * arco_anchor_pix (E 1 / 3 / 21, idx_stride > Q), arco_gather_rows(_h) (idx64 / idx32 / neither, with and without list, first > 0,
    n 0 / 1 / 3 / 4 / 5, D 4 / 16 / 260 / 496 and 6 (scalar path), ld_src > D, ld_out > D with untouched pad; misaligned strides are
    rejected on the host), arco_bank_append (empty bank, below / at / above the queue size, more new keys than the queue holds, no
    new key, D 1 / 16), arco_neg_multiplicity and the M of arco_nce_prep (torch.bincount; L 1 / 2 / 33 / 257, negative indices,
    ld > L, ragged lens, one row drawn 1 / 300 / 4097 times, zero pad columns), the LDS counters of arco_nce_fused (through W).

  per-element bounds k u sum|terms| (u = 2^-24; derivations in tests/loss_kernel_refs.py; worst err / bound: CPU emulation | GPU)
  * arco_masked_proto            0.20 | n/m    arco_weighted_row_sum   0.23 | n/m    arco_weighted_row_sum_h   0.22 | n/m
    (every lpr, both NDI, 2 and 3 class groups, ldt > D, ldo > D, 1 ... 1000 rows, the capped grids, an empty class: NaN | exact 0)
  * arco_normalize_rows          0.48 | n/m    arco_normalize_rows_pad 0.48 | n/m    arco_nce_normalize_banks  0.48 | n/m
    row half of arco_nce_prep    0.48 | n/m    (D 1 ... 496, Dp = D and padded, zero row, norms beside eps, zero pad)
  * arco_infonce_fwd             0.75 | n/m    arco_nce_fused          0.75 | n/m    arco_nce_score + finish   0.75 | n/m
    (Q 1 / 63 / 64 / 65, lens 1 ... 300 ragged, D 4 / 16 / 20 / 496, temp 0.05 / 0.5 / 4, cosines +1 / -1 / 0, a zero bank row, the
    deepest underflow of the fixed shift; loss, W = d loss / d S, gpos, loss_sum, Bt)
  * arco_infonce_anchor_grad     0.40 | n/m    arco_nce_anchor_grad    0.40 | n/m    arco_nce_anchor_grad_scaled 0.40 | n/m
  * arco_scatter_add_rows        0.42 | n/m    arco_sum_scale          0.14 | n/m
The emulation's figures are the largest printed by tests/test_loss_kernels_cpu.py.  n/m: not measured - this file has not yet run on
an MI355X; every test prints its worst err / bound, and the largest per kernel belongs in the GPU column."""
import ctypes

import pytest
import torch

import loss_kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    import arco_amd._lib as lib
    lib.load()
    return lib


def dev(t):
    return None if t is None else t.to(DEV)


def filled(shape, dtype=torch.float32, value=R.SENTINEL):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def report(name, ratio):
    print(f"{name}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


# ---- mask codes, scan, compaction, low-valid weights ---------------------------------------------------------------------------------
def run_mask_codes(L, c):
    C, n_pix, nb = c["C"], c["n_pix"], c["nblocks"]
    codes = filled((n_pix,), torch.int64, R.ISENT)
    counts = filled((3 * C * nb,), torch.int32, R.ISENT)
    offsets = filled((3 * C * nb,), torch.int32, R.ISENT)
    totals = filled((3 * C,), torch.int64, R.ISENT)
    keep = [dev(c[k]) for k in ("lab_l", "lab_u", "prob_l", "prob_u", "lowm", "highm")]
    L.call("arco_mask_codes", *[L.ptr(t) for t in keep], c["n_l"], c["n_u"], C, c["P"], R.DELTA_P, R.DELTA_N, c["low"], c["high"],
           L.ptr(codes), L.ptr(counts), L.ptr(offsets), L.ptr(totals))
    torch.cuda.synchronize()
    return codes, counts.view(3 * C, nb), offsets.view(3 * C, nb), totals


@pytest.mark.parametrize("i", range(len(R.MASK_CASES)), ids=lambda i: "C{}-l{}-u{}-P{}-lo{}-hi{}-{}".format(*R.MASK_CASES[i]))
def test_mask_codes_scan_compact_and_lv_weights(L, i):
    """codes, per-block counts, exclusive offsets, totals: exact.  Then, from the kernel's OWN codes and offsets: the 2 C row lists
    (prefix == torch.nonzero order of the reference mask, sentinel behind it) and the low-valid weight rows with Cp > C."""
    c = R.mask_case(i)
    C, n_pix = c["C"], c["n_pix"]
    codes, counts, offsets, totals = run_mask_codes(L, c)
    assert R.exact(codes, c["codes"])
    assert R.exact(counts, c["counts"]) and R.exact(offsets, c["offsets"]) and R.exact(totals, c["totals"])
    lists = filled((2 * C, n_pix), torch.int32, R.ISENT)
    L.call("arco_compact_rows", L.ptr(codes), n_pix, C, L.ptr(offsets), L.ptr(lists))
    assert R.lists_ok(lists, torch.cat((c["anchor"], c["neg"]), 0))
    for cp in (C, C + 3):
        W = filled((n_pix, cp))
        L.call("arco_lv_weights", L.ptr(codes), n_pix, C, cp, L.ptr(W))
        ref = torch.zeros((n_pix, cp))
        ref[:, :C] = c["lv"].t().float()
        assert R.exact(W, ref)


@pytest.mark.parametrize("E", (1, 3, 21))
def test_anchor_pix(L, E):
    """out[e Q + q] = lists[k[e]][idx_all[e idx_stride + q]] with idx_stride > Q (the production layout carries the negatives behind)"""
    Q, n_pix, stride = 5, 37, 5 + 11
    g = R.gen(11, E)
    lists = torch.randint(0, 1 << 20, (2 * E + 1, n_pix), generator=g, dtype=torch.int32)
    k = torch.randperm(2 * E + 1, generator=g)[:E]
    idx = torch.randint(0, n_pix, (E * stride,), generator=g)
    out = filled((E * Q + 2,), torch.int64, R.ISENT)
    dl, di = dev(lists), dev(idx)
    L.call("arco_anchor_pix", L.ptr(dl), n_pix, ints(k.tolist()), E, L.ptr(di), stride, Q, L.ptr(out))
    ref = torch.stack([lists[k[e]].long()[idx[e * stride:e * stride + Q]] for e in range(E)]).flatten()
    assert R.exact(out[:E * Q], ref) and bool((out[E * Q:] == R.ISENT).all())


# ---- gather, bank append ---------------------------------------------------------------------------------------------------------------
GATHER_D = (4, 16, 260, 496, 6)


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("D", GATHER_D)
def test_gather_rows(L, D, half):
    """out[j] = src[list ? list[i_j] : i_j], i_j = idx64[first + j] | idx32[first + j] | first + j; all three index forms with and without
    list, first = 2, n 0 / 1 / 3 / 4 / 5 (one block = four rows), ld_src > D, ld_out > D.  f16 rows widen exactly.  D = 6: scalar path."""
    g = R.gen(12, D, half)
    n_src, first = 23, 2
    vec = D % 4 == 0
    lds, ldo = D + (4 if vec else 1), D + (4 if vec else 3)
    src = torch.randn((n_src, lds), generator=g)
    src = src.half() if half else src
    lst = torch.randperm(n_src, generator=g).to(torch.int32)
    idx = torch.randint(0, n_src, (first + 5,), generator=g)
    d_src, d_lst, d64, d32 = dev(src), dev(lst), dev(idx), dev(idx.to(torch.int32))
    name = "arco_gather_rows_h" if half else "arco_gather_rows"
    for form in ("idx64", "idx32", "none"):
        for use_list in (False, True):
            for n in (0, 1, 3, 4, 5):
                out = filled((max(n, 1), ldo))
                L.call(name, L.ptr(d_src), lds, D, L.ptr(d_lst) if use_list else None, L.ptr(d64) if form == "idx64" else None,
                       L.ptr(d32) if form == "idx32" else None, first, n, L.ptr(out), ldo)
                rows = idx[first:first + n] if form != "none" else torch.arange(first, first + n)
                rows = lst.long()[rows] if use_list else rows
                assert R.exact(out[:n, :D], src[rows][:, :D].float()), (form, use_list, n)
                assert R.pad_ok(out[:n], D) and bool((out[n:] == R.SENTINEL).all()), (form, use_list, n)


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
def test_gather_rows_rejects_misaligned_vector_rows(L, half):
    """D % 4 == 0 takes 16-byte (f16: 8-byte) row accesses: strides that are no multiple of 4 elements and misaligned base pointers are
    argument errors - the call raises and nothing is launched (the output keeps its sentinel).  Every caller (rows_view, fresh
    tensors, channel offsets that are multiples of 16) satisfies the contract."""
    src = torch.zeros((8, 12), device=DEV, dtype=torch.float16 if half else torch.float32)
    out = filled((4, 12))
    name = "arco_gather_rows_h" if half else "arco_gather_rows"
    es = src.element_size()
    bad = [(L.ptr(src), 9, L.ptr(out), 12), (L.ptr(src), 12, L.ptr(out), 10),
           (ctypes.c_void_p(src.data_ptr() + es), 12, L.ptr(out), 12), (L.ptr(src), 12, ctypes.c_void_p(out.data_ptr() + 4), 12)]
    for (ps, lds, po, ldo) in bad:
        with pytest.raises(RuntimeError):
            L.call(name, ps, lds, 8, None, None, None, 0, 2, po, ldo)
    torch.cuda.synchronize()
    assert bool((out == R.SENTINEL).all())
    L.call(name, L.ptr(src), 9, 6, None, None, None, 0, 2, L.ptr(out), 10)          # the scalar path has no such contract
    flat = out.flatten()
    assert bool((flat[:6] == 0).all()) and bool((flat[10:16] == 0).all())


BANK_CASES = [(0, 5, 8), (3, 4, 8), (3, 5, 8), (6, 5, 8), (3, 12, 8), (5, 0, 8), (0, 9, 8), (8, 1, 8)]


@pytest.mark.parametrize("D", (1, 16))
@pytest.mark.parametrize("len_old,n,qs", BANK_CASES, ids=lambda v: str(v))
def test_bank_append(L, len_old, n, qs, D):
    """out = cat(old, keys)[-min(len_old + n, queue_size):]: empty bank | below | exactly at | above the queue size | more new keys than
    the queue holds (drop > len_old) | no new key | a full bank.  Rows behind the result keep the sentinel."""
    g = R.gen(13, len_old, n, D)
    old, keys = torch.randn((len_old, D), generator=g), torch.randn((n, D), generator=g)
    out = filled((qs + 1, D))
    d_old, d_keys = dev(old), dev(keys)
    L.call("arco_bank_append", L.ptr(d_old) if len_old else None, len_old, L.ptr(d_keys) if n else None, n, qs, D, L.ptr(out))
    ref = torch.cat((old, keys))[-min(len_old + n, qs):]
    m = ref.shape[0]
    assert R.exact(out[:m], ref) and bool((out[m:] == R.SENTINEL).all())


# ---- multiplicities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.MULT_CASES)), ids=lambda i: "L{}-Nn{}-pad{}".format(*R.MULT_CASES[i]))
def test_neg_multiplicity(L, i):
    """M[q][k] = number of times row k (negative indices + L) is drawn by query q == torch.bincount; pad columns zero; one row drawn Nn times"""
    c = R.mult_case(i)
    M = filled((3, c["ld"]), torch.int32, R.ISENT)
    d_idx = dev(c["idx"])
    L.call("arco_neg_multiplicity", L.ptr(d_idx), 3, c["nn"], c["L"], c["ld"], L.ptr(M))
    assert R.exact(M, c["ref"])


def run_prep(L, c, A, P, d, dp):
    """arco_nce_prep on the case's indices: returns An, invA, Pn, M (as int64)"""
    n, q, E = A.shape[0], c["q"], c["E"]
    An, invA, Pn = filled((n, dp)), filled((n,)), filled((P.shape[0], dp))
    M = filled((n, c["lp"]), torch.int16, R.ISENT)
    dA, dP, di = dev(A.contiguous()), dev(P.contiguous()), dev(c["idx_all"])
    L.call("arco_nce_prep", L.ptr(dA), n, L.ptr(dP), P.shape[0], d, dp, R.EPS, L.ptr(An), L.ptr(invA), L.ptr(Pn), ints(c["lens"]), E,
           L.ptr(di), q, c["stride"], q, c["nn"], c["lp"], L.ptr(M))
    torch.cuda.synchronize()
    return An, invA, Pn, M.cpu().long() & 0xffff


@pytest.mark.parametrize("i", range(len(R.NCE_CASES)), ids=lambda i: "Q{}-lens{}-D{}-T{}-Nn{}".format(*R.NCE_CASES[i]))
def test_nce_prep_multiplicities(L, i):
    """the 16-bit M rows of arco_nce_prep == torch.bincount over ragged lens, zero in every pad column l >= len[e] (odd and even lens:
    two counters per LDS word)"""
    c = R.nce_case(i)
    g = R.gen(14, i)
    A, P = torch.randn((c["E"] * c["q"], c["d"]), generator=g), torch.randn((c["n_p"], c["d"]), generator=g)
    assert c["lp"] <= L.query("arco_nce_max_len") == 2 * ((160 * 1024 - 512) // 4)      # 16-bit counters in <= 160 KB of LDS
    _, _, _, M = run_prep(L, c, A, P, c["d"], c["dp"])
    assert R.exact(M, c["M"].view(-1, c["lp"]))


# ---- row sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.PROTO_CASES)), ids=lambda i: "D{}-C{}-n{}-ldt+{}".format(*R.PROTO_CASES[i][:4]))
def test_masked_proto(L, i):
    c = R.proto_case(i)
    d, C, n = c["d"], c["C"], c["n"]
    ws = filled((L.query("arco_proto_ws_floats", n, C, d),))
    proto = filled((C + 1, d))
    dT, dc, dt = dev(c["T"]), dev(c["codes"]), dev(c["totals"])
    L.call("arco_masked_proto", L.ptr(dT), c["ldt"], L.ptr(dc), n, C, d, L.ptr(dt), L.ptr(ws), L.ptr(proto))
    if C > 1:
        assert bool(torch.isnan(proto[C - 1]).all())                   # the class without a pixel: 0 / 0
    assert bool((proto[C] == R.SENTINEL).all())
    report(f"arco_masked_proto k={c['k']}", R.worst(proto[:C], c["ref"], c["tol"]))


@pytest.mark.parametrize("half", (False, True), ids=("f32", "f16"))
@pytest.mark.parametrize("i", range(len(R.ROW_SUM_CASES)), ids=lambda i: "D{}-C{}-n{}-ldt+{}-ldo+{}-tot{}".format(*R.ROW_SUM_CASES[i]))
def test_weighted_row_sum(L, i, half):
    c = R.weighted_case(i, half)
    d, C, n = c["d"], c["C"], c["n"]
    ws = filled((L.query("arco_proto_ws_floats", n, C, d),))
    out = filled((C + 1, c["ldo"]))
    dT, dW, dt = dev(c["T"]), dev(c["W"]), dev(c["totals"])
    L.call("arco_weighted_row_sum_h" if half else "arco_weighted_row_sum", L.ptr(dT), c["ldt"], L.ptr(dW), c["ldw"], n, C, d, L.ptr(dt),
           L.ptr(ws), L.ptr(out), c["ldo"])
    assert R.pad_ok(out[:C], d) and bool((out[C] == R.SENTINEL).all())
    if C > 1:
        last = out[C - 1, :d]
        assert bool(torch.isnan(last).all()) if c["totals"] is not None else bool((last == 0).all())
    report(f"arco_weighted_row_sum{'_h' if half else ''} k={c['k']}", R.worst(out[:C, :d], c["ref"], c["tol"]))


# ---- normalisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.NORM_D)
def test_normalize_rows(L, D):
    """y, yt, inv each present or absent (all eight combinations, the empty one included), n 1 / 4 / 5, ldx > D, ldy > D (pad untouched),
    ldyt > n.  Zero row: exact 0 and inv == 1.0f / eps."""
    worst = 0.0
    for n in R.NORM_N:
        for combo in range(8):
            c = R.norm_case(D, n, combo)
            x = torch.full((n, D + 3), R.SENTINEL)
            x[:, :D] = c["x"]
            dx = dev(x)
            y = filled((n, D + 2)) if combo & 1 else None
            yt = filled((D, n + 1)) if combo & 2 else None
            inv = filled((n + 1,)) if combo & 4 else None
            L.call("arco_normalize_rows", L.ptr(dx), D + 3, n, D, R.EPS, L.ptr(y), D + 2, L.ptr(yt), n + 1, L.ptr(inv))
            zero = c["nrm"] == 0
            if y is not None:
                assert R.pad_ok(y, D) and bool((y.cpu()[zero][:, :D] == 0).all())
                worst = max(worst, R.worst(y[:, :D], c["y"], c["ytol"]))
            if yt is not None:
                assert R.pad_ok(yt, n)
                worst = max(worst, R.worst(yt[:, :n].t(), c["y"], c["ytol"]))
            if inv is not None:
                assert float(inv[n]) == R.SENTINEL and bool((inv.cpu()[:n][zero] == R.INV_EPS_F).all())
                worst = max(worst, R.worst(inv[:n], c["inv"], c["itol"]))
    report(f"arco_normalize_rows D={D}", worst)


@pytest.mark.parametrize("D", R.NORM_D)
def test_normalize_rows_pad_and_prep_rows(L, D):
    """arco_normalize_rows_pad (inv present and absent) and the row half of arco_nce_prep (An, invA, Pn) with Dp = D and Dp = the next
    multiple of 16: pad columns exactly 0, zero row exactly 0 with inv == 1.0f / eps, rows with norms beside eps."""
    w_pad = w_prep = 0.0
    for n in R.NORM_N:
        for dp in sorted({D, R.ceil_to(D, 16)}):
            c = R.norm_case(D, n, n + dp)
            zero = c["nrm"] == 0
            for with_inv in (True, False):
                x = torch.full((n, D + 1), R.SENTINEL)
                x[:, :D] = c["x"]
                dx = dev(x)
                y, inv = filled((n, dp + 1)), filled((n + 1,)) if with_inv else None
                L.call("arco_normalize_rows_pad", L.ptr(dx), D + 1, n, D, dp, R.EPS, L.ptr(y), dp + 1, L.ptr(inv))
                assert R.pad_ok(y, dp) and bool((y[:, D:dp] == 0).all()) and bool((y.cpu()[zero][:, :dp] == 0).all())
                w_pad = max(w_pad, R.worst(y[:, :D], c["y"], c["ytol"]))
                if with_inv:
                    assert bool((inv.cpu()[:n][zero] == R.INV_EPS_F).all()) and float(inv[n]) == R.SENTINEL
                    w_pad = max(w_pad, R.worst(inv[:n], c["inv"], c["itol"]))
            # arco_nce_prep: E = 1 entry of Q = n anchors, the same rows once more as 'prototypes'
            pc = dict(q=n, E=1, lens=[16], lp=16, nn=2, stride=n + 2 * n, idx_all=torch.zeros(3 * n, dtype=torch.int64))
            An, invA, Pn, M = run_prep(L, pc, c["x"], c["x"], D, dp)
            for got in (An, Pn):
                assert bool((got[:, D:] == 0).all()) and bool((got.cpu()[zero] == 0).all())
                w_prep = max(w_prep, R.worst(got[:, :D], c["y"], c["ytol"]))
            assert bool((invA.cpu()[zero] == R.INV_EPS_F).all())
            w_prep = max(w_prep, R.worst(invA, c["inv"], c["itol"]))
            assert bool((M[:, 0] == 2).all()) and bool((M[:, 1:] == 0).all())
    report(f"arco_normalize_rows_pad D={D}", w_pad)
    report(f"arco_nce_prep rows D={D}", w_prep)


@pytest.mark.parametrize("lp", R.BANK_LP)
@pytest.mark.parametrize("D", R.NORM_D)
def test_nce_normalize_banks(L, D, lp):
    """Bn [E][Lp][Dp] and Bt [E][Dp][Lp] (present and absent) over ragged lens 1 / 15 / 16 / 17 / Lp: rows >= len, pad columns and the
    Bt pad entries exactly 0; Bt is Bn transposed exactly."""
    c = R.banks_case(D, lp)
    E = len(c["lens"])
    d_banks = [dev(b) for b in c["banks"]]
    ptrs = (ctypes.c_void_p * E)(*[b.data_ptr() for b in d_banks])
    worst = 0.0
    for dp in sorted({D, R.ceil_to(D, 16)}):
        ref = torch.zeros((E, lp, dp), dtype=torch.float64)
        ref[:, :, :D] = c["bn"]
        tol = torch.zeros_like(ref)
        tol[:, :, :D] = c["tol"]
        for with_bt in (True, False):
            Bn, Bt = filled((E, lp, dp)), filled((E, dp, lp)) if with_bt else None
            L.call("arco_nce_normalize_banks", ptrs, ints(c["lens"]), E, D, dp, lp, R.EPS, L.ptr(Bn), L.ptr(Bt))
            worst = max(worst, R.worst(Bn, ref, tol))             # tol == 0 in pad rows / columns and zero rows: exact there
            if with_bt:
                assert torch.equal(Bt, Bn.transpose(1, 2))
    report(f"arco_nce_normalize_banks D={D} Lp={lp}", worst)


# ---- InfoNCE: three routes, one formula ----------------------------------------------------------------------------------------------
def nce_check(name, ref, tols, loss, W, gpos, M):
    """loss, W (exactly 0 where M == 0), gpos against the float64 formula; returns the worst ratio"""
    assert bool((W.cpu()[M == 0] == 0).all()), name
    r = max(R.worst(loss, ref["loss"], tols["loss"]), R.worst(W, ref["W"], tols["W"]), R.worst(gpos, ref["gpos"], tols["gpos"]))
    return r


NCE_IDS = ["Q{}-lens{}-D{}-T{}-Nn{}".format(*c) for c in R.NCE_CASES]


@pytest.mark.parametrize("i", range(len(R.NCE_CASES)), ids=NCE_IDS)
def test_infonce_fwd_and_nce_fused(L, i):
    """The two staged routes read the score matrix S (here: the float64 cosines rounded to fp32 - an exact input), so only pos, the
    softmax and the weights are theirs.  arco_infonce_fwd: per entry, M from arco_neg_multiplicity's format (uint32), a shared
    positive (ldp == 0) and one positive row per query (ldp == Dp); W is written for k < len only (pad keeps the sentinel).
    arco_nce_fused: all entries in one launch, LDS counters from the indices; W zero up to ld."""
    c = R.nce_case(i)
    E, q, lp, dp = c["E"], c["q"], c["lp"], c["dp"]
    s32 = c["cos"].float()
    ref = R.nce_ref(s32.double(), c["M"], c["pos"], c["temp"])
    assert bool(torch.isfinite(ref["loss"]).all())
    e_s, e_pos = R.staged_logit_errors(c, s32, ref)
    tols = R.nce_tols(ref, e_s, e_pos, R.staged_round_mag(ref))
    S, An, Pn = dev(s32), dev(c["An"]), dev(c["Pn"])
    w_fwd = 0.0
    for e, l in enumerate(c["lens"]):
        sub = {k: v[e] for k, v in ref.items() if torch.is_tensor(v)}
        subt = {k: v[e] for k, v in tols.items()}
        Md = dev(c["M"][e].to(torch.int32))
        for ldp in (0, dp):
            pn = Pn[c["prow"][e]].repeat(q if ldp else 1, 1).contiguous()
            W, gpos, loss = filled((q, lp)), filled((q,)), filled((q,))
            L.call("arco_infonce_fwd", L.ptr(S[e]), lp, L.ptr(Md), l, L.ptr(An[e * q:]), L.ptr(pn), ldp, q, dp, c["temp"], L.ptr(W),
                   L.ptr(gpos), L.ptr(loss))
            assert R.pad_ok(W, l)
            w_fwd = max(w_fwd, nce_check("fwd", {k: v[:, :l] if v.dim() == 2 else v for k, v in sub.items()},
                                         {k: v[:, :l] if v.dim() == 2 else v for k, v in subt.items()}, loss, W[:, :l], gpos, c["M"][e][:, :l]))
    report("arco_infonce_fwd", w_fwd)
    di = dev(c["idx_all"])
    W, gpos, loss = filled((E, q, lp)), filled((E * q,)), filled((E * q,))
    L.call("arco_nce_fused", L.ptr(S), lp, ints(c["lens"]), ints(c["prow"]), E, L.ptr(di), q, c["stride"], q, c["nn"], L.ptr(An), L.ptr(Pn),
           dp, c["temp"], L.ptr(W), L.ptr(gpos), L.ptr(loss))
    report("arco_nce_fused", nce_check("fused", ref, tols, loss.view(E, q), W, gpos.view(E, q), c["M"]))
    loss2, gpos2 = filled((E * q,)), filled((E * q,))                     # W == NULL: no gradient wanted
    L.call("arco_nce_fused", L.ptr(S), lp, ints(c["lens"]), ints(c["prow"]), E, L.ptr(di), q, c["stride"], q, c["nn"], L.ptr(An), L.ptr(Pn),
           dp, c["temp"], None, L.ptr(gpos2), L.ptr(loss2))
    assert torch.equal(loss2, loss) and torch.equal(gpos2, gpos)


@pytest.mark.parametrize("i", range(len(R.NCE_CASES)), ids=NCE_IDS)
def test_nce_score_and_finish(L, i):
    """The MFMA score GEMM with the softmax-CE in its epilogue, then arco_nce_finish: Q, L and Dp that are no multiples of the
    64 x 128 x 16 tiles, one K chunk | a ragged last chunk (D 20 in Dp 32) | 31 chunks, Bt emitted and Bt == NULL.  pos, loss,
    gpos, loss_sum and the weights gscale * Wu * max(||b||, eps) = d loss / d S against the same float64 formula; Wu exactly 0 where
    M == 0 and in the pad columns; Bt == the raw bank transposed, zero pad.  temp 0.05 is the boundary at which _contrast.py still
    takes this route: the all-cosines -1 query is exp(-40) per term, far above the fp32 underflow."""
    c = R.nce_case(i)
    E, q, lp, dp, d = c["E"], c["q"], c["lp"], c["dp"], c["d"]
    ref = R.nce_ref(c["cos"], c["M"], c["pos"], c["temp"])
    e_s, e_pos, k_ib = R.score_logit_errors(c, ref)
    tols = R.nce_tols(ref, e_s, e_pos, R.score_round_mag(ref), extra_rel=R.gamma(k_ib) + 4 * R.U)
    banks = [dev(b) for b in c["banks"]]
    ptrs = (ctypes.c_void_p * E)(*[b.data_ptr() for b in banks])
    An, Pn, M = dev(c["An"]), dev(c["Pn"]), dev(c["M"].view(-1, lp).to(torch.int16))
    n_lt = int(L.query("arco_nce_score_ltiles", lp))
    scale = 1.0 / (q * 3)
    outs = []
    for with_bt in (True, False):
        Wu, Zp, pos = filled((E, q, lp)), filled((E * q, n_lt)), filled((E * q,))
        Bt = filled((E, dp, lp)) if with_bt else None
        L.call("arco_nce_score", L.ptr(An), dp, d, ptrs, ints(c["lens"]), ints(c["prow"]), E, lp, q, L.ptr(M), L.ptr(Pn), c["temp"], R.EPS,
               L.ptr(Wu), L.ptr(Zp), L.ptr(pos), L.ptr(Bt))
        gpos, gscale, loss, lsum = filled((E * q,)), filled((E * q,)), filled((E * q,)), filled((2,))
        L.call("arco_nce_finish", L.ptr(pos), E * q, L.ptr(Zp), lp, c["temp"], scale, L.ptr(gpos), L.ptr(gscale), L.ptr(loss), L.ptr(lsum))
        outs.append((Wu, pos, gpos, gscale, loss, lsum))
        if with_bt:
            bt = torch.zeros((E, dp, lp))
            for e, b in enumerate(c["banks"]):
                bt[e, :d, :b.shape[0]] = b.t()
            assert R.exact(Bt, bt)
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                          # Bt or not: the same numbers
    Wu, pos, gpos, gscale, loss, lsum = outs[0]
    assert bool((Wu.cpu()[c["M"] == 0] == 0).all()) and float(lsum[1]) == R.SENTINEL
    t = ref["t"]
    report("arco_nce_score pos", R.worst(pos.view(E, q), c["pos"], e_pos * t + R.TINY))
    W = gscale.cpu().double().view(E, q, 1) * Wu.cpu().double() * c["bnorm"].unsqueeze(1)
    report("arco_nce_score + arco_nce_finish", nce_check("score", ref, tols, loss.view(E, q), W, gpos.view(E, q), c["M"]))
    want = ref["loss"].sum() * scale
    report("arco_nce_finish loss_sum", R.worst(lsum[:1], want.view(1), tols["loss"].sum() * scale + 2 * R.U * want.abs()))


# ---- anchor gradients ----------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, 4, 16), (4, 16, 16), (5, 20, 32), (5, 496, 496), (4, 65, 80)]


@pytest.mark.parametrize("n,d,dp", GRAD_SHAPES)
def test_anchor_grads(L, n, d, dp):
    """float64 autograd of A -> scale <A / max(||A||, eps), G_total> with a zero row, a row of norm eps / 2 (both clamped: g / eps) and a
    row just above eps.  arco_infonce_anchor_grad: rows of Dp floats, ldp == 0 (shared positive) and ldp == Dp; arco_nce_anchor_grad
    and _scaled: E entries of Q rows (n = E Q), Dp > D, ld_dA > D with untouched pad, scale 0.375."""
    w1 = w2 = w3 = 0.0
    for shared in (True, False):
        c = R.grad_case(n, d, dp, shared)
        prow = torch.zeros(n, dtype=torch.int64) if shared else torch.arange(n)
        ref, tol = R.grad_ref(c, prow, False)
        G, An, Pn, gp, inv = (dev(c[k]) for k in ("G", "An", "Pn", "gpos", "inv"))
        dA = filled((n + 1, dp))
        L.call("arco_infonce_anchor_grad", L.ptr(G), L.ptr(An), L.ptr(Pn), 0 if shared else dp, L.ptr(gp), L.ptr(inv), n, dp, R.EPS,
               c["scale"], L.ptr(dA))
        assert bool((dA[n] == R.SENTINEL).all())
        w1 = max(w1, R.worst(dA[:n, :d], ref, tol))
    # grouped: E entries of Q rows, prototype row per entry
    for (E, q) in {(1, n), (n, 1)}:
        c = R.grad_case(n, d, dp, False, seed=E)
        pr = torch.randperm(n, generator=R.gen(15, n, E))[:E]
        prow = pr.repeat_interleave(q)
        G, An, Pn, gp, inv, gs = (dev(c[k]) for k in ("G", "An", "Pn", "gpos", "inv", "gscale"))
        for scaled in (False, True):
            ref, tol = R.grad_ref(c, prow, scaled)
            dA = filled((n, d + 3))
            if scaled:
                L.call("arco_nce_anchor_grad_scaled", L.ptr(G), L.ptr(An), L.ptr(Pn), ints(pr.tolist()), E, L.ptr(gp), L.ptr(inv), L.ptr(gs),
                       q, d, dp, R.EPS, c["scale"], L.ptr(dA), d + 3)
                w3 = max(w3, R.worst(dA[:, :d], ref, tol))
            else:
                L.call("arco_nce_anchor_grad", L.ptr(G), L.ptr(An), L.ptr(Pn), ints(pr.tolist()), E, L.ptr(gp), L.ptr(inv), q, d, dp, R.EPS,
                       c["scale"], L.ptr(dA), d + 3)
                w2 = max(w2, R.worst(dA[:, :d], ref, tol))
            assert R.pad_ok(dA, d)
    report("arco_infonce_anchor_grad", w1)
    report("arco_nce_anchor_grad", w2)
    report("arco_nce_anchor_grad_scaled", w3)


# ---- scatter-add, loss sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_list", (False, True), ids=("direct", "list"))
@pytest.mark.parametrize("d,n,m", [(1, 0, 0), (4, 1, 1), (65, 9, 3), (16, 130, 64)])
def test_scatter_add_rows(L, d, n, m, use_list):
    """dst[list ? list[idx[j]] : idx[j]] += a src[j], a = alpha or alpha * alpha_dev[0]; duplicate destinations with multiplicity up to
    64 (atomics, any order): (m + 1) u sum|terms|.  ld_src > D, ld_dst > D with untouched pad, n == 0 leaves dst as it was."""
    c = R.scatter_case(d, n, m, use_list)
    worst = 0.0
    for adev in (None, 3.0):
        a = 0.5 * (adev or 1.0)
        ref, tol = R.scatter_ref(c, a)
        dst, src, idx, lst = dev(c["dst"].clone()), dev(c["src"]), dev(c["idx"]), dev(c["list"])
        ad = torch.tensor([adev], device=DEV) if adev else None
        L.call("arco_scatter_add_rows", L.ptr(src) if n else None, d + 4, d, L.ptr(lst) if use_list else None, L.ptr(idx) if n else None, n,
               L.ptr(ad), 0.5, L.ptr(dst), d + 3)
        assert R.pad_ok(dst, d)
        if n == 0:
            assert R.exact(dst, c["dst"])
        worst = max(worst, R.worst(dst[:, :d], ref, tol))
    report(f"arco_scatter_add_rows m={c['mult']}", worst)


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("n", R.SUM_N)
def test_sum_scale(L, n, accumulate):
    """out = (accumulate ? out : 0) + scale * sum x, the sum in double: values of both signs that cancel, 2 u |result| + u |out_before|"""
    c = R.sum_case(n)
    out = torch.tensor([c["before"], R.SENTINEL], device=DEV)
    x = dev(c["x"])
    L.call("arco_sum_scale", L.ptr(x), n, c["scale"], L.ptr(out), accumulate)
    ref, tol = R.sum_ref(c, accumulate)
    assert float(out[1]) == R.SENTINEL
    report(f"arco_sum_scale n={n}", R.worst(out[:1], ref, tol))
