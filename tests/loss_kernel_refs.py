"""Inputs, float64 references, per-element tolerances and comparison helpers shared by tests/test_loss_kernels_gpu.py (the HIP kernels
of csrc/loss_front.hip, one entry point at a time) and tests/test_loss_kernels_cpu.py (the same bounds held against an fp32 emulation
of every kernel formula, the input conditions, and planted errors).  Plain CPU torch only; nothing here touches a GPU.

Every reference is float64 (int64 for the integer kernels) computed from the SAME fp32 / f16 input values the kernel reads.  Every
bound is per element, k * u * sum|terms| with u = 2^-24 and k the longest fp32 rounding chain read off the kernel (gamma(k) =
k u / (1 - k u) is used so that the first-order bound is a true bound); the derivations stand beside the tolerance functions."""
import functools
import math

import torch

U = 2.0 ** -24
EPS = 1e-8                                            # torch.cosine_similarity eps (arco_amd/_contrast.py)
EPS_F = float(torch.tensor(EPS, dtype=torch.float32))   # the value the kernels see (eps travels as a C float)
INV_EPS_F = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(EPS, dtype=torch.float32))    # 1.0f / eps in fp32
TINY = 1e-300
MAXC = 21                                             # ARCO_MAXC; code bits: LV c, ANCHOR 21 + c, NEG 42 + c
SENTINEL = -7.25                                      # prefill of every float output buffer: untouched pad must keep it
ISENT = -7                                            # ... and of every integer output buffer


def gamma(k):
    return k * U / (1.0 - k * U)


def ceil_to(x, m):
    return (x + m - 1) // m * m


def gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ---- comparison helpers (each is shown to reject a planted error in the CPU file) ----------------------------------------------------
def worst(got, ref, tol):
    """max over the elements of |got - ref| / tol, per ELEMENT.  Where ref is NaN, got must be NaN (counts as 0); a NaN anywhere else,
    or any deviation where tol is 0, is infinite."""
    got, ref = got.detach().double().cpu(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64) + torch.zeros_like(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    both_nan = torch.isnan(ref) & torch.isnan(got)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(both_nan, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max())


def exact(got, ref):
    """torch.equal on the CPU after bringing both to one integer / float type (no tolerance)."""
    got = got.detach().cpu()
    return got.shape == ref.shape and torch.equal(got, ref.to(got.dtype))


def lists_ok(lists, masks, sentinel=ISENT):
    """lists [K][n] (prefilled with `sentinel`): row k must start with torch.nonzero(masks[k]) in order and keep the sentinel behind it."""
    lists = lists.detach().cpu()
    for k in range(masks.shape[0]):
        want = torch.nonzero(masks[k]).flatten().to(lists.dtype)
        m = int(want.shape[0])
        if not torch.equal(lists[k, :m], want) or not bool((lists[k, m:] == sentinel).all()):
            return False
    return True


def pad_ok(buf, d, sentinel=SENTINEL):
    """columns >= d of a [rows][ld] buffer still hold the sentinel"""
    return bool((buf.detach().cpu()[..., d:] == sentinel).all())


# ======================================================================================================================================
# (1) mask codes, counts, scan, compaction, low-valid weights                                          exact
# ======================================================================================================================================
PROB_VALUES = (0.0, 0.25, 0.75, 1.0)                  # few values: ties in most pixels; delta_p and delta_n are BOTH in the set
MASK_VALUES = (0.0, 0.5, 1.0)
DELTA_P, DELTA_N = 0.25, 0.75
#             C  n_l n_u  P      low high masks    n_pix
MASK_CASES = [(1, 1, 0, 1, 0, 0, "mix"),          # 1      one pixel, one thread
              (1, 0, 1, 255, 0, 1, "mix"),        # 255    unlabeled only, low_rank 0, high_rank C
              (1, 1, 0, 256, 0, 1, "zero"),       # 256    all masks zero: every counter column zero
              (2, 0, 1, 255, 0, 2, "mix"),        # 255
              (2, 2, 0, 128, 2, 2, "zero"),       # 256    low_rank == high_rank == C
              (4, 2, 1, 85, 2, 2, "mix"),         # 255    low_rank == high_rank: no unlabeled negative
              (4, 1, 1, 128, 1, 3, "mix"),        # 256    exactly one full block
              (4, 1, 0, 257, 0, 4, "zero"),       # 257
              (19, 0, 1, 257, 3, 19, "mix"),      # 257    one pixel in the second block; the forced wave block
              (19, 1, 1, 128, 3, 19, "zero"),
              (21, 1, 1, 128, 3, 20, "zero"),
              (21, 1, 1, 32918, 3, 20, "mix"),    # 65 836 = 65 536 + 300: 258 blocks -> scan per == 2, threads 129 ... 255 empty
              (4, 2, 0, 32918, 4, 4, "mix")]      # the same size with labeled images only, low_rank == C


@functools.lru_cache(maxsize=None)
def mask_case(i):
    """Inputs as the kernel takes them (NC[spatial] planes), and the reference: rank of each class in a STABLE descending sort of the
    pixel's probabilities, then the masks of loss_helper_3d.py:341-401 in float64 / int64:
        lv = lab * low_mask != 0, hv = lab * high_mask != 0, anchor = p > delta_p & lv, hard = p < delta_n & hv,
        neg = hard & (labeled ? rank < low_rank & lab == 0 : low_rank <= rank < high_rank).
    (A labeled pixel can never be a negative - lab == 0 contradicts hv - so the NEG columns of a case without unlabeled images are zero.)
    Pixels n_pix - 1, - 2, - 3 (where they exist): all C probabilities equal | p[0] == delta_p | p[0] == delta_n exactly.
    Cases of >= 257 pixels: the ANCHOR bit of class 0 is forced over block 0 so that its four waves hold 0, 1, 63 and 64 set bits."""
    C, n_l, n_u, P, low, high, mmode = MASK_CASES[i]
    n_img, n_pix = n_l + n_u, (n_l + n_u) * P
    g = gen(1, i)
    pv = torch.tensor(PROB_VALUES, dtype=torch.float32)
    prob = pv[torch.randint(0, len(pv), (n_pix, C), generator=g)]
    lab = torch.randint(0, 2, (n_pix, C), generator=g)
    mv = torch.tensor(MASK_VALUES, dtype=torch.float32)
    lowm = mv[torch.randint(0, 3, (n_pix,), generator=g)]
    highm = mv[torch.randint(0, 3, (n_pix,), generator=g)]
    if mmode == "zero":
        lowm, highm = torch.zeros(n_pix), torch.zeros(n_pix)
    prob[n_pix - 1, :] = 0.75
    if n_pix >= 3:
        prob[n_pix - 2, 0], prob[n_pix - 3, 0] = DELTA_P, DELTA_N
        lab[n_pix - 3:, 0] = 1
        if mmode == "mix":
            lowm[n_pix - 3:], highm[n_pix - 3:] = 1.0, 0.5
    forced = n_pix >= 257 and mmode == "mix"
    if forced:
        on = torch.zeros(256, dtype=torch.bool)
        on[64 + 17] = True                     # wave 1: one bit
        on[128:191] = True                     # wave 2: 63 bits
        on[192:256] = True                     # wave 3: 64 bits
        lab[:256, 0], lowm[:256] = 1, 1.0
        prob[:256, 0] = torch.where(on, torch.tensor(1.0), torch.tensor(0.0))
    # reference
    p64 = prob.double()
    order = torch.sort(p64, dim=1, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(C).expand(n_pix, C).contiguous())
    labf = lab.double()
    lv = (labf * lowm.double().view(-1, 1)) != 0
    hv = (labf * highm.double().view(-1, 1)) != 0
    anchor = (p64 > DELTA_P) & lv
    hard = (p64 < DELTA_N) & hv
    labeled = (torch.arange(n_pix) < n_l * P).view(-1, 1)
    cls = torch.where(labeled, (rank < low) & (lab == 0), (rank >= low) & (rank < high))
    neg = hard & cls
    sh = torch.arange(C, dtype=torch.int64)
    codes = ((lv.long() << sh) | (anchor.long() << (MAXC + sh)) | (neg.long() << (2 * MAXC + sh))).sum(1)
    bits = torch.cat((lv.t(), anchor.t(), neg.t()), 0).long()                       # [3C][n_pix], kernel column order
    nblocks = (n_pix + 255) // 256
    padded = torch.zeros((3 * C, nblocks * 256), dtype=torch.int64)
    padded[:, :n_pix] = bits
    counts = padded.view(3 * C, nblocks, 256).sum(2)
    offsets = counts.cumsum(1) - counts
    planes = lambda t: t.view(n_img, P, C).permute(0, 2, 1).contiguous()
    pa, la = planes(prob), planes(lab)
    sorted_p = p64.sort(1).values
    tie = (sorted_p[:, 1:] == sorted_p[:, :-1]).any(1) if C > 1 else torch.zeros(n_pix, dtype=torch.bool)
    return dict(C=C, n_l=n_l, n_u=n_u, P=P, n_pix=n_pix, low=low, high=high, nblocks=nblocks, forced=forced,
                prob_l=pa[:n_l].contiguous(), prob_u=pa[n_l:].contiguous(), lab_l=la[:n_l].contiguous(), lab_u=la[n_l:].contiguous(),
                lowm=lowm, highm=highm, prob=prob, codes=codes, counts=counts, offsets=offsets, totals=counts.sum(1),
                lv=lv.t().contiguous(), anchor=anchor.t().contiguous(), neg=neg.t().contiguous(), tie_share=float(tie.double().mean()))


def emulate_mask_codes(case):
    """The kernel's own formula: rank = #{j : p_j > p_c or (p_j == p_c and j < c)} in fp32, masks from fp32 products; block counts."""
    C, n_pix, n_l, P = case["C"], case["n_pix"], case["n_l"], case["P"]
    p = case["prob"]
    lab = torch.cat((case["lab_l"], case["lab_u"]), 0).permute(0, 2, 1).reshape(n_pix, C)
    j = torch.arange(C)
    before = (p[:, :, None] > p[:, None, :]) | ((p[:, :, None] == p[:, None, :]) & (j[:, None] < j[None, :]))    # [pix][j][c]
    rank = before.sum(1)
    labf = lab.float()
    lv = (labf * case["lowm"].view(-1, 1)) != 0
    hv = (labf * case["highm"].view(-1, 1)) != 0
    dp, dn = torch.tensor(DELTA_P, dtype=torch.float32), torch.tensor(DELTA_N, dtype=torch.float32)
    labeled = (torch.arange(n_pix) < n_l * P).view(-1, 1)
    cls = torch.where(labeled, (rank < case["low"]) & (lab == 0), (rank >= case["low"]) & (rank < case["high"]))
    sh = torch.arange(C, dtype=torch.int64)
    return ((lv.long() << sh) | (((p > dp) & lv).long() << (MAXC + sh)) | (((p < dn) & hv & cls).long() << (2 * MAXC + sh))).sum(1)


# ======================================================================================================================================
# (2) row sums: arco_masked_proto, arco_weighted_row_sum(_h)                                           k u sum|w t| / total
# ======================================================================================================================================
# chain read off masked_row_sum_kernel / weighted_row_sum_kernel: lpr lanes cover one row (lpr = smallest power of two with 4 lpr >= D,
# at most 64), a wave takes rpw = 64 / lpr rows per trip, the block's four waves 4 rpw; one lane adds ceil(rows_per_block / (4 rpw))
# terms in sequence, then log2(rpw) shuffle steps, two additions for the four waves, and one rounding of the slab sum; the finalize
# kernels add the slabs in double and round once (the division included).  The weighted kernel rounds each product w * t once more.
def row_sum_geometry(n_rows, d, slab_rows, cap):
    grid = max(1, min(cap, (n_rows + slab_rows - 1) // slab_rows))
    rpb = (n_rows + grid - 1) // grid
    lpr = 1
    while lpr * 4 < d and lpr < 64:
        lpr *= 2
    ndi = (d + lpr * 4 - 1) // (lpr * 4)
    rpw = 64 // lpr
    trips = (rpb + 4 * rpw - 1) // (4 * rpw)
    return dict(grid=grid, rpb=rpb, lpr=lpr, ndi=ndi, rpw=rpw, trips=trips, last=n_rows % rpb or rpb, empty=grid - (n_rows + rpb - 1) // rpb)


def row_sum_k(n_rows, d, slab_rows, cap, weighted):
    geo = row_sum_geometry(n_rows, d, slab_rows, cap)
    return geo["trips"] + int(math.log2(geo["rpw"])) + 2 + 1 + 1 + (1 if weighted else 0)


#                D    C   n_rows  ldt - D  ldo - D  totals
ROW_SUM_CASES = [(4, 1, 1, 0, 0, True),
                 (8, 8, 63, 4, 4, False),
                 (20, 9, 64, 4, 0, True),            # lpr 8, lanes with d >= D in the last lane group; two c0 groups
                 (64, 21, 65, 0, 12, False),         # three c0 groups
                 (260, 9, 1000, 4, 4, True),         # lpr 64, NDI 2, second pass only 4 columns wide
                 (496, 21, 1000, 0, 0, False),
                 (512, 8, 65, 8, 0, True),
                 (4, 9, 1024 * 64 + 77, 4, 4, True)]  # capped weighted grid: 1024 slabs of 65 rows (one more than a wave step), short last slab
PROTO_CASES = ROW_SUM_CASES[:7] + [(4, 9, 2048 * 256 + 777, 4, 0, True)]          # capped masked grid: 2048 slabs of 257 rows (two trips), short last slab


def _row_values(g, n, d, half):
    t = torch.randn((n, d), generator=g)
    if half:
        t = t.half()
        sub = torch.randint(-1023, 1024, (n, d), generator=g).to(torch.float64) * 2.0 ** -24       # f16 subnormals
        pick = torch.rand((n, d), generator=g) < 0.1
        t = torch.where(pick, sub.half(), t)
    return t


@functools.lru_cache(maxsize=None)
def weighted_case(i, half):
    """T [n][ldt] (fp32 or f16 with subnormals), weights in {0, 1, fractions} [n][Cp], class C - 1 all zero: an exact 0 without
    totals, NaN (0 / 0, as documented for torch.mean of an empty set) with them."""
    d, C, n, padt, pado, use_tot = ROW_SUM_CASES[i]
    g = gen(2, i, half)
    ldt, cp = d + padt, ceil_to(C, 4)
    T = torch.full((n, ldt), SENTINEL, dtype=torch.float16 if half else torch.float32)
    T[:, :d] = _row_values(g, n, d, half)
    r = torch.rand((n, cp), generator=g)
    W = torch.where(r < 0.4, torch.zeros(()), torch.where(r < 0.7, torch.ones(()), torch.rand((n, cp), generator=g)))
    totals = torch.randint(1, 50, (C,), generator=g)
    if C > 1:
        W[:, C - 1], totals[C - 1] = 0.0, 0
    t64, w64 = T[:, :d].double(), W[:, :C].double()
    s, mag = w64.t() @ t64, w64.abs().t() @ t64.abs()
    k = row_sum_k(n, d, 64, 1024, True)
    div = totals.double().view(-1, 1) if use_tot else torch.ones((C, 1), dtype=torch.float64)
    return dict(d=d, C=C, n=n, ldt=ldt, ldw=cp, ldo=d + pado, T=T, W=W, totals=totals if use_tot else None, ref=s / div,
                tol=gamma(k) * mag / div + TINY, k=k)


@functools.lru_cache(maxsize=None)
def proto_case(i):
    """codes with random low-valid bits (only those are read), class C - 1 without any pixel: NaN in proto."""
    d, C, n, padt, _, _ = PROTO_CASES[i]
    g = gen(3, i)
    ldt = d + padt
    T = torch.full((n, ldt), SENTINEL, dtype=torch.float32)
    T[:, :d] = _row_values(g, n, d, False)
    lv = torch.rand((n, C), generator=g) < 0.4
    if C > 1:
        lv[:, C - 1] = False
    lv[0, 0] = True
    sh = torch.arange(C, dtype=torch.int64)
    codes = (lv.long() << sh).sum(1) | (torch.randint(0, 2, (n,), generator=g) << (MAXC + 1))      # other bits are ignored
    totals = torch.zeros(3 * C, dtype=torch.int64)
    totals[:C] = lv.sum(0)
    totals[C:] = 5                                                                                  # anchor / negative counts: not read
    t64, w64 = T[:, :d].double(), lv.double()
    div = totals[:C].double().view(-1, 1)
    k = row_sum_k(n, d, 256, 2048, False)
    return dict(d=d, C=C, n=n, ldt=ldt, T=T, codes=codes, totals=totals, lv=lv, ref=(w64.t() @ t64) / div,
                tol=gamma(k) * (w64.t() @ t64.abs()) / div + TINY, k=k)


def emulate_row_sum(T, W, div):
    """fp32 products and sums in torch's order, the one f16 widening first; division in fp32."""
    s = W.float().t() @ T.float()
    return s if div is None else s / div.float()


# ======================================================================================================================================
# (3) row normalisation: arco_normalize_rows, _pad, arco_nce_normalize_banks, the row half of arco_nce_prep
# ======================================================================================================================================
# chain: ss = sum x^2 - one lane adds ceil(D / 64) squares (one rounding each), six shuffle steps: relative error (ceil(D / 64) + 7) u,
# all terms being positive; sqrtf halves it and adds u; 1 / max(., eps) adds u; x * inv adds u:  y within ((ceil(D / 64) + 7) / 2 + 3) u |y|,
# inv within ((ceil(D / 64) + 7) / 2 + 2) u |inv|.  A zero row is exact: y == 0, inv == 1.0f / eps.  The rows at the clamp have norms
# eps (1 +- 2^-10), a thousand times further from eps than the error of the norm, so the side of the clamp is not in doubt.
NORM_D = (1, 16, 63, 64, 65, 496)
NORM_N = (1, 4, 5)


def norm_k(d):
    return (math.ceil(d / 64) + 7) / 2 + 3


def special_rows(x, g):
    """rows 0 ... of x [n][d] (as far as they exist): all zero | norm just above eps | norm just below eps"""
    n, d = x.shape
    x[0] = 0.0
    for r, f in ((1, 1.0 + 2.0 ** -10), (2, 1.0 - 2.0 ** -10)):
        if n > r:
            v = torch.rand(d, generator=g) + 0.5
            x[r] = (v.double() / v.double().norm() * EPS_F * f).float()
    return x


def normalize_ref(x64):
    nrm = x64.norm(dim=-1, keepdim=True)
    inv = 1.0 / torch.clamp(nrm, min=EPS_F)
    return x64 * inv, inv.squeeze(-1)


@functools.lru_cache(maxsize=None)
def norm_case(d, n, seed=0):
    g = gen(4, d, n, seed)
    x = special_rows(torch.randn((n + 1, d), generator=g), g)
    x = x[1:] if n == 1 and seed % 2 else x[:n]                  # n == 1: the zero row (even seed) or an ordinary row
    y, inv = normalize_ref(x.double())
    k = norm_k(d)
    return dict(x=x.contiguous(), y=y, inv=inv, ytol=gamma(k) * y.abs(), itol=gamma(k - 1) * inv.abs(), nrm=x.double().norm(dim=-1))


def emulate_normalize(x):
    ss = (x * x).sum(-1, keepdim=True)
    inv = 1.0 / torch.clamp(ss.sqrt(), min=torch.tensor(EPS, dtype=torch.float32))
    return x * inv, inv.squeeze(-1)


BANK_LP = (16, 48)


def bank_lens(lp):
    return sorted({l for l in (1, 15, 16, 17, lp) if l <= lp})


@functools.lru_cache(maxsize=None)
def banks_case(d, lp):
    """E banks [len][d] with ragged lengths, each with the three special rows where it is long enough"""
    lens = bank_lens(lp)
    g = gen(5, d, lp)
    banks = [special_rows(torch.randn((l, d), generator=g), g) if l >= 3 else torch.randn((l, d), generator=g) for l in lens]
    bn = torch.zeros((len(lens), lp, d), dtype=torch.float64)          # rows >= len stay zero; the tests add the pad columns
    for e, b in enumerate(banks):
        bn[e, :b.shape[0]] = normalize_ref(b.double())[0]
    return dict(banks=banks, lens=lens, bn=bn, tol=gamma(norm_k(d)) * bn.abs())


# ======================================================================================================================================
# (4) multiplicities                                                                                    exact
# ======================================================================================================================================
#             L   Nn    ld - L
MULT_CASES = [(1, 1, 3), (2, 300, 2), (33, 4097, 15), (257, 300, 15), (257, 4097, 0), (2, 1, 0), (33, 300, 7)]


@functools.lru_cache(maxsize=None)
def mult_case(i, q=3):
    """idx [q][Nn] in [-L, L): query 0 draws ONE row Nn times (through a negative index), the others are random with negative values."""
    L, nn, pad = MULT_CASES[i]
    g = gen(6, i)
    idx = torch.randint(-L, L, (q, nn), generator=g)
    idx[0, :] = -1                                           # row L - 1, Nn times
    m = torch.stack([torch.bincount(torch.where(r < 0, r + L, r), minlength=L) for r in idx])
    ref = torch.zeros((q, L + pad), dtype=torch.int64)
    ref[:, :L] = m
    return dict(L=L, nn=nn, ld=L + pad, idx=idx.contiguous(), ref=ref)


# ======================================================================================================================================
# (5) InfoNCE: arco_infonce_fwd | arco_nce_fused | arco_nce_score + arco_nce_finish against ONE float64 formula
# ======================================================================================================================================
#            Q   lens            D    temp  Nn
NCE_CASES = [(1, (1,), 4, 0.5, 5),
             (63, (127, 128, 1), 16, 0.05, 9),
             (64, (129,), 20, 4.0, 300),
             (65, (300, 17, 128), 496, 0.05, 33),
             (5, (300,), 20, 0.5, 4097),
             (64, (128, 129, 127), 4, 0.05, 17),
             # the two-per-word 16-bit LDS counters: odd and even lens 1 / 2 / 33 / 257 (ld 272 > L), one row drawn 1 / 300 / 4097 times
             (2, (1, 2, 33, 257), 4, 0.5, 1),
             (3, (257, 2, 33), 4, 4.0, 300),
             (2, (33, 257, 1, 2), 4, 0.5, 4097)]


@functools.lru_cache(maxsize=None)
def nce_case(i):
    """E entries: raw banks [len_e][D], anchors already normalised An [E*Q][Dp] (fp32, zero pad), normalised prototypes Pn [nP][Dp],
    sampled negatives idx_all (layout of _contrast.py: per entry Q anchor indices, then Q * Nn negatives).  Built so that cosines of
    exactly +1, -1 and 0 occur: bank rows 0, 1, 2 of every entry long enough are +v, -v (v a signed power-of-two pattern: unit norm
    exact in fp32) and a vector orthogonal to v; anchor 0 of every entry is v, its prototype is -v.  Bank row 3 is all zero (sampled:
    a zero row with nonzero multiplicity).  Query 0 samples only row 1 (cosine -1) while its positive has cosine -1: at temp 0.05 the
    deepest underflow the fixed shift exp((s - 1) / T) can see.  Query 1 (where Q > 1) samples one row Nn times through index -1.
    Reference per query, float64: x = [pos / T, S_k / T with multiplicity M_k], loss = logsumexp(x) - pos / T,
    W_k = M_k exp(S_k / T - lse) / T = d loss / d S_k, gpos = (exp(pos / T - lse) - 1) / T."""
    q, lens, d, temp, nn = NCE_CASES[i]
    E, dp, lp = len(lens), ceil_to(d, 16), ceil_to(max(lens), 16)
    g = gen(7, i)
    # v: d entries of +-2^-m with sum of squares exactly 1 when d is a power of four times ... keep it simple: four entries of 1/2
    v = torch.zeros(d)
    v[:4] = torch.tensor([0.5, -0.5, 0.5, 0.5])
    w = torch.zeros(d)
    w[:4] = torch.tensor([0.5, 0.5, -0.5, 0.5])                      # <v, w> = 0.25 - 0.25 - 0.25 + 0.25 = 0
    banks = []
    for l in lens:
        b = torch.randn((l, d), generator=g) * (torch.rand((l, 1), generator=g) * 3 + 0.1)
        for r, val in ((0, 3.0 * v), (1, -0.75 * v), (2, 2.0 * w), (3, torch.zeros(d))):
            if l > r:
                b[r] = val
        banks.append(b.contiguous())
    n_p = E + 1
    prow = [(e + 1) % n_p for e in range(E)]
    P = torch.randn((n_p, d), generator=g)
    A = torch.randn((E * q, d), generator=g)
    for e in range(E):
        A[e * q] = v
        P[prow[e]] = -v
    an = torch.zeros((E * q, dp))
    an[:, :d] = normalize_ref(A.double())[0].float()
    pn = torch.zeros((n_p, dp))
    pn[:, :d] = normalize_ref(P.double())[0].float()
    stride = q + q * nn + 3
    idx_all = torch.zeros(E * stride, dtype=torch.int64)
    M = torch.zeros((E, q, lp), dtype=torch.int64)
    for e, l in enumerate(lens):
        idx = torch.randint(-l, l, (q, nn), generator=g)
        idx[0, :] = min(1, l - 1)
        if q > 1:
            idx[1, :] = -1
        if q > 2 and l > 3:
            idx[2, 0] = 3                                            # the zero bank row
        idx_all[e * stride:e * stride + q] = torch.randint(0, 7, (q,), generator=g)
        idx_all[e * stride + q:e * stride + q + q * nn] = idx.flatten()
        M[e, :, :l] = torch.stack([torch.bincount(torch.where(r < 0, r + l, r), minlength=l) for r in idx])
    # float64 cosines from the fp32 values, their magnitude sums, bank norms
    cos = torch.zeros((E, q, lp), dtype=torch.float64)
    mag = torch.zeros((E, q, lp), dtype=torch.float64)               # sum_d |a_d b_d| / max(||b||, eps)
    bnorm = torch.ones((E, lp), dtype=torch.float64)
    a64 = an.double().view(E, q, dp)[:, :, :d]
    for e, b in enumerate(banks):
        b64 = b.double()
        nb = torch.clamp(b64.norm(dim=1), min=EPS_F)
        cos[e, :, :lens[e]] = (a64[e] @ b64.t()) / nb
        mag[e, :, :lens[e]] = (a64[e].abs() @ b64.abs().t()) / nb
        bnorm[e, :lens[e]] = nb
    p64 = pn.double()[prow]                                           # [E][dp]
    pos = (an.double().view(E, q, dp) * p64[:, None, :]).sum(-1)
    pmag = (an.double().view(E, q, dp) * p64[:, None, :]).abs().sum(-1)
    return dict(q=q, lens=lens, d=d, dp=dp, lp=lp, E=E, temp=temp, nn=nn, banks=banks, An=an, Pn=pn, prow=prow, n_p=n_p,
                idx_all=idx_all, stride=stride, M=M, cos=cos, mag=mag, bnorm=bnorm, pos=pos, pmag=pmag)


def nce_ref(s64, m, pos, temp):
    """s64 [E][q][lp] scores (float64), m multiplicities, pos [E][q] -> loss, W, gpos, lse, p_pos (all float64)"""
    t = float(torch.tensor(temp, dtype=torch.float32))               # temp travels as a C float
    x = torch.where(m > 0, s64 / t, torch.full_like(s64, -math.inf))
    logm = torch.where(m > 0, m.double().log(), torch.full_like(s64, -math.inf))
    lse = torch.logsumexp(torch.cat(((pos / t).unsqueeze(-1), x + logm), -1), -1)
    w = torch.where(m > 0, torch.exp(x + logm - lse.unsqueeze(-1)) / t, torch.zeros_like(s64))
    p_pos = torch.exp(pos / t - lse)
    return dict(loss=lse - pos / t, W=w, gpos=(p_pos - 1.0) / t, lse=lse, p_pos=p_pos, x=x, t=t)


def nce_tols(ref, e_s, e_pos, round_mag, extra_rel=0.0):
    """First-order propagation through the softmax.  e_s [E][q][lp], e_pos [E][q]: absolute errors of the LOGITS S_k / T and pos / T as
    the route computes them (below).  d lse / d x_k = softmax probability p_k (= T W_k), d lse / d (pos / T) = p_pos, so
        d_lse  = sum_k p_k e_s_k + p_pos e_pos + 8 u round_mag
        d_loss = sum_k p_k e_s_k + (1 - p_pos) e_pos + 8 u round_mag
    - 8 u round_mag: expf (2 u relative on every term, so 2 u on the sum, an absolute 2 u on its logarithm), the sum of the staged
    kernels (double), log and its rounding to fp32, the rounding of shift + log, of pos * (1 / T) and of the final difference;
    round_mag is the sum of the magnitudes these roundings act on, + 1 (staged: |lse| + |pos / T| + |lse - row maximum| + 1; score
    kernel, everything shifted by 1 / T: |lse - 1 / T| + |pos / T - 1 / T| + 1).
        W_k    relative e_s_k + d_lse + u |x_k - lse| + 6 u + extra_rel    (argument of expf, expf, the products with M and 1 / T)
        gpos   (p_pos (e_pos + d_lse + u |pos / T - lse| + 3 u) + 2 u (1 - p_pos)) / T"""
    t = ref["t"]
    p = ref["W"] * t
    base = (p * e_s).sum(-1)
    post = ref["lse"] - ref["loss"]                                    # pos / T
    d_lse = base + ref["p_pos"] * e_pos + 8 * U * round_mag
    d_loss = base + (1 - ref["p_pos"]) * e_pos + 8 * U * round_mag
    xk = torch.where(torch.isfinite(ref["x"]), ref["x"], torch.zeros_like(ref["x"]))
    w_tol = ref["W"].abs() * (e_s + d_lse.unsqueeze(-1) + U * (xk - ref["lse"].unsqueeze(-1)).abs() + 6 * U + extra_rel)
    g_tol = (ref["p_pos"] * (e_pos + d_lse + U * (post - ref["lse"]).abs() + 3 * U) + 2 * U * (1 - ref["p_pos"])) / t
    return dict(loss=d_loss, W=w_tol, gpos=g_tol, lse=d_lse)


def staged_round_mag(ref):
    post = ref["lse"] - ref["loss"]
    mx = torch.maximum(post, ref["x"].max(-1).values)
    return ref["lse"].abs() + post.abs() + (ref["lse"] - mx).abs() + 1


def score_round_mag(ref):
    post = ref["lse"] - ref["loss"]
    return (ref["lse"] - 1 / ref["t"]).abs() + (post - 1 / ref["t"]).abs() + 1


def staged_logit_errors(case, s32, ref):
    """arco_infonce_fwd / arco_nce_fused: S is an fp32 INPUT (exact); the logit s * (1 / T) - mx rounds 1 / T, the product and the
    difference: u (2 |S_k| / T + |x_k - mx|) <= 4 u max(|S_k|, 1) / T + ... kept as u (2 |S_k| / T + 2 / T + 2 |pos| / T).
    pos = <An, Pn> over Dp columns: one thread adds ceil(Dp / 256) products, six shuffle steps, two additions for the four waves, one
    rounding per product: k_dot = ceil(Dp / 256) + 9; the same three roundings of the logit follow."""
    t = ref["t"]
    span = (2.0 + 2.0 * case["pos"].abs()) / t
    e_s = U * (2 * s32.double().abs() / t + span.unsqueeze(-1))
    k_dot = math.ceil(case["dp"] / 256) + 9
    e_pos = gamma(k_dot) * case["pmag"] / t + U * (2 * case["pos"].abs() / t + span)
    return e_s, e_pos


def score_logit_errors(case, ref):
    """arco_nce_score: S_k = acc * ib.  acc: Dp / 4 chained v_mfma_f32_16x16x4_f32, four products and four additions each: at most
    Dp additions and one rounding per product, k_dot = Dp + 1 on sum|a_d b_d|.  ib = 1 / max(sqrt(ssq), eps): a thread adds, per chunk
    of 16 columns, a quad of squares (one rounding each, two additions) to its partial (nchunks additions), the four quad partials of
    a row are then added in sequence: relative (nchunks + 7) u on ssq, halved by sqrtf, + 2 u for sqrtf and the division.  One more
    rounding for acc * ib, three for (s - 1) * (1 / T).  The row sum of the weighted exponentials is fp32 in this kernel: four
    additions in a lane, four shuffle steps, one for the two wave columns - nine additions of positive terms = 9 u relative on the
    sum = 9 u on lse, counted into every logit.  pos: per chunk a quad of products (one rounding each, two additions) added to the
    thread's partial, then the four quad partials: k_pos = nchunks + 7."""
    t = ref["t"]
    nchunks = case["dp"] // 16
    k_ib = (nchunks + 7) / 2 + 3
    e_s = (gamma(case["dp"] + 1) * case["mag"] + gamma(k_ib) * case["cos"].abs()) / t + U * (3 * (case["cos"].abs() + 1) / t + 9)
    e_pos = gamma(nchunks + 7) * case["pmag"] / t + 3 * U * (case["pos"].abs() + 1) / t
    return e_s, e_pos, k_ib


# ======================================================================================================================================
# (6) anchor gradients
# ======================================================================================================================================
@functools.lru_cache(maxsize=None)
def grad_case(n, d, dp, shared_pos, seed=0):
    """A [n][d] with a zero row (clamped), a row of norm eps / 2 (clamped) and one just above eps where n allows; G [n][dp], gpos,
    gscale, prototypes.  Reference: float64 autograd of A -> scale * <A / max(||A||, eps), gs * G + gpos * Pn>.
    The kernel reads An and inv rounded to fp32 (u each).  g_d = G gs + gp Pn_d: three roundings.  dot = sum g_d An_d: a lane adds
    ceil(Dp / 64) products, six shuffle steps: k = ceil(Dp / 64) + 7, + 3 for g, + 1 for An.  Then An_d * dot, the difference, * inv,
    * scale: one rounding each and u for An and inv:
        tol_d = |inv scale| u ((k + 8) |An_d| sum|g An| + 8 (|G_d gs| + |gp Pn_d|))          (|g_d - An_d dot| <= |g_d| + |An_d| sum|g An|)
    A clamped row is g * inv * scale: inside the second term."""
    g = gen(8, n, d, dp, shared_pos, seed)
    A = torch.randn((n, d), generator=g)
    A[0] = 0.0
    if n > 1:
        v = torch.rand(d, generator=g) + 0.5
        A[1] = (v.double() / v.double().norm() * EPS_F * 0.5).float()
    if n > 2:
        v = torch.rand(d, generator=g) + 0.5
        A[2] = (v.double() / v.double().norm() * EPS_F * (1 + 2.0 ** -10)).float()
    G = torch.zeros((n, dp))
    G[:, :d] = torch.randn((n, d), generator=g)
    n_p = 1 if shared_pos else n
    pn = torch.zeros((n_p, dp))
    pn[:, :d] = normalize_ref(torch.randn((n_p, d), generator=g).double())[0].float()
    gpos = -torch.rand(n, generator=g)
    gscale = torch.rand(n, generator=g) + 0.5
    scale = 0.375
    y, inv = normalize_ref(A.double())
    an = torch.zeros((n, dp))
    an[:, :d] = y.float()
    return dict(n=n, d=d, dp=dp, A=A, G=G, Pn=pn, gpos=gpos, gscale=gscale, scale=scale, An=an, inv=inv.float())


def grad_ref(case, prow, use_gscale):
    """prow [n]: prototype row of every anchor row"""
    d, dp = case["d"], case["dp"]
    gs = case["gscale"].double() if use_gscale else torch.ones(case["n"], dtype=torch.float64)
    gt = case["G"].double() * gs.view(-1, 1) + case["gpos"].double().view(-1, 1) * case["Pn"].double()[prow]
    a = case["A"].double().clone().requires_grad_(True)
    y = a / torch.clamp(a.norm(dim=1, keepdim=True), min=EPS_F)
    (case["scale"] * (y * gt[:, :d]).sum()).backward()
    an, inv = case["An"].double(), case["inv"].double().view(-1, 1)
    k = math.ceil(dp / 64) + 7
    gmag = (case["G"].double() * gs.view(-1, 1)).abs() + (case["gpos"].double().view(-1, 1) * case["Pn"].double()[prow]).abs()
    dotmag = (gmag * an.abs()).sum(1, keepdim=True)
    tol = (inv * case["scale"]).abs() * U * ((k + 8) * an.abs() * dotmag + 8 * gmag)
    return a.grad, tol[:, :d] + TINY


def emulate_anchor_grad(case, prow, use_gscale):
    d = case["d"]
    gs = case["gscale"] if use_gscale else torch.ones(case["n"])
    g = case["G"] * gs.view(-1, 1) + case["gpos"].view(-1, 1) * case["Pn"][prow]
    dot = (g * case["An"]).sum(1, keepdim=True)
    iv = case["inv"].view(-1, 1)
    clamped = iv >= torch.tensor(INV_EPS_F)
    v = torch.where(clamped, g * iv, iv * (g - case["An"] * dot))
    return (v * torch.tensor(case["scale"]))[:, :d]


# ======================================================================================================================================
# (7) scatter-add and the loss sum
# ======================================================================================================================================
@functools.lru_cache(maxsize=None)
def scatter_case(d, n, m, use_list, seed=0):
    """n source rows onto 6 destination rows; destination 2 receives m of them (duplicates add in ANY order: atomics).  Every element
    is dst + sum of a * src over its sources: one rounding per product, one per addition, at most m of them:
    (m + 1) u sum|terms|, the destination's own value being a term.  alpha * alpha_dev is exact (0.5 * 3)."""
    g = gen(9, d, n, m, use_list, seed)
    n_dst = 6
    rows = torch.randint(0, n_dst - 1, (n,), generator=g)
    rows = torch.where(rows >= 2, rows + 1, rows)                          # the others avoid destination 2 ...
    rows[torch.randperm(n, generator=g)[:m]] = 2                           # ... which receives exactly m rows
    mult = int(torch.bincount(rows, minlength=n_dst).max()) if n else 0
    lst = torch.randperm(n_dst, generator=g).to(torch.int32)               # list[idx] -> destination row
    inv_list = torch.argsort(lst.long())
    idx = inv_list[rows] if use_list else rows
    src = torch.randn((n, d + 4), generator=g)
    dst = torch.full((n_dst, d + 3), SENTINEL)
    dst[:, :d] = torch.randn((n_dst, d), generator=g)
    return dict(d=d, n=n, n_dst=n_dst, rows=rows, idx=idx.contiguous(), list=lst, src=src, dst=dst, mult=mult)


def scatter_ref(case, a):
    d = case["d"]
    ref, mag = case["dst"][:, :d].double().clone(), case["dst"][:, :d].double().abs()
    ref.index_add_(0, case["rows"], a * case["src"][:, :d].double())
    mag.index_add_(0, case["rows"], abs(a) * case["src"][:, :d].double().abs())
    return ref, gamma(case["mult"] + 1) * mag + TINY


SUM_N = (1, 255, 257, 5000)


@functools.lru_cache(maxsize=None)
def sum_case(n):
    """multiples of 2^-10 of both signs (they cancel; the kernel's double sum is exact), out_before and scale arbitrary:
    the kernel rounds scale * sum to fp32 (u |v|) and, accumulating, the sum with out_before (u |result|): 2 u |result| + u |out_before|."""
    g = gen(10, n)
    x = torch.randint(-4096, 4097, (n,), generator=g).float() / 1024
    return dict(x=x, scale=float(torch.tensor(1.0 / 768, dtype=torch.float32)), before=float(torch.tensor(-3.3, dtype=torch.float32)))


def sum_ref(case, accumulate):
    v = float(case["x"].double().sum()) * case["scale"]
    res = v + (case["before"] if accumulate else 0.0)
    return torch.tensor([res], dtype=torch.float64), torch.tensor([2 * U * abs(res) + U * abs(case["before"]) + TINY], dtype=torch.float64)
