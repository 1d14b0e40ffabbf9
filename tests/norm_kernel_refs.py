"""Case tables, input generators, float64 references, per-element bounds and fp32 emulations shared by tests/test_norm_kernels_gpu.py
(the BatchNorm / GroupNorm kernel family of csrc/elementwise.hip, one entry point at a time) and tests/test_norm_kernels_cpu.py (the
same bounds held against an fp32 emulation of every kernel, the input conditions, planted errors, host-side argument checks).
Plain CPU torch / numpy only; nothing here touches a GPU.

Every reference is float64, written from the OPERATION (sums of a row range, the BatchNorm / GroupNorm formulas, F.batch_norm /
F.group_norm autograd for the chains) on the SAME fp32 / f16 input values the kernel reads.  Every bound is per element, with
u = 2^-24 and gamma(k) = k u / (1 - k u); k is the longest fp32 rounding chain read off the kernel.  The derivations stand beside
the functions.  One stored f16 result adds 2^-11 |ref| + 2^-25 (tests/test_unet_ops_edges_gpu.py).

Kinds of input
  exact   values k * 2^-3, |k| <= 32, 20 % zeros; parameters powers of two / small dyadic numbers: every fp32 operation of the kernel
          is exact (or the result carries ONE final rounding), so the result must equal the float64 value bit for bit.
  wide    six decades of magnitude, mixed signs, 20 % zeros: held per element to the derived bound.  Elements whose float64
          pre-activation lies within 8 x its bound of zero are moved away from zero here (settle), so that the fp32 sign decision of
          the LeakyReLU is the float64 one and no element is left out of a comparison.
  offset  channel mean 100, standard deviation 1, the last channel constant 1.5 (statistics and chains)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from loss_kernel_refs import U, gamma, gen

EPS_BN = float(np.float32(1e-5))                      # eps and momentum travel as C floats: the references use the fp32 values
MOM = float(np.float32(0.1))
GRID_CAP = 4096 * 256                                 # work items one trip of an ew_grid launch covers (4096 workgroups of 256)
H_REL, H_ABS = 2.0 ** -11, 2.0 ** -25                 # one f16 rounding
D = 2.0 ** -53
KINDS = ("exact", "wide", "offset")
SLOPES = (0.0, 0.01, 0.25)


def f32(v):
    return float(np.float32(v))


# ======================================================================================================================================
# geometry of the slab reductions (chan_stats_kernel, bn_act_bwd_reduce_kernel)
# ======================================================================================================================================
def chan_blocks(M):
    """arco_chan_stats_blocks restated: 512 rows per block, at least min(512, M / 16) blocks, at most 2048"""
    b = max((M + 511) // 512, min((M + 15) // 16, 512))
    return max(1, min(b, 2048))


def geometry(M, C):
    """M rows per group.  t = additions on the longest path of one slab: rows per thread, the shuffle tree (log2 of the threads that
    share a channel quad inside a wave, + 2 for the four waves) or the serial LDS loop (rstep), + 1 for the squaring / product"""
    nblk = chan_blocks(M)
    rpb = -(-M // nblk)
    q4 = C // 4
    rstep = 256 // q4
    rpt = -(-rpb // rstep)
    shuffle = (q4 & (q4 - 1)) == 0 and q4 <= 64
    tree = int(math.log2(64 // q4)) + 2 if shuffle else rstep
    return dict(nblk=nblk, rpb=rpb, q4=q4, rstep=rstep, rpt=rpt, shuffle=shuffle, t=rpt + tree + 1,
                empty=nblk - -(-M // rpb))


def slab_ranges(M, nblk, shift=0):
    """row range of every slab; `shift` plants the error 'ranges shifted by one slab'"""
    rpb = -(-M // nblk)
    return [(min(M, (b + shift) * rpb), min(M, (b + shift + 1) * rpb)) for b in range(nblk)]


def slab_sums(V, groups, nblk, shift=0):
    """float64 sums of V [groups * M, C] over the row range of every slab -> [groups, nblk, C]; empty ranges give 0"""
    GM, C = V.shape
    M = GM // groups
    out = V.new_zeros(groups, nblk, C)
    Vg = V.view(groups, M, C)
    rpb = -(-M // nblk)
    if shift == 0:
        pad = V.new_zeros(groups, nblk * rpb, C)
        pad[:, :M] = Vg
        return pad.view(groups, nblk, rpb, C).sum(2)
    for b, (r0, r1) in enumerate(slab_ranges(M, nblk, shift)):
        if r1 > r0:
            out[:, b] = Vg[:, r0:r1].sum(1)
    return out


def stats_layout(S):
    """[groups, nblk, C] -> the [C][groups * nblk] layout of arco_chan_stats / arco_bn_finalize"""
    G, nblk, C = S.shape
    return S.permute(2, 0, 1).reshape(C, G * nblk).contiguous()


def bwd_layout(S):
    """[groups, nblk, C] -> the [groups][C][nblk] layout of the backward's workspace"""
    return S.permute(0, 2, 1).contiguous()


def emu_slabs(S, Q, groups, C):
    """fp32 emulation of the block reduction, in the kernel's order: thread (tq, tr) adds the rows r0 + tr, + rstep, ... of its channel
    quad one after the other, then block_channel_totals (xor-shuffle tree inside a wave and (w0 + w1) + (w2 + w3), or the serial
    loop over tr).  S, Q: the fp32 terms [groups * M, C] (x and x * x; dy and dy * xhat).  -> two [groups, nblk, C] arrays"""
    S, Q = np.asarray(S, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    M = S.shape[0] // groups
    g = geometry(M, C)
    nblk, rpb, q4, rstep, rpt = g["nblk"], g["rpb"], g["q4"], g["rstep"], g["rpt"]
    out = []
    for V in (S, Q):
        pad = np.zeros((groups, nblk * rpb, C), np.float32)
        pad[:, :M] = V.reshape(groups, M, C)
        p2 = np.zeros((groups, nblk, rpt * rstep, C), np.float32)
        p2[:, :, :rpb] = pad.reshape(groups, nblk, rpb, C)
        p2 = p2.reshape(groups, nblk, rpt, rstep, C)
        acc = np.zeros((groups, nblk, rstep, C), np.float32)
        for i in range(rpt):
            acc = acc + p2[:, :, i]
        if g["shuffle"]:
            per = 64 // q4                                            # threads of one wave that share a channel quad
            a = acc.reshape(groups, nblk, 4, per, C)
            step = 1
            while step < per:
                a = a + a[:, :, :, np.arange(per) ^ step]
                step *= 2
            a = a[:, :, :, 0]
            tot = (a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])
        else:
            tot = np.zeros((groups, nblk, C), np.float32)
            for r in range(rstep):
                tot = tot + acc[:, :, r]
        out.append(torch.from_numpy(tot))
    return out


def emu_slab_total(slabs):
    """slab_sums2<256> + the wave / block tree in fp64, in the kernel's order: slabs [..., n] float32 -> [...] float64"""
    a = np.asarray(slabs, dtype=np.float64)
    n = a.shape[-1]
    k = -(-n // 256)
    pad = np.zeros(a.shape[:-1] + (k * 256,))
    pad[..., :n] = a
    pad = pad.reshape(a.shape[:-1] + (k, 256))
    acc = np.zeros(a.shape[:-1] + (256,))
    for i in range(k):
        acc = acc + pad[..., i, :]
    w = acc.reshape(a.shape[:-1] + (4, 64))
    o = 32
    while o:
        w = w + w[..., np.arange(64) ^ o]
        o //= 2
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


# ======================================================================================================================================
# inputs
# ======================================================================================================================================
def values(g, rows, C, kind, half=False, decades=(-3, 3)):
    """[rows, C] float32 values of one kind (f16-representable when half); wide: magnitudes 10^decades[0] .. 10^decades[1]"""
    if kind == "exact":
        x = torch.randint(-32, 33, (rows, C), generator=g).double() / 8
    elif kind == "wide":
        x = 10.0 ** (torch.rand(rows, C, generator=g, dtype=torch.float64) * (decades[1] - decades[0]) + decades[0])
        x = x * (torch.randint(0, 2, (rows, C), generator=g) * 2 - 1)
    else:
        x = 100.0 + torch.randn(rows, C, generator=g, dtype=torch.float64)
    if kind != "offset":
        x[torch.rand(rows, C, generator=g) < 0.2] = 0
    else:
        x[:, C - 1] = 1.5
    x = x.float()
    return x.half().float() if half else x


def params(g, groups, C, kind, nozero_shift=False):
    """mean / istd [groups, C], gamma / beta [C] as float32.  exact: (z - mu) * is * ga + be is exact in fp32 (z, mu multiples of 2^-3,
    |z - mu| <= 5, is and |ga| in {1/2, 1, 2}, be a multiple of 2^-2; nozero_shift: be an odd multiple of 2^-6, so that no
    pre-activation is 0).  offset: mean near 100."""
    if kind == "exact":
        mu = torch.randint(-8, 9, (groups, C), generator=g).float() / 8
        istd = 2.0 ** torch.randint(-1, 2, (groups, C), generator=g).float()
        ga = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float() * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        be = torch.randint(-8, 9, (C,), generator=g).float() / 4
        if nozero_shift:
            be = (2 * torch.randint(-64, 64, (C,), generator=g).float() + 1) / 64
    else:
        mu = torch.randn(groups, C, generator=g) + (100.0 if kind == "offset" else 0.0)
        istd = 0.5 + 2 * torch.rand(groups, C, generator=g)
        ga = (0.5 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        be = torch.randn(C, generator=g)
    return dict(mu=mu.float(), istd=istd.float(), ga=ga.float(), be=be.float())


# ======================================================================================================================================
# dropout mask (csrc/common.h: pcg_hash, drop_thr16, drop_keep) restated in numpy uint32 / uint64
# ======================================================================================================================================
M32 = np.uint32


def pcg(v):
    v = np.asarray(v, dtype=np.uint32)
    s = v * M32(747796405) + M32(2891336453)
    w = ((s >> ((s >> M32(28)) + M32(4))) ^ s) * M32(277803737)
    return (w >> M32(22)) ^ w


def drop_seed(seed, salt):
    """graph-captured forwards xor a per-replay salt from device memory into the seed"""
    return seed if salt is None else seed ^ ((salt * 0x9E3779B97F4A7C15) % 2 ** 64)


def drop_thr(p):
    return int(np.uint32(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))


def keep_mask(seed, e, p):
    """e: uint64 element indices.  16 random bits per element, two elements per hash."""
    e = np.asarray(e, dtype=np.uint64)
    e2 = e >> np.uint64(1)
    lo = (e2 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (e2 >> np.uint64(32)).astype(np.uint32)
    inner = pcg(hi + np.asarray([seed & 0xFFFFFFFF], dtype=np.uint32))
    h = pcg(lo ^ inner ^ np.asarray([seed >> 32], dtype=np.uint32))
    bits = np.where((e & np.uint64(1)) != 0, h >> M32(16), h & M32(0xFFFF))
    return bits >= M32(drop_thr(p))


def drop_index(rows, C, groups, mode, P, with_row0=True):
    """element index of (row, channel): mode 1 per element of the WHOLE tensor (the group's first row enters through row0), mode 2 per
    (image, channel) with P rows per image.  with_row0 = False plants the error 'index without the group's row0'."""
    r = np.arange(rows, dtype=np.uint64)
    if not with_row0:
        r = r % np.uint64(rows // groups)
    if mode == 2:
        r = r // np.uint64(P)
    return r[:, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :]


def keep_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def drop_keep(drop, rows, C, groups, with_row0=True):
    """drop = (mode, p, seed, P, salt) -> bool [rows, C] torch"""
    mode, p, seed, P, salt = drop
    k = keep_mask(drop_seed(seed, salt), drop_index(rows, C, groups, mode, P, with_row0), p)
    return torch.from_numpy(np.ascontiguousarray(k))


# ======================================================================================================================================
# forward apply:  a = drop(lrelu((z - mu) * is * ga + be)) + R
# ======================================================================================================================================
def preact(Z, prm, groups, nomean=False):
    """float64 pre-activation y [rows, C], t = (z - mu) * is * ga, and the bound of the fp32 y: three roundings on t (difference and two
    products), one on the sum - gamma(3) |t| + u |y| - also where the compiler contracts the last product and the sum."""
    rows, C = Z.shape
    z = Z.double().view(groups, rows // groups, C)
    if nomean:
        return z.reshape(rows, C), torch.zeros(rows, C, dtype=torch.float64), torch.zeros(rows, C, dtype=torch.float64)
    t = (z - prm["mu"].double()[:, None]) * prm["istd"].double()[:, None] * prm["ga"].double()
    y = t + prm["be"].double()
    return y.reshape(rows, C), t.reshape(rows, C), (gamma(3) * t.abs() + U * y.abs()).reshape(rows, C)


def settle(Z, prm, groups, half=False, extra=None, factor=8):
    """move the elements whose float64 pre-activation lies within 8 x its bound (+ `extra`, the chain's share) of zero to a
    pre-activation near +-1, deterministically.  -> (Z, number of elements moved)"""
    y, _, by = preact(Z, prm, groups)
    if extra is not None:
        by = by + extra
    near = y.abs() <= factor * by
    near &= by > 0
    n = int(near.sum())
    if n:
        rows, C = Z.shape
        M = rows // groups
        mu = prm["mu"].double()[:, None].expand(groups, M, C).reshape(rows, C)
        scale = (prm["istd"].double()[:, None] * prm["ga"].double()).expand(groups, M, C).reshape(rows, C)
        sign = torch.where(torch.arange(rows * C).view(rows, C) % 2 == 0, 1.0, -1.0).double()
        znew = (mu + (sign - prm["be"].double()) / scale).float()
        if half:
            znew = znew.half().float()
        Z = torch.where(near, znew, Z)
    return Z, n


def margin(Z, prm, groups, extra=None):
    """min over the elements of |y| / (8 x bound): > 1 means no fp32 sign decision can differ from the float64 one"""
    y, _, by = preact(Z, prm, groups)
    if extra is not None:
        by = by + extra
    m = by > 0
    return float((y.abs()[m] / (8 * by[m])).min()) if bool(m.any()) else math.inf


def fwd_ref(Z, prm, slope, groups, drop=None, R=None, half=False, nomean=False, with_row0=True):
    """-> (a float64 [rows, C], bound, kept mask or None).  The activation multiplies the bound of y by |slope| and adds one rounding
    where it multiplies; dropout multiplies by keep_scale (the fp32 value) with one more rounding; the skip adds one more."""
    rows, C = Z.shape
    y, _, by = preact(Z, prm, groups, nomean)
    s = f32(slope)
    neg = y < 0
    a = torch.where(neg, y * s, y)
    b = torch.where(neg, by * abs(s) + U * a.abs(), by)
    keep = None
    if drop is not None and drop[1] > 0:
        keep = drop_keep(drop, rows, C, groups, with_row0)
        ks = keep_scale(drop[1])
        a = torch.where(keep, a * ks, torch.zeros_like(a))
        b = torch.where(keep, b * ks + U * a.abs(), torch.zeros_like(b))
    if R is not None:
        a = a + R.double()
        b = b + U * a.abs()
    if half:
        b = b + H_REL * (a.abs() + b) + H_ABS
    return a, b, keep


def fwd_roundings(slope, drop, R, half):
    """roundings an EXACT-kind result carries: the slope product unless the slope is 0 or a power of two, keep_scale, the skip
    addition, the f16 store.  With at most one, the fp32 / f16 result is the correctly rounded float64 one."""
    return int(slope == 0.01) + int(drop is not None and drop[1] > 0) + int(R is not None) + int(half)


def emu_fwd(Z, prm, slope, groups, drop=None, R=None, half=False, nomean=False):
    """fp32 in the kernel's order of operations"""
    rows, C = Z.shape
    z = Z.float().view(groups, rows // groups, C)
    if nomean:
        y = z
    else:
        y = (z - prm["mu"][:, None]) * prm["istd"][:, None] * prm["ga"] + prm["be"]
    y = y.reshape(rows, C)
    y = torch.where(y >= 0, y, y * torch.tensor(slope, dtype=torch.float32))
    if drop is not None and drop[1] > 0:
        keep = drop_keep(drop, rows, C, groups)
        y = torch.where(keep, y * torch.tensor(keep_scale(drop[1]), dtype=torch.float32), torch.zeros_like(y))
    if R is not None:
        y = y + R.float()
    return y.half() if half else y


# ======================================================================================================================================
# statistics: slabs, finalize, deferred running statistics
# ======================================================================================================================================
def stats_ref(X, groups, C, shift=0):
    """float64 slabs of sum x and sum x^2 in the [C][groups * nblk] layout, with the bounds gamma(t) sum|x| and gamma(t) sum x^2"""
    M = X.shape[0] // groups
    g = geometry(M, C)
    x = X.double()
    s, q = slab_sums(x, groups, g["nblk"], shift), slab_sums(x * x, groups, g["nblk"], shift)
    ts = gamma(g["t"]) * slab_sums(x.abs(), groups, g["nblk"], shift)
    return dict(g=g, s=stats_layout(s), q=stats_layout(q), ts=stats_layout(ts), tq=stats_layout(gamma(g["t"]) * q))


def quantum_budget(M, C):
    """exact kind: x^2 <= 16 = 1024 quanta of 2^-6, so a slab of rpb rows holds at most rpb * 1024 quanta; below 2^24 every fp32
    partial of sum x (quanta of 2^-3) and sum x^2 is an exact integer number of quanta"""
    return geometry(M, C)["rpb"] * 1024


def fin_slabs(g, C, groups, npg, cnt):
    """host-written slabs [C][groups * npg] for the finalize tests: wide-kind sums, sum-of-squares slabs scaled so that the variance is
    about half of E[x^2]; the last channel (C >= 3) has all-zero squares and non-zero sums: var = -m^2 < 0 exercises the clamp"""
    s = values(g, C, groups * npg, "wide").double()
    q = values(g, C, groups * npg, "wide").double().abs() + 1e-3
    for c in range(C):
        for gi in range(groups):
            sl = slice(gi * npg, (gi + 1) * npg)
            m2 = float(s[c, sl].sum() / cnt) ** 2
            eq = float(q[c, sl].sum() / cnt)
            if m2 > 0.5 * eq:
                s[c, sl] *= math.sqrt(0.5 * eq / m2)
    if C >= 3:
        q[C - 1] = 0
        s[C - 1] = s[C - 1].abs() + 1.0
    return s.float(), q.float()


def finalize_ref(ssum, ssq, C, groups, cnt, eps=EPS_BN, slab_err=None):
    """ssum / ssq: the GIVEN fp32 slabs [C][groups * npg]; cnt = elements per channel and group.  -> float64 mean, var (clamped), istd
    [groups, C] with bounds.  The kernel sums in fp64 (any order: n summands cost at most n 2^-53 sum|.|), so mean carries one fp32
    rounding; var = q / n - m^2 is ill-conditioned: |dvar| <= (npg + 4) 2^-53 (sum|q| / n + 2 |m| sum|s| / n + m^2), and
    d istd / istd <= dvar / (2 (var + eps)) + 2 2^-53 + u.  slab_err = (es, eq) [C][groups * npg]: errors of the slabs themselves
    (the chains: the slabs come from the fp32 kernel), propagated the same way."""
    npg = ssum.shape[1] // groups
    s = ssum.double().view(C, groups, npg)
    q = ssq.double().view(C, groups, npg)
    S, Q = s.sum(2).t(), q.sum(2).t()                                # [groups, C]
    Sa, Qa = s.abs().sum(2).t(), q.abs().sum(2).t()
    m = S / cnt
    raw = Q / cnt - m * m
    var = raw.clamp_min(0.0)
    istd = 1.0 / torch.sqrt(var + eps)
    dm = (npg + 1) * D * Sa / cnt
    dvar = (npg + 4) * D * (Qa / cnt + 2 * m.abs() * Sa / cnt + m * m)
    if slab_err is not None:
        es = slab_err[0].double().view(C, groups, npg).sum(2).t() / cnt
        eq = slab_err[1].double().view(C, groups, npg).sum(2).t() / cnt
        dm = dm + es
        dvar = dvar + eq + 2 * m.abs() * es + es * es
    tm = dm + U * (m.abs() + dm)
    rel = dvar / (2 * (var + eps) - dvar).clamp_min(1e-300) + 2 * D
    ti = istd * (rel + U * (1 + rel))
    unb = var * cnt / (cnt - 1.0) if cnt > 1 else var
    dunb = dvar * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
    return dict(m=m, var=var, raw=raw, istd=istd, tm=tm, ti=ti, unb=unb, dm=dm, dunb=dunb, dvar=dvar)


def running_ref(rm0, rv0, fin, groups, mom=MOM, upto=None, biased=False, order=None):
    """the running statistics after the groups' updates in group order (float64, no intermediate rounding) and their bound: every
    update rounds once, u |value|, and the earlier error shrinks by (1 - momentum); the finalize errors of m and of the unbiased
    variance enter with weight momentum.  `upto`: only groups < upto update (defer_from).  Planted errors: biased, order."""
    rm, rv = rm0.double().clone(), rv0.double().clone()
    tm, tv = torch.zeros_like(rm), torch.zeros_like(rv)
    gs = list(range(groups if upto is None else upto))
    for g in (gs if order is None else order):
        rm = (1.0 - mom) * rm + mom * fin["m"][g]
        rv = (1.0 - mom) * rv + mom * (fin["var"][g] if biased else fin["unb"][g])
        tm = (1.0 - mom) * tm + mom * fin["dm"][g] + 1.01 * U * rm.abs()
        tv = (1.0 - mom) * tv + mom * fin["dunb"][g] + 1.01 * U * rv.abs()
    return rm, rv, tm, tv


def emu_finalize(ssum, ssq, C, groups, cnt, eps=EPS_BN):
    """the kernel's order: strided fp64 partials per thread, wave tree, four waves; mean / istd rounded to float"""
    npg = ssum.shape[1] // groups
    S = emu_slab_total(ssum.view(C, groups, npg).numpy()).T
    Q = emu_slab_total(ssq.view(C, groups, npg).numpy()).T
    m = S / cnt
    var = np.maximum(Q / cnt - m * m, 0.0)
    return dict(m=torch.from_numpy(m.astype(np.float32)), istd=torch.from_numpy((1.0 / np.sqrt(var + eps)).astype(np.float32)),
                m64=torch.from_numpy(m), unb=torch.from_numpy(var * cnt / (cnt - 1.0) if cnt > 1 else var))


def emu_running(rm0, rv0, em, groups, mom=MOM, upto=None):
    rm, rv = rm0.clone(), rv0.clone()
    for g in range(groups if upto is None else upto):
        rm = ((1.0 - mom) * rm.double() + mom * em["m64"][g]).float()
        rv = ((1.0 - mom) * rv.double() + mom * em["unb"][g]).float()
    return rm, rv


def deferred_ref(rm0, rv0, terms, mom):
    """bn_apply_deferred: terms [n][2][C] float32 applied one after the other with a float rounding after every step -> (rm, rv float32,
    bounds).  The kernel evaluates the same fp64 expression; a contracted multiply-add may move a value that sits on a rounding
    boundary, hence the bound of one rounding per step instead of bit equality (the exact-kind layer, momentum 1/2 and dyadic
    values, has no rounding at all and is compared bit for bit)."""
    rm, rv = rm0.clone(), rv0.clone()
    tm, tv = torch.zeros_like(rm, dtype=torch.float64), torch.zeros_like(rv, dtype=torch.float64)
    for g in range(terms.shape[0]):
        rm = ((1.0 - mom) * rm.double() + mom * terms[g, 0].double()).float()
        rv = ((1.0 - mom) * rv.double() + mom * terms[g, 1].double()).float()
        tm = (1.0 - mom) * tm + 2 * U * rm.abs().double()
        tv = (1.0 - mom) * tv + 2 * U * rv.abs().double()
    return rm, rv, tm, tv


DEFER_FMT = "PPPiifi"                                 # BnDeferDesc of include/arco_hip.h: three pointers, C, n, momentum, pad


# ======================================================================================================================================
# backward:  dy = dA * mask * keep_scale * lrelu'(y);  dz = ga * is * (dy - sum dy / n - xh * sum(dy xh) / n)
# ======================================================================================================================================
def bwd_ref(dA, Z, prm, slope, groups, drop=None, half=False, nomean=False, cpg=0, swap_sums=False, gn_gamma=True, with_row0=True):
    """float64 reference of arco_bn_act_bwd / arco_gn_act_bwd from the same inputs, with every bound:
      slabs    gamma(t + 2) sum|dy| and gamma(t + 5) sum|dy xh| over the slab's rows (dy carries the slope and keep_scale roundings,
               xh two more, the product one)
      sums     the fp64 sum of the kernel's own fp32 slabs rounded to float: the slab bounds added up + u |sum|
      dz       gamma(9) |ga is| (|dy| + |sd / n| + |xh sx / n|): xh gamma(2), the fp32 reciprocal of n one, each product and
               difference one, + the sums' errors |ga is| (dsd + |xh| dsx) / n;  one f16 store on top
      dgamma / dbeta   groups > 1: the sum of the float-rounded per-group sums; accumulate adds the prefilled value, one rounding.
    cpg >= 1 (GroupNorm, groups = samples): the set sums A = sum_j ga_j sd_j, B = sum_j ga_j sx_j replace sd, sx, n = M cpg and
    dz = is (ga dy - A / n - xh B / n).  Planted errors: swap_sums, gn_gamma = False (gamma left out of the set sums)."""
    rows, C = Z.shape
    M = rows // groups
    geo = geometry(M, C)
    dA64 = dA.double()
    s = f32(slope)
    if nomean:
        y = Z.double()
        dy = torch.where(y >= 0, dA64, dA64 * s)
        b = torch.where(y >= 0, torch.zeros_like(dy), U * dy.abs())
        if drop is not None and drop[1] > 0:
            keep = drop_keep(drop, rows, C, 1, with_row0)
            dy = torch.where(keep, dy * keep_scale(drop[1]), torch.zeros_like(dy))
            b = torch.where(keep, b * keep_scale(drop[1]) + U * dy.abs(), torch.zeros_like(b))
        if half:
            b = b + H_REL * (dy.abs() + b) + H_ABS
        return dict(dz=dy, tz=b)
    mu, istd = prm["mu"].double()[:, None], prm["istd"].double()[:, None]
    ga, be = prm["ga"].double(), prm["be"].double()
    xh = (Z.double().view(groups, M, C) - mu) * istd
    y = xh * ga + be
    dy = torch.where(y >= 0, dA64.view(groups, M, C), dA64.view(groups, M, C) * s)
    keep = None
    if drop is not None and drop[1] > 0:
        keep = drop_keep(drop, rows, C, groups, with_row0).view(groups, M, C)
        dy = torch.where(keep, dy * keep_scale(drop[1]), torch.zeros_like(dy))
    dyx = dy * xh
    t = geo["t"]
    nblk = geo["nblk"]
    sl_s, sl_q = slab_sums(dy.reshape(rows, C), groups, nblk), slab_sums(dyx.reshape(rows, C), groups, nblk)
    tl_s = gamma(t + 2) * slab_sums(dy.abs().reshape(rows, C), groups, nblk)
    tl_q = gamma(t + 5) * slab_sums(dyx.abs().reshape(rows, C), groups, nblk)
    sd, sx = dy.sum(1), dyx.sum(1)                                   # [groups, C]
    if swap_sums:
        sd, sx = sx, sd
    dsd = tl_s.sum(1) + (nblk + 1) * D * dy.abs().sum(1) + U * sd.abs()
    dsx = tl_q.sum(1) + (nblk + 1) * D * dyx.abs().sum(1) + U * sx.abs()
    sums = torch.stack((sd, sx), 1)                                  # [groups, 2, C]
    tsums = torch.stack((dsd, dsx), 1)
    # dgamma / dbeta: the float-rounded per-group sums added up (in fp64) and rounded once
    dbeta, dgamma = sd.sum(0), sx.sum(0)
    tb = dsd.sum(0) + U * (dbeta.abs() + dsd.sum(0))
    tg = dsx.sum(0) + U * (dgamma.abs() + dsx.sum(0))
    if cpg:
        n = float(M * cpg)
        gw = ga if gn_gamma else torch.ones_like(ga)
        A = (sd * gw).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C)
        B = (sx * gw).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C)
        dAs = (dsd * ga.abs()).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C)
        dBs = (dsx * ga.abs()).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C)
        dAs = dAs + (cpg + 1) * D * dAs + U * A.abs()
        dBs = dBs + (cpg + 1) * D * dBs + U * B.abs()
        sums, tsums = torch.stack((A, B), 1), torch.stack((dAs, dBs), 1)
        A, B, dAs, dBs = A[:, None], B[:, None], dAs[:, None], dBs[:, None]
        dz = istd * (ga * dy - A / n - xh * B / n)
        tz = gamma(9) * istd.abs() * ((ga * dy).abs() + (A / n).abs() + (xh * B / n).abs()) + istd.abs() * (dAs + xh.abs() * dBs) / n
    else:
        n = float(M)
        SD, SX, dSD, dSX = sd[:, None], sx[:, None], dsd[:, None], dsx[:, None]
        gi = (ga * istd).abs()
        dz = ga * istd * (dy - SD / n - xh * SX / n)
        tz = gamma(9) * gi * (dy.abs() + (SD / n).abs() + (xh * SX / n).abs()) + gi * (dSD + xh.abs() * dSX) / n
    if half:
        tz = tz + H_REL * (dz.abs() + tz) + H_ABS
    return dict(dz=dz.reshape(rows, C), tz=tz.reshape(rows, C), slab_s=bwd_layout(sl_s), slab_q=bwd_layout(sl_q),
                tslab_s=bwd_layout(tl_s), tslab_q=bwd_layout(tl_q), sums=sums, tsums=tsums, dgamma=dgamma, dbeta=dbeta, tg=tg, tb=tb,
                keep=None if keep is None else keep.reshape(rows, C), geo=geo)


def emu_bwd(dA, Z, prm, slope, groups, drop=None, half=False, cpg=0):
    """fp32 in the kernel's order: reduce (emu_slabs), finalize in fp64 to float sums, optional GroupNorm merge, apply"""
    rows, C = Z.shape
    M = rows // groups
    f = torch.float32
    xh = (Z.float().view(groups, M, C) - prm["mu"][:, None]) * prm["istd"][:, None]
    y = xh * prm["ga"] + prm["be"]
    d = dA.float().view(groups, M, C)
    dy = torch.where(y >= 0, d, d * torch.tensor(slope, dtype=f))
    if drop is not None and drop[1] > 0:
        keep = drop_keep(drop, rows, C, groups).view(groups, M, C)
        dy = torch.where(keep, dy * torch.tensor(keep_scale(drop[1]), dtype=f), torch.zeros_like(dy))
    sl_s, sl_q = emu_slabs(dy.reshape(rows, C).numpy(), (dy * xh).reshape(rows, C).numpy(), groups, C)
    sd = torch.from_numpy(emu_slab_total(bwd_layout(sl_s).numpy())).float()        # [groups, C]
    sx = torch.from_numpy(emu_slab_total(bwd_layout(sl_q).numpy())).float()
    dbeta = sd.double().sum(0).float() if groups > 1 else sd[0]
    dgamma = sx.double().sum(0).float() if groups > 1 else sx[0]
    inv = torch.tensor(1.0, dtype=f) / (torch.tensor(float(M), dtype=f) * torch.tensor(float(cpg if cpg else 1), dtype=f))
    ga, istd = prm["ga"], prm["istd"][:, None]
    if cpg:
        g64 = ga.double()
        A = (sd.double() * g64).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C).float()
        B = (sx.double() * g64).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C).float()
        sums = torch.stack((A, B), 1)
        dz = istd * (ga * dy - A[:, None] * inv - xh * B[:, None] * inv)
    else:
        sums = torch.stack((sd, sx), 1)
        dz = ga * istd * (dy - sd[:, None] * inv - xh * sx[:, None] * inv)
    dz = dz.reshape(rows, C)
    return dict(dz=dz.half() if half else dz, slab_s=bwd_layout(sl_s), slab_q=bwd_layout(sl_q), sums=sums, dgamma=dgamma, dbeta=dbeta)


# ======================================================================================================================================
# depth-to-space row maps: Y rows = (voxel of the NV x X2 x Y2 x Z2 grid, tap), tap = dx * 4 + dy * 2 + dz
# ======================================================================================================================================
D2S_GRIDS = ((1, 1, 1, 1), (2, 1, 2, 3), (2, 3, 2, 1))


def d2s(Y, grid, C, taps=(0, 1, 2, 3, 4, 5, 6, 7)):
    """(voxel, tap) rows -> the rows of the [NV, 2 X2, 2 Y2, 2 Z2] tensor.  `taps` plants the error 'one tap permuted'."""
    nv, x2, y2, z2 = grid
    t = Y.view(nv, x2, y2, z2, 8, C)[:, :, :, :, list(taps)].reshape(nv, x2, y2, z2, 2, 2, 2, C)
    return t.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(nv * 8 * x2 * y2 * z2, C).contiguous()


def s2d(A, grid, C):
    """the inverse: voxel rows of the depth-to-space'd tensor -> (voxel, tap) rows"""
    nv, x2, y2, z2 = grid
    t = A.view(nv, x2, 2, y2, 2, z2, 2, C).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return t.reshape(nv * 8 * x2 * y2 * z2, C).contiguous()


# ======================================================================================================================================
# GroupNorm finalize on given slabs
# ======================================================================================================================================
GN_SETS = ((4, 1), (8, 2), (16, 4), (12, 3), (16, 16), (256, 256))


def gn_finalize_ref(ssum, ssq, C, cpg, N, cnt, eps=EPS_BN, slab_err=None):
    """slabs [C][N * npg]; a set = cpg consecutive channels of one sample, cnt elements per (sample, channel) -> the set's mean / istd
    in each of its channels, [N, C].  The set's slabs are those of one 'channel' of cpg * npg slabs and cnt * cpg elements."""
    npg = ssum.shape[1] // N
    sets = C // cpg

    def regroup(x):
        return x.view(sets, cpg, N, npg).permute(0, 2, 1, 3).reshape(sets, N * cpg * npg)
    err = None if slab_err is None else (regroup(slab_err[0]), regroup(slab_err[1]))
    fin = finalize_ref(regroup(ssum), regroup(ssq), sets, N, cnt * cpg, eps, err)
    return {k: (v.repeat_interleave(cpg, 1) if torch.is_tensor(v) else v) for k, v in fin.items()}


def emu_gn_finalize(ssum, ssq, C, cpg, N, cnt, eps=EPS_BN):
    npg = ssum.shape[1] // N
    s = ssum.view(C // cpg, cpg, N, npg).numpy()
    q = ssq.view(C // cpg, cpg, N, npg).numpy()
    S = sum(emu_slab_total(s[:, j]) for j in range(cpg)).T          # per-thread partials run on over the set's channels; same bound
    Q = sum(emu_slab_total(q[:, j]) for j in range(cpg)).T
    m = S / (cnt * cpg)
    var = np.maximum(Q / (cnt * cpg) - m * m, 0.0)
    rep = lambda a: torch.from_numpy(np.repeat(a, cpg, axis=1))
    return dict(m=rep(m.astype(np.float32)), istd=rep((1.0 / np.sqrt(var + eps)).astype(np.float32)))


# ======================================================================================================================================
# chains: statistics -> finalize -> apply -> backward against F.batch_norm / F.group_norm autograd
# ======================================================================================================================================
def chain_ref(X, dA, ga, be, slope, groups, cpg=0, half=False):
    """float64 autograd reference of the whole chain on X [groups * M, C] (BatchNorm: `groups` independent batches; GroupNorm: groups =
    samples, sets of cpg channels) and its bounds.  The bounds are those of the single kernels with the errors of the kernels in
    front propagated to first order:
      slabs -> mean, istd   finalize_ref(slab_err): dm, and d istd / istd <= dvar / (2 (var + eps)) with dvar carrying the conditioning
                            E[x^2] / (var + eps) of var = E[x^2] - m^2 through gamma(t) E[x^2]
      y                     |is ga| dmu + |(z - mu) ga| dis on top of the apply bound
      xh                    is dmu + |z - mu| dis
      sums                  sum|dy| dxh on sum(dy xh)
      dz                    |ga| dis |dy - sd / n - xh sx / n| + |ga is| (dxh |sx| / n) on top of the backward bound."""
    rows, C = X.shape
    M = rows // groups
    st = stats_ref(X, groups, C)
    es, eq = st["ts"].clone(), st["tq"].clone()
    # a constant channel whose value v has v and v^2 on a coarse dyadic grid (1.5: quanta of 2^-1 and 2^-2) has EXACT fp32 slabs: every
    # partial sum is an integer number of quanta below 2^24
    const = (X == X[:1]).all(0)
    for c in torch.nonzero(const).flatten().tolist():
        v = float(X[0, c])
        if v * 4 == round(v * 4) and v * v * 4 * st["g"]["rpb"] < 2 ** 24:
            es[c], eq[c] = 0, 0
    # statistics from the EXACT float64 slabs (= from the data), errors of the fp32 slabs as slab_err
    if cpg:
        fin = gn_finalize_ref(st["s"], st["q"], C, cpg, groups, M, slab_err=(es, eq))
    else:
        fin = finalize_ref(st["s"], st["q"], C, groups, M, slab_err=(es, eq))
    x = X.double().view(groups, M, C).clone().requires_grad_(True)
    g64, b64 = ga.double().clone().requires_grad_(True), be.double().clone().requires_grad_(True)
    outs = []
    for g in range(groups):
        if cpg:
            yn = F.group_norm(x[g].t().reshape(1, C, M), C // cpg, g64, b64, EPS_BN).reshape(C, M).t()
        else:
            yn = F.batch_norm(x[g], None, None, g64, b64, True, 0.0, EPS_BN)
        outs.append(F.leaky_relu(yn, f32(slope)))
    a = torch.stack(outs)
    a.backward(dA.double().view(groups, M, C))
    prm = dict(mu=fin["m"].float(), istd=fin["istd"].float(), ga=ga, be=be)
    dmu, dis = fin["tm"][:, None], fin["ti"][:, None]
    z = X.double().view(groups, M, C)
    mu, istd = fin["m"][:, None], fin["istd"][:, None]
    gad = ga.double()
    ey = ((istd * gad).abs() * dmu + ((z - mu) * gad).abs() * dis)           # the chain's share of the error of y
    prm64 = dict(mu=fin["m"], istd=fin["istd"], ga=ga, be=be)
    _, _, by = preact(X, prm64, groups)
    by = by.view(groups, M, C) + ey
    s = f32(slope)
    ta = torch.where(a.detach() < 0, by * abs(s) + U * a.detach().abs(), by)
    # backward
    br = bwd_ref(dA, X, prm64, slope, groups, cpg=cpg)
    xh = (z - mu) * istd
    dxh = istd * dmu + (z - mu).abs() * dis
    yv = xh * gad + be.double()
    dy = torch.where(yv >= 0, dA.double().view(groups, M, C), dA.double().view(groups, M, C) * s)
    esx = (dy.abs() * dxh).sum(1)                                            # [groups, C]
    sd, sx = br["sums"][:, 0], br["sums"][:, 1]
    if cpg:
        n = float(M * cpg)
        esx = (esx * gad.abs()).view(groups, C // cpg, cpg).sum(2, keepdim=True).expand(groups, C // cpg, cpg).reshape(groups, C)
        inner = (gad * dy - sd[:, None] / n - xh * sx[:, None] / n).abs()
        tz = br["tz"].view(groups, M, C) + dis * inner + istd.abs() * (dxh * sx[:, None].abs() + xh.abs() * esx[:, None]) / n
        tg = br["tg"] + (dy.abs() * dxh).sum((0, 1))
    else:
        n = float(M)
        inner = (dy - sd[:, None] / n - xh * sx[:, None] / n).abs()
        gi = (gad * istd).abs()
        tz = br["tz"].view(groups, M, C) + gad.abs() * dis * inner + gi * (dxh * sx[:, None].abs() + xh.abs() * esx[:, None]) / n
        tg = br["tg"] + esx.sum(0)
    if half:
        ta = ta + H_REL * (a.detach().abs() + ta) + H_ABS
        tz = tz + H_REL * (x.grad.abs() + tz) + H_ABS
    cond = ((z * z).mean(1) / (fin["var"] + EPS_BN))
    live = fin["var"] > 0                                                    # without the constant channel of the offset kind
    return dict(cond_live=float(cond[live].max()), fin=fin, prm=prm, a=a.detach().reshape(rows, C), ta=ta.reshape(rows, C), dz=x.grad.reshape(rows, C), tz=tz.reshape(rows, C),
                dgamma=g64.grad, dbeta=b64.grad, tg=tg, tb=br["tb"], ey=ey.reshape(rows, C), cond=float(cond.max()), st=st)


def chain_inputs(seed, C, M, groups, kind, slope, half=False, cpg=0):
    """inputs of a chain with the pre-activations settled away from zero against the chain's own bound"""
    g = gen(seed, C, M, groups)
    X = values(g, groups * M, C, kind, half)
    dA = values(g, groups * M, C, "wide", half, (-4, 0) if half else (-3, 3))     # f16: dz of the constant channel (istd = 316) stays finite
    p = params(g, 1, C, "wide")
    moved = 0
    for _ in range(12):                                                      # moving elements moves the statistics a little: settle again
        c = chain_ref(X, dA, p["ga"], p["be"], slope, groups, cpg, half)
        prm64 = dict(mu=c["fin"]["m"], istd=c["fin"]["istd"], ga=p["ga"], be=p["be"])
        X2, n = settle(X, prm64, groups, half, extra=c["ey"], factor=16)     # twice the window that is asserted: the loop ends
        if kind == "offset":
            X2[:, C - 1] = 1.5
        if n == 0 or bool((X2 == X).all()):
            break
        X, moved = X2, moved + n
    return X, dA, p["ga"], p["be"], moved


# ======================================================================================================================================
# case tables
# ======================================================================================================================================
STATS_C = (4, 8, 12, 16, 20, 48, 64, 256, 260, 512, 1024)
STATS_M = (1, 15, 17, 513, 8193)
# (C, M per group, groups, kind, pad, column offset): every C with every M up to 513, M = 8193 (512 blocks of 17 rows, the last 30 empty)
# at the narrow C only (the geometry does not depend on C); groups and kinds cycle through all nine combinations
STATS_CASES = []
for _M in STATS_M:
    for _C in STATS_C:
        if _M == 8193 and _C > 20:
            continue
        _i = len(STATS_CASES)
        STATS_CASES.append((_C, _M, 1 + _i % 3, KINDS[(_i // 3) % 3], 8 * (_i % 2), 4 * ((_i // 2) % 2) * (_i % 2)))
STATS_BIG = (4, 2048 * 512 + 777, 1, "exact", 0, 0)                          # the 2048-block cap: rpb = 513


@functools.lru_cache(maxsize=4)
def stats_case(i, half):
    C, M, groups, kind, pad, off = STATS_BIG if i < 0 else STATS_CASES[i]
    X = values(gen(11, C, M, groups), groups * M, C, kind, half)
    r = stats_ref(X, groups, C)
    return dict(C=C, M=M, groups=groups, kind=kind, ld=C + pad, off=off, X=X, **r)


FIN_NPG = (1, 255, 256, 257, 2047, 2048, 2049, 2053)
FIN_C = (1, 3, 16)
FIN_CNT = (1, 2, 10 ** 6)
FIN_MODES = ("none", "running", "defer0", "defer1", "deferlast")
FIN_CASES = []
for _g in (1, 2, 3):
    for _n in FIN_NPG:
        _i = len(FIN_CASES)
        FIN_CASES.append((_n, FIN_C[(_i + _i // 3) % 3], _g, FIN_CNT[(_i // 2) % 3], FIN_MODES[_i % 5]))


def defer_from(mode, groups):
    return {"defer0": 0, "defer1": min(1, groups - 1), "deferlast": groups - 1}.get(mode)


@functools.lru_cache(maxsize=4)
def fin_case(i):
    npg, C, groups, cnt, mode = FIN_CASES[i]
    g = gen(23, i)
    s, q = fin_slabs(g, C, groups, npg, cnt)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return dict(npg=npg, C=C, groups=groups, cnt=cnt, mode=mode, s=s, q=q, rm0=rm0, rv0=rv0, fin=finalize_ref(s, q, C, groups, cnt))


FWD_C = (4, 8, 12, 16, 20, 64, 256)
FWD_M = (1, 7, 1025)
# (C, M per group, groups, kind, slope, nomean)
FWD_CASES = []
for _M in FWD_M:
    for _C in FWD_C:
        _i = len(FWD_CASES)
        FWD_CASES.append((_C, _M, 1 + _i % 3, ("exact", "wide")[(_i // 3) % 2], SLOPES[(_i // 2) % 3], False))
FWD_CASES += [(12, 7, 2, "exact", 0.25, True), (16, 1025, 1, "wide", 0.01, True), (4, 7, 3, "wide", 0.0, True)]
# layouts (pad of Z, offset of Z, pad of A, offset of A): dense, padded, channel slices
LAYOUTS = ((0, 0, 0, 0), (8, 0, 4, 0), (8, 4, 16, 8))
# f16 variants that must agree bit for bit: all strides multiples of 8 and offsets 0 (eight-channel path where C allows), one stride
# not a multiple of 8, a column offset of 4 (both quad path)
H_VARIANTS = ((8, 0, 8, 0), (8, 0, 4, 0), (8, 4, 8, 0))
# the large grids: all four in-flight rows, a second trip with a ragged end (forward); two rows and a second trip (backward)
FWD_BIG_M = 4 * GRID_CAP + 3
BWD_BIG_M = 2 * GRID_CAP + 3
P_ROWS = 5                                            # rows per image of the dropout cases
# (C, images per group, groups, kind, mode, p, salt)
DROP_CASES = [(C, 8, groups, kind, mode, p, salt)
              for (C, kind) in ((8, "exact"), (12, "wide")) for groups in (1, 2) for mode in (1, 2) for p in (0.1, 0.5)
              for salt in (None, 0x1234567)]
DROP_SEED = 0x9E3779B97F4A7C15 ^ 0x51ED270B


@functools.lru_cache(maxsize=8)
def fwd_case(C, M, groups, kind, slope, nomean, half=False, drop=None, with_r=False, seed=31):
    g = gen(seed, C, M, groups, int(half))
    rows = groups * M
    Z = values(g, rows, C, kind, half)
    prm = params(g, groups, C, kind, nozero_shift=drop is not None)
    moved = 0
    if kind != "exact" and not nomean:
        Z, moved = settle(Z, prm, groups, half)
    R = values(g, rows, C, kind, half) if with_r else None
    a, b, keep = fwd_ref(Z, prm, slope, groups, drop, R, half, nomean)
    return dict(C=C, M=M, groups=groups, kind=kind, slope=slope, nomean=nomean, half=half, drop=drop, Z=Z, prm=prm, R=R, ref=a, tol=b,
                keep=keep, moved=moved, bit_exact=kind == "exact" and fwd_roundings(slope, drop, R, half) <= 1)


@functools.lru_cache(maxsize=8)
def bwd_case(C, M, groups, kind, slope, nomean, half=False, drop=None, cpg=0, seed=37):
    g = gen(seed, C, M, groups, int(half))
    rows = groups * M
    # f16 storage: dz holds xh^2 dy-sized terms; four decades each keep it below the largest finite f16 (65504)
    Z = values(g, rows, C, kind, half, (-3, 1) if half else (-3, 3))
    prm = params(g, groups, C, kind, nozero_shift=drop is not None)
    moved = 0
    if kind != "exact" and not nomean:
        Z, moved = settle(Z, prm, groups, half)
    dA = values(g, rows, C, kind, half, (-4, 0) if half else (-3, 3))
    r = bwd_ref(dA, Z, prm, slope, groups, drop, half, nomean, cpg)
    return dict(C=C, M=M, groups=groups, kind=kind, slope=slope, nomean=nomean, half=half, drop=drop, cpg=cpg, Z=Z, dA=dA, prm=prm,
                moved=moved, **r)


def bwd_quanta(c):
    """exact kind, slope 0 or 1/4: dy * xh is a multiple of 2^-9 (dA 2^-3, slope 2^-2, z - mu 2^-3, istd 2^-1); the largest number of such
    quanta a slab's sum of |dy xh| holds - below 2^24 every fp32 partial is exact"""
    return float(c["tslab_q"].max()) / gamma(c["geo"]["t"] + 5) * 2 ** 9


def drop_of(case):
    C, img, groups, kind, mode, p, salt = case
    return (mode, p, DROP_SEED, P_ROWS, salt)


# (NV, X2, Y2, Z2), groups, C, with R
D2S_CASES = [(grid, groups, C, r) for grid in D2S_GRIDS for groups in ((1,) if grid[0] == 1 else (1, 2)) for C in (4, 16) for r in (False, True)]
# (C, cpg, N, voxels per sample)
GN_CASES = [(C, cpg, N, V) for i, (C, cpg) in enumerate(GN_SETS) for N in (1, 2, 3) for V in (1, 33, 1025)
            if (C < 256 or V < 1025) and (N + V + i) % 2 == 0 or (N, V) == (3, 1025) and C < 256]
# (NB, groups, H, W, C)
POOL_CASES = [(NB, groups, H, W, C) for NB in (1, 4) for groups in ((1,) if NB == 1 else (1, 2)) for (H, W) in ((2, 2), (4, 6), (34, 2))
              for C in (4, 20)]
CHAIN_C, CHAIN_M, CHAIN_G = 16, 1025, 2


def pool2(A, NB, H, W, C):
    """2 x 2 maximum of the rows of [NB, H, W, C]"""
    t = A.view(NB, H // 2, 2, W // 2, 2, C)
    return t.amax((2, 4)).reshape(NB * (H // 2) * (W // 2), C)
