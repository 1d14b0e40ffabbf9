"""Inputs, float64 / int64 references, per-element tolerances and fp32 emulations shared by tests/test_glue_kernels_gpu.py (the 22
entry points of csrc/glue.hip called one at a time) and tests/test_glue_kernels_cpu.py (the same bounds held against an fp32
op-by-op emulation of every bounded formula, the input conditions, and planted errors).  Plain CPU torch / numpy; nothing here
touches a GPU, the oracle, a golden file or another HIP route.

Every reference is float64 (int64 for the integer kernels) computed from the SAME fp32 input values the kernel reads.  Integer
kernels, pure selects and copies are compared with torch.equal.  Every other output is held per element to k u sum|terms| with
u = 2^-24 and k the longest fp32 rounding chain read off the kernel; the derivations stand beside the tolerance functions.  The
counts k below are in units of u and depend on the data where the kernel's error does (|x - max| enters the error of an exponential);
U1 = u (1 + 2^-10) turns the first-order sums into true bounds (the chains stay far below 2^10 roundings).

Assumed for the device math library, as in tests/loss_kernel_refs.py: expf within 2 u relative, logf within 2 u relative, on top
of the propagated error of their argument.  A result below the smallest normal fp32 number (2^-126) may be flushed or rounded as a
denormal: FLOOR = 2^-125 is added wherever an exponential may underflow.  The fp64 accumulations of the partial / final kernels add
nothing at this level, so the bound of a sum over rows is the sum of the row bounds - plus acc64(n) sum|terms|, the n - 1 fp64 additions
of n terms in any order ((n - 1) 2^-53 each at most), which is all that is left where the terms themselves are exact (a sum of fp32
values in fp64 is exact only while their magnitudes span less than 2^29: saturated probabilities span more)."""
import functools
import math

import numpy as np
import torch

from loss_kernel_refs import SENTINEL, U, gamma, gen

ISENT = -7
U1 = U * (1.0 + 2.0 ** -10)
FLOOR = 2.0 ** -125
TINY = 1e-300
EXP_K = 2.0                                           # expf: 2 u relative
LOG_K = 2.0                                           # logf: 2 u relative
GL_MAXC = 32
CANCEL64 = 2.0 ** -50 / U                             # fp64 roundings of a cancelling fp64 expression, in units of u
EPS_ENT = float(torch.tensor(1e-10, dtype=torch.float32))    # the 1e-10f of the entropy, as the kernel sees it


def acc64(n):
    return n * 2.0 ** -53


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def padded(t, pad, value=SENTINEL):
    """[rows][d] -> [rows][d + pad] with the sentinel in the pad columns (an input pad must not be read: a sentinel there would show)"""
    out = torch.full((t.shape[0], t.shape[1] + pad), value, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ======================================================================================================================================
# shared: the log-sum-exp of a row as every loss kernel here forms it
# ======================================================================================================================================
# d_c = x_c - mx (one rounding: absolute u |d_c|, which is a RELATIVE u |d_c| on the exponential), e_c = expf(d_c) (2 u):
#   e_c within ke_c u relative, ke_c = 2 + |d_c|.
# s = sum_c e_c, C positive terms added in sequence: C - 1 roundings, each relative to a partial sum <= s, plus the weighted error of
# the terms:   s within ks u relative, ks = (C - 1) + sum_c (e_c / s) ke_c.
# logf(s): absolute ks u (the relative error of its argument) + 2 u |log s|.
# lse = mx + logf(s): one more rounding:   lse within klse u ABSOLUTE, klse = ks + 2 |log s| + |lse|.
def lse_parts(x32):
    x = x32.double()
    C = x.shape[1]
    mx = x.max(1, keepdim=True).values
    d = x - mx
    e = d.exp()
    s = e.sum(1, keepdim=True)
    p = e / s
    ke = EXP_K + d.abs()
    ks = (C - 1) + (p * ke).sum(1, keepdim=True)
    logs = s.log()
    lse = mx + logs
    klse = ks + LOG_K * logs.abs() + lse.abs()
    return dict(x=x, mx=mx, d=d, e=e, s=s, p=p, ke=ke, ks=ks, logs=logs, lse=lse, klse=klse)


def emu_lse(x):
    """fp32, op by op"""
    mx = x.max(1, keepdim=True).values
    d = x - mx
    e = d.exp()
    s = e.sum(1, keepdim=True)
    return mx, d, e, s


# ======================================================================================================================================
# (1) arco_softmax_rows
# ======================================================================================================================================
# p_c = e_c / s: ke_c + ks + 1 roundings:                                   tol_p = U1 (ke_c + ks + 1) p_c + FLOOR
# max: the maximum is 1-Lipschitz in the sup norm:                          tol_max = max_c tol_p
# entropy = -sum_c t_c, t_c = p_c * logf(p_c + 1e-10f).  a = p_c + 1e-10f: absolute tol_p + u a, i.e. relative ka = tol_p / (u a) + 1;
# logf(a): absolute ka u + 2 u |log a|; times p_c: p_c (ka + 2 |log a|) u, and the error of the factor p_c itself (kp |t_c| u), the
# rounding of the product (|t_c| u) and the C - 1 additions ((C - 1) |t_c| u each):
#     tol_ent = U1 sum_c [ p_c ka_c + (2 + kp_c + 1 + C - 1) |t_c| ] + 25 C FLOOR        (|log a| <= 23.1)
# arg-max: exact on rows of bit-equal logits (e_c = 1 for every c, s = C, all p equal: the first wins) and wherever the float64
# top-two gap exceeds tol_p of the two; the rest is left out (decided rows are at least 99.9 % of every case: CPU file).
#                 C   M    P    pad scale
SOFTMAX_CASES = [(1, 1, 1, 0, 1.0),
                 (1, 257, 257, 2, 1.0),
                 (2, 255, 255, 0, 1.0),
                 (2, 256, 256, 1, 40.0),
                 (4, 256, 256, 3, 40.0),
                 (4, 257, 257, 0, 1.0),
                 (5, 257, 257, 0, 1.0),
                 (5, 255, 85, 2, 40.0),             # three images
                 (19, 255, 85, 5, 1.0),             # three images, padded rows
                 (19, 1, 1, 0, 40.0),
                 (32, 257, 257, 0, 40.0),
                 (32, 255, 85, 4, 1.0),
                 (32, 256, 256, 0, 1.0),
                 (2, 524288 + 300, 524288 + 300, 0, 1.0),      # gl_grid caps at 2048 blocks: 300 threads take a second row
                 (2, 524288 + 300, (524288 + 300) // 4, 2, 1.0)]    # ... and the plane index n changes inside the second trip (4 images)


@functools.lru_cache(maxsize=None)
def softmax_case(i):
    """rows r % 7 == 3: all C logits bit-equal; the rest randn * scale (scale 40: most rows saturate, p == 1 and entropy -0.0)"""
    C, M, P, pad, scale = SOFTMAX_CASES[i]
    g = gen(21, i)
    x = torch.randn((M, C), generator=g) * scale
    equal = (torch.arange(M) % 7) == 3
    x[equal] = x[equal][:, :1].expand(-1, C).clone()
    L = lse_parts(x)
    p = L["p"]
    kp = L["ke"] + L["ks"] + 1
    tol_p = U1 * kp * p + FLOOR
    a = p + EPS_ENT
    la = a.log()
    t = p * la
    ka = tol_p / (U * a) + 1
    tol_ent = U1 * (p * ka + (LOG_K + kp + 1 + C - 1) * t.abs()).sum(1) + 25 * C * FLOOR
    top = torch.topk(p, min(2, C), dim=1)
    if C > 1:
        gap = top.values[:, 0] - top.values[:, 1]
        decided = gap > tol_p.gather(1, top.indices).sum(1)
    else:
        decided = torch.ones(M, dtype=torch.bool)
    amax = torch.where(equal, torch.zeros(M, dtype=torch.int64), top.indices[:, 0])
    decided = decided | equal
    # saturated rows: every other class further than 110 below the maximum: expf underflows to exactly 0, p == 1, entropy == -0.0
    sat = ((L["d"] < -110) | (L["d"] == 0)).all(1) & ((L["d"] == 0).sum(1) == 1)
    planes = lambda v: v.view(M // P, P, C).permute(0, 2, 1).contiguous()
    return dict(C=C, M=M, P=P, ld=C + pad, X=padded(x, pad), x=x, equal=equal, sat=sat, decided=decided, amax=amax,
                ref=dict(prob=planes(p), maxp=p.max(1).values, ent=-t.sum(1)),
                tol=dict(prob=planes(tol_p), maxp=tol_p.max(1).values, ent=tol_ent))


def emu_softmax(c):
    x, M, P, C = c["x"], c["M"], c["P"], c["C"]
    mx, d, e, s = emu_lse(x)
    p = e / s
    ent = torch.zeros(M)
    for k in range(C):
        ent = ent + p[:, k] * torch.log(p[:, k] + torch.tensor(1e-10, dtype=torch.float32))
    return dict(prob=p.view(M // P, P, C).permute(0, 2, 1).contiguous(), maxp=p.max(1).values, ent=-ent, amax=p.argmax(1))


# ======================================================================================================================================
# (2) arco_label_onehot                                                                                 exact
# ======================================================================================================================================
#                C   M   P
ONEHOT_CASES = [(1, 1, 1), (4, 257, 257), (19, 255, 85), (4, 255, 85), (19, 257, 257), (1, 524288 + 300, 524288 + 300),
                (1, 524288 + 300, (524288 + 300) // 4)]


@functools.lru_cache(maxsize=None)
def onehot_case(i):
    C, M, P = ONEHOT_CASES[i]
    lab = torch.randint(-1, C, (M,), generator=gen(22, i))
    lab[0], lab[M - 1] = -1, C - 1
    cl = lab.clamp_min(0)
    ref = torch.zeros((M, C), dtype=torch.int64)
    ref[torch.arange(M), cl] = 1
    return dict(C=C, M=M, P=P, lab=lab, ref=ref.view(M // P, P, C).permute(0, 2, 1).contiguous())


# ======================================================================================================================================
# (3) arco_sup_loss_fwd / _bwd, arco_dice_probs_fwd / _bwd
# ======================================================================================================================================
# forward, per row (the sums over rows are fp64):
#   ce = logf(s) - (x_l - mx): logf(s) within (ks + 2 |log s|) u, the difference x_l - mx within |d_l| u, the subtraction |ce| u:
#       k_ce = ks + 2 |log s| + |d_l| + |ce|                                       (absolute, units of u)
#   p_c = expf(x_c - lse): the argument within (klse + |x_c - lse|) u absolute, expf 2 u:   kq_c = klse + |log p_c| + 2   (relative)
#   I_c = sum p t (the product with t in {0, 1} is exact): kq_c;   Z_c = sum p * p: 2 kq_c + 1;   Y_c, n_px: exact
#   CE = (float)(S0 / M): tol_S0 / M + u |CE|;   dice = (float)(mean_c 1 - num_c / den_c), num = 2 I + 1e-5, den = Z + Y + 1e-5:
#       tol_dice = mean_c (2 tol_I / den + num tol_Z / den^2) + u |dice|
# backward, per element, with the fp64 `sums` EXACT (the test writes the reference's sums into the workspace):
#   gce = g_ce / (float)M, gd = g_dice / (float)C: one rounding each.  p_c = expf(d_c) / s: kp_c = ke_c + ks + 1.
#   dp_c = -gd * (float)E_c, E_c = (2 t den - 2 num p_c) / den^2 in fp64: the error of p_c gives |gd| (2 num / den^2) p_c kp_c,
#       the rounding to float, of gd and of the product 3 |dp_c|                                             -> e_dp_c
#   dot = sum_c dp_c p_c: p_c e_dp_c + |dp_c p_c| (kp_c + 1) per term, C - 1 additions on sum|dp p|           -> e_dot
#   t1 = gce * (p_c - t): |gce| (p_c kp_c + |p_c - t|) + 2 |t1|
#   t2 = p_c * (dp_c - dot): p_c (e_dp_c + e_dot + |dp_c - dot|) + |t2| (kp_c + 1)
#   dX = t1 + t2: + |dX|.   (A fused multiply-add only removes roundings.)
#   E_c cancels where p_c == t (a class that owns every pixel: 2 den - 2 num == 0): there the fp64 roundings of E_c itself are all
#   that is left, in the kernel and in the reference alike: 2^-50 of the magnitude (2 t den + 2 num p_c) / den^2 is added to e_dp.
# dice on probabilities: p is an INPUT.  I, Y: the fp64 additions only; Z = sum p * p: 1;  out as above with the weights; backward:
#   -gd * w_c * (float)E_c with E_c in fp64 from exact inputs: gd, gd * w_c, the rounding to float and the product: 4 |dP|,
#   + 2^-50 |gd w_c| (2 t den + 2 num p) / den^2 for the cancellation of E_c.
#   + FLOOR: a saturated softmax hands over denormal probabilities, and the gradient of such an element is itself below 2^-126.
SUP_C = (1, 2, 3, 4, 5, 8, 9, 19, 21, 32)
#             C   M    pad_in pad_out scale kind
SUP_CASES = [(1, 1, 0, 0, 1.0, "rand"),
             (1, 257, 2, 1, 1.0, "rand"),
             (2, 255, 0, 0, 1.0, "rand"),
             (2, 262144 + 257, 0, 0, 1.0, "rand"),          # 1024 partial blocks (cap), 257 threads take a second row
             (3, 257, 1, 2, 1.0, "absent"),
             (4, 255, 0, 3, 40.0, "rand"),
             (4, 257, 4, 0, 1.0, "owner"),
             (5, 257, 0, 0, 1.0, "rand"),
             (5, 255, 3, 3, 40.0, "absent"),
             (8, 257, 0, 2, 1.0, "rand"),
             (8, 1, 0, 0, 1.0, "rand"),
             (9, 255, 0, 0, 1.0, "rand"),
             (19, 257, 5, 0, 1.0, "absent"),
             (21, 255, 0, 3, 40.0, "rand"),
             (32, 257, 0, 0, 1.0, "rand"),
             (32, 255, 2, 2, 1.0, "owner")]
G_CE, G_DICE = f32(0.7), f32(-1.3)                   # upstream gradients


def sup_labels(g, C, M, kind):
    lab = torch.randint(0, C, (M,), generator=g)
    if kind == "absent" and C > 1:
        lab[lab == C - 1] = 0                         # class C - 1 owns no pixel: dice denominator Z + 1e-5
    if kind == "owner":
        lab[:] = C // 2                               # one class owns every pixel
    return lab


def dice_from_sums(I, Z, Y, w=None):
    C = I.shape[0]
    w = torch.ones(C, dtype=torch.float64) if w is None else w
    return (w * (1.0 - (2.0 * I + 1e-5) / (Z + Y + 1e-5))).sum() / C


@functools.lru_cache(maxsize=None)
def sup_case(i):
    C, M, padi, pado, scale, kind = SUP_CASES[i]
    g = gen(23, i)
    x = torch.randn((M, C), generator=g) * scale
    lab = sup_labels(g, C, M, kind)
    L = lse_parts(x)
    oh = torch.zeros((M, C), dtype=torch.float64)
    oh[torch.arange(M), lab] = 1.0
    p, logs = L["p"], L["logs"]
    d_l = (L["d"] * oh).sum(1, keepdim=True)
    ce = logs - d_l
    k_ce = L["ks"] + LOG_K * logs.abs() + d_l.abs() + ce.abs()
    kq = L["klse"] + (L["x"] - L["lse"]).abs() + EXP_K
    I, Z, Y = (p * oh).sum(0), (p * p).sum(0), oh.sum(0)
    tI = U1 * (p * oh * kq).sum(0) + M * FLOOR + acc64(M) * I
    tZ = U1 * (p * p * (2 * kq + 1)).sum(0) + M * FLOOR + acc64(M) * Z
    sums = torch.cat((ce.sum().view(1), torch.tensor([float(M)], dtype=torch.float64), I, Z, Y))
    tol_sums = torch.cat(((U1 * k_ce.sum() + acc64(M) * ce.abs().sum()).view(1), torch.zeros(1, dtype=torch.float64), tI, tZ, torch.zeros(C, dtype=torch.float64)))
    CE = sums[0] / M
    num, den = 2.0 * I + 1e-5, Z + Y + 1e-5
    dice = dice_from_sums(I, Z, Y)
    out = torch.stack((CE, dice))
    tol_out = torch.stack((tol_sums[0] / M + U1 * CE.abs(), (2 * tI / den + num * tZ / den ** 2).sum() / C + U1 * dice.abs())) + TINY
    # backward: float64 autograd of g_ce CE + g_dice dice
    xa = x.double().clone().requires_grad_(True)
    lp = torch.log_softmax(xa, 1)
    pa = lp.exp()
    loss = G_CE * (-(lp * oh).sum() / M) + G_DICE * dice_from_sums((pa * oh).sum(0), (pa * pa).sum(0), Y)
    loss.backward()
    gce, gd = G_CE / M, G_DICE / C
    kp = L["ke"] + L["ks"] + 1
    E = (2.0 * oh * den - 2.0 * num * p) / den ** 2
    dp = -gd * E
    e_dp = abs(gd) * (2.0 * num / den ** 2) * p * kp + 3 * dp.abs() + abs(gd) * CANCEL64 * (2.0 * oh * den + 2.0 * num * p) / den ** 2
    prod = dp * p
    dot = prod.sum(1, keepdim=True)
    e_dot = (p * e_dp + prod.abs() * (kp + 1)).sum(1, keepdim=True) + (C - 1) * prod.abs().sum(1, keepdim=True)
    t1, t2 = gce * (p - oh), p * (dp - dot)
    e1 = abs(gce) * (p * kp + (p - oh).abs()) + 2 * t1.abs()
    e2 = p * (e_dp + e_dot + (dp - dot).abs()) + t2.abs() * (kp + 1)
    tol_dx = U1 * (e1 + e2 + (t1 + t2).abs()) + FLOOR
    return dict(C=C, M=M, ld=C + padi, ldo=C + pado, X=padded(x, padi), x=x, lab=lab, kind=kind, Y=Y,
                ref=dict(out=out, sums=sums, dx=xa.grad), tol=dict(out=tol_out, sums=tol_sums + TINY, dx=tol_dx),
                dx_formula=t1 + t2)


def emu_sup(c):
    """fp32 op by op; the sums over rows in float64 like the kernel's accumulators"""
    x, lab, C, M = c["x"], c["lab"], c["C"], c["M"]
    oh = torch.zeros((M, C))
    oh[torch.arange(M), lab] = 1.0
    mx, d, e, s = emu_lse(x)
    logs = s.log()
    lse = mx + logs
    ce = logs - (d * oh).sum(1, keepdim=True)
    p = (x - lse).exp()
    I, Z, Y = (p * oh).double().sum(0), (p * p).double().sum(0), oh.double().sum(0)
    sums = torch.cat((ce.double().sum().view(1), torch.tensor([float(M)], dtype=torch.float64), I, Z, Y))
    out = torch.stack((sums[0] / M, dice_from_sums(I, Z, Y))).float()
    # backward from the REFERENCE sums
    rs = c["ref"]["sums"]
    den, num = rs[2 + C:2 + 2 * C] + rs[2 + 2 * C:] + 1e-5, 2.0 * rs[2:2 + C] + 1e-5
    gce = torch.tensor(G_CE) / torch.tensor(float(M))
    gd = torch.tensor(G_DICE) / torch.tensor(float(C))
    v = e / s
    dp = -gd * ((2.0 * oh.double() * den - num * 2.0 * v.double()) / (den * den)).float()
    dot = torch.zeros((M, 1))
    for k in range(C):
        dot = dot + dp[:, k:k + 1] * v[:, k:k + 1]
    dx = gce * (v - oh) + v * (dp - dot)
    return dict(out=out, sums=sums, dx=dx)


DICE_W = (None, "w")


def dice_weights(C):
    return (torch.arange(C, dtype=torch.float32) * 0.37 + 0.25) % 1.5 + 0.125       # non-uniform, fp32


@functools.lru_cache(maxsize=None)
def dice_case(i, weighted):
    """the scores are the fp32 softmax of the supervised case's logits (rows of probabilities, as the trainer passes them)"""
    s = sup_case(i)
    C, M = s["C"], s["M"]
    p32 = torch.softmax(s["x"], 1)
    lab = s["lab"]
    w32 = dice_weights(C) if weighted else None
    w = None if w32 is None else w32.double()
    p = p32.double()
    oh = torch.zeros((M, C), dtype=torch.float64)
    oh[torch.arange(M), lab] = 1.0
    I, Z, Y = (p * oh).sum(0), (p * p).sum(0), oh.sum(0)
    sums = torch.cat((I, Z, Y))
    tol_sums = torch.cat((acc64(M) * I, (U1 + acc64(M)) * Z, torch.zeros(C, dtype=torch.float64)))
    out = dice_from_sums(I, Z, Y, w)
    wa = torch.ones(C, dtype=torch.float64) if w is None else w.abs()
    den, num = Z + Y + 1e-5, 2.0 * I + 1e-5
    tol_out = (wa * (2 * tol_sums[:C] / den + num * tol_sums[C:2 * C] / den ** 2)).sum() / C + U1 * out.abs() + TINY
    pa = p.clone().requires_grad_(True)
    (G_DICE * dice_from_sums((pa * oh).sum(0), (pa * pa).sum(0), Y, w)).backward()
    return dict(C=C, M=M, ld=s["ld"], ldo=s["ldo"], Pm=padded(p32, s["ld"] - C), p32=p32, lab=lab, w32=w32,
                ref=dict(out=out.view(1), sums=sums, dp=pa.grad),
                tol=dict(out=tol_out.view(1), sums=tol_sums + TINY,
                         dp=gamma(4) * pa.grad.abs() + 2.0 ** -50 * abs(G_DICE / C) * wa * (2.0 * oh * den + 2.0 * num * p) / den ** 2 + FLOOR))


def emu_dice(c):
    p, lab, C, M, w = c["p32"], c["lab"], c["C"], c["M"], c["w32"]
    oh = torch.zeros((M, C))
    oh[torch.arange(M), lab] = 1.0
    I, Z, Y = (p * oh).double().sum(0), (p * p).double().sum(0), oh.double().sum(0)
    out = dice_from_sums(I, Z, Y, None if w is None else w.double()).float().view(1)
    rs = c["ref"]["sums"]
    den, num = rs[C:2 * C] + rs[2 * C:] + 1e-5, 2.0 * rs[:C] + 1e-5
    gd = torch.tensor(G_DICE) / torch.tensor(float(C))
    ww = torch.ones(C) if w is None else w
    dp = (-gd * ww) * ((2.0 * oh.double() * den - num * 2.0 * p.double()) / (den * den)).float()
    return dict(out=out, sums=torch.cat((I, Z, Y)), dp=dp)


# ======================================================================================================================================
# (4) arco_unsup_loss_fwd / _bwd
# ======================================================================================================================================
# loss = sum_b w_b S_b / N, w_b = n_conf_b / n_valid_b (fp64 of exact counts), S_b = sum of ce over the selected rows of image b (fp64
# of fp32 ce), N = the number of selected rows (exact).  ce as in (3): k_ce = ks + 2 |log s| + |d_l| + |ce|.
#     tol_loss = sum_b w_b U1 sum_sel k_ce / N + u |loss|
# The selection ce > 0 is decidable by construction: every valid row is either POSITIVE (float64 ce >= 1e-3, ten thousand times its
# bound) or a CONSTRUCTED ZERO (the labelled logit exceeds every other by >= 120: each other expf underflows to exactly 0, s == 1,
# logf(1) == 0, x_l - mx == 0: ce == 0 in fp32 under any association).  The reference selects the positive rows.
# An image without a selected row contributes nothing (masked_select(w, ce > 0) never picks one of its pixels), whatever n_conf / 0 is.
# backward, with the fp64 stats EXACT (written into the workspace by the test): gs = g / (float)N (one rounding; (float)N exact),
# w = gs * (float)w_b (two), p_c = expf(x_c - lse) (kq_c as in (3)), p_c - t (one), the product (one):
#     tol_dx = U1 (|w| (p_c kq_c + |p_c - t|) + 4 |dx|) + FLOOR;   rows not selected: exactly 0.
UNSUP_THR = 0.75
CONF_VALUES = (0.25, 0.5, 0.75, 1.0)                  # the threshold occurs in conf: the >= edge
G_UNSUP = f32(1.7)
#               B  P    C  pad_in pad_out scale special
UNSUP_CASES = [(1, 1, 2, 0, 0, 1.0, None),
               (1, 131072 + 300, 2, 0, 0, 1.0, None),        # 512 slabs: 300 threads take a second pixel
               (1, 255, 4, 0, 0, 1.0, "all_invalid"),
               (2, 255, 4, 1, 2, 1.0, None),
               (2, 257, 2, 0, 0, 1.0, "all_invalid"),
               (3, 257, 19, 0, 0, 1.0, "one_invalid"),
               (3, 1, 4, 0, 0, 1.0, None),
               (4, 255, 2, 0, 3, 3.0, None),
               (4, 257, 19, 3, 0, 1.0, "one_invalid"),
               (7, 257, 4, 2, 0, 1.0, "one_invalid"),
               (7, 255, 2, 0, 0, 1.0, None),
               (8, 255, 19, 0, 0, 1.0, None),
               (8, 257, 4, 0, 1, 3.0, "one_invalid"),
               (9, 257, 4, 0, 0, 1.0, "one_invalid"),
               (9, 255, 2, 1, 1, 1.0, None)]


@functools.lru_cache(maxsize=None)
def unsup_case(i):
    B, P, C, padi, pado, scale, special = UNSUP_CASES[i]
    M = B * P
    g = gen(24, i)
    x = torch.randn((M, C), generator=g) * scale
    lab = torch.randint(-1, C, (M,), generator=g)
    if P == 1:
        lab = lab.clamp_min(0)
    conf = torch.tensor(CONF_VALUES)[torch.randint(0, 4, (M,), generator=g)]
    conf[0] = UNSUP_THR
    # constructed zeros: ~6 % of the rows, and every valid row whose float64 ce falls below 1e-3
    ce0 = torch.logsumexp(x.double(), 1) - x.double().gather(1, lab.clamp_min(0).view(-1, 1)).squeeze(1)
    make_zero = ((torch.rand(M, generator=g) < 0.06) & (torch.arange(M) % P != 0)) | ((ce0 < 1e-3) & (lab >= 0))
    if P == 1 and B == 1:
        make_zero[:] = ce0 < 1e-3
    zr = torch.nonzero(make_zero & (lab >= 0)).flatten()
    x[zr] = x[zr].clamp(-8.0, 8.0)
    x[zr, lab[zr]] = x[zr].max(1).values + 121.0
    if special == "one_invalid":
        lab[(B // 2) * P:(B // 2 + 1) * P] = -1
    if special == "all_invalid":
        lab[:] = -1
    valid = lab >= 0
    L = lse_parts(x)
    oh = torch.zeros((M, C), dtype=torch.float64)
    oh[torch.arange(M)[valid], lab[valid]] = 1.0
    d_l = (L["d"] * oh).sum(1)
    logs = L["logs"].squeeze(1)
    ce = logs - d_l
    x_l_is_max = d_l == 0
    constructed = valid & x_l_is_max & ((L["d"] + oh * -1e9).max(1).values <= -120.0) if C > 1 else valid & False
    positive = valid & (ce >= 1e-3)
    sel = positive
    k_ce = L["ks"].squeeze(1) + LOG_K * logs.abs() + d_l.abs() + ce.abs()
    img = torch.arange(M) // P
    n_conf = torch.zeros(B, dtype=torch.float64).index_add_(0, img, (conf >= UNSUP_THR).double())
    n_valid = torch.zeros(B, dtype=torch.float64).index_add_(0, img, valid.double())
    n_sel = torch.zeros(B, dtype=torch.float64).index_add_(0, img, sel.double())
    S = torch.zeros(B, dtype=torch.float64).index_add_(0, img, torch.where(sel, ce, torch.zeros_like(ce)))
    tS = torch.zeros(B, dtype=torch.float64).index_add_(0, img, torch.where(sel, U1 * k_ce, torch.zeros_like(ce))) + acc64(P) * S
    has = n_sel > 0
    w = torch.where(has, n_conf / n_valid.clamp_min(1.0), torch.zeros(B, dtype=torch.float64))
    N = n_sel.sum()
    loss = (w * S).sum() / N if N > 0 else torch.tensor(math.nan, dtype=torch.float64)
    tol_loss = (w * tS).sum() / N.clamp_min(1.0) + U1 * (loss.abs() if N > 0 else 0.0) + TINY
    stats = torch.cat((w, N.view(1)))
    # backward: float64 autograd of the reference arithmetic
    xa = x.double().clone().requires_grad_(True)
    cea = torch.logsumexp(xa, 1) - (xa * oh).sum(1)
    if N > 0:
        (G_UNSUP * (w[img] * torch.where(sel, cea, torch.zeros_like(cea))).sum() / N).backward()
        dx = xa.grad
    else:
        dx = torch.zeros((M, C), dtype=torch.float64)
    kq = L["klse"] + (L["x"] - L["lse"]).abs() + EXP_K
    wrow = (G_UNSUP / N.clamp_min(1.0) * w[img]).view(-1, 1) * sel.view(-1, 1).double()
    tol_dx = U1 * (wrow.abs() * (L["p"] * kq + (L["p"] - oh).abs()) + 4 * dx.abs()) + FLOOR * sel.view(-1, 1).double()
    return dict(B=B, P=P, C=C, M=M, ld=C + padi, ldo=C + pado, X=padded(x, padi), x=x, lab=lab, conf=conf, special=special,
                valid=valid, positive=positive, constructed=constructed, sel=sel, has=has, ce=ce,
                ref=dict(loss=loss.view(1), stats=stats, dx=dx), tol=dict(loss=tol_loss.view(1), dx=tol_dx))


def emu_unsup(c):
    x, lab, C, M, P, B = c["x"], c["lab"], c["C"], c["M"], c["P"], c["B"]
    valid = lab >= 0
    mx, d, e, s = emu_lse(x)
    logs = s.log().squeeze(1)
    xl = x.gather(1, lab.clamp_min(0).view(-1, 1))
    ce = logs - (xl - mx).squeeze(1)
    sel = valid & (ce > 0)
    img = torch.arange(M) // P
    S = torch.zeros(B, dtype=torch.float64).index_add_(0, img, torch.where(sel, ce, torch.zeros_like(ce)).double())
    n_sel = torch.zeros(B, dtype=torch.float64).index_add_(0, img, sel.double())
    n_conf = torch.zeros(B, dtype=torch.float64).index_add_(0, img, (c["conf"] >= torch.tensor(UNSUP_THR)).double())
    n_valid = torch.zeros(B, dtype=torch.float64).index_add_(0, img, valid.double())
    w = torch.where(n_sel > 0, n_conf / n_valid.clamp_min(1.0), torch.zeros(B, dtype=torch.float64))
    loss = ((w * S).sum() / n_sel.sum()).float().view(1)
    st = c["ref"]["stats"]
    gs = torch.tensor(G_UNSUP) / st[B].float()
    lse = mx + s.log()
    oh = torch.zeros((M, C))
    oh[torch.arange(M)[valid], lab[valid]] = 1.0
    wr = (gs * st[:B].float()[img]).view(-1, 1)
    dx = torch.where(sel.view(-1, 1), wr * ((x - lse).exp() - oh), torch.zeros(()))
    return dict(loss=loss, dx=dx, sel=sel)


# ======================================================================================================================================
# (5) arco_eqv_loss_fwd / _bwd
# ======================================================================================================================================
# per row: lsp = mp + logf(sp), lsq = mq + logf(sq): klse_p, klse_q u absolute.  lt_c = q_c - lsq: klse_q + |lt_c|;  t_c = expf(lt_c):
# relative kt_c = klse_q + |lt_c| + 2.   D_c = lt_c - (p_c - lsp): e_D = klse_q + |lt_c| + klse_p + |p_c - lsp| + |D_c|.
# kl = sum_c t_c D_c (terms with t_c == 0 skipped): |t_c D_c| (kt_c + 1) + t_c e_D per term, C - 1 additions on sum|t D|; kl * m: one more.
#     tol_row = m U1 [ sum_c (|t D| (kt + 1) + t e_D) + (C - 1) sum|t D| + |kl| ] + m C FLOOR (1 + max|D|)
# num_b = fp64 sum of the rows, den_b = sum m + 1e-7 in fp64 (its P additions only); loss = (float)(mean_b num_b / den_b):
#     tol_loss = mean_b tol_num_b / den_b + u |loss|
# backward, with den EXACT in the workspace: w = g * m / (float)(den_b * B): three roundings.  softmax p_c = expf(d_c) / sp:
# kp_c = ke_c + ks + 1, the same for q; the difference and the product with w one rounding each:
#     tol_dP = U1 (|w| (sp_c kp_c + sq_c kq_c + |sp_c - sq_c|) + 4 |dP|) + |w| FLOOR
G_EQV = f32(0.6)
MASK_VALUES = (0.0, 0.5, 1.0, 0.3)
#             B  P    C  padp padq pado special
EQV_CASES = [(1, 1, 1, 0, 1, 0, None),
             (1, 131072 + 300, 4, 0, 0, 0, None),
             (1, 255, 19, 1, 2, 3, "same"),
             (2, 255, 4, 1, 2, 0, None),
             (2, 257, 1, 2, 1, 1, "zero_mask"),
             (3, 257, 19, 0, 3, 0, "zero_mask"),
             (3, 1, 4, 0, 0, 0, None),
             (4, 255, 4, 2, 0, 2, "zero_mask"),
             (4, 257, 1, 0, 0, 0, None),
             (7, 257, 4, 2, 1, 0, "zero_mask"),
             (7, 255, 19, 0, 1, 0, "same"),
             (8, 255, 19, 1, 0, 0, None),
             (8, 257, 4, 0, 2, 1, "zero_mask"),
             (9, 257, 4, 3, 1, 0, "zero_mask"),
             (9, 255, 1, 1, 2, 1, None)]


def eqv_rows(p64, q64, m):
    lp, lq = torch.log_softmax(p64, 1), torch.log_softmax(q64, 1)
    return ((lq.exp() * (lq - lp)).sum(1)) * m


@functools.lru_cache(maxsize=None)
def eqv_case(i):
    """teacher rows r % 11 == 5 are saturated (one logit + 200): t == 0 exactly for every other class (the t > 0 guard)"""
    B, P, C, padp, padq, pado, special = EQV_CASES[i]
    M = B * P
    g = gen(25, i)
    p = torch.randn((M, C), generator=g) * 2.0
    q = torch.randn((M, C), generator=g) * 2.0
    sat = (torch.arange(M) % 11) == 5
    q[sat, 0] += 200.0
    if special == "same":
        q, sat = p.clone(), sat & False
    m = torch.tensor(MASK_VALUES)[torch.randint(0, 4, (M,), generator=g)]
    if P == 1:
        m[:] = 0.3
    if special == "zero_mask":
        m[(B // 2) * P:(B // 2 + 1) * P] = 0.0
    Lp, Lq = lse_parts(p), lse_parts(q)
    m64 = m.double()
    lt = Lq["x"] - Lq["lse"]
    t = lt.exp()
    lpp = Lp["x"] - Lp["lse"]
    D = lt - lpp
    kt = Lq["klse"] + lt.abs() + EXP_K
    e_D = Lq["klse"] + lt.abs() + Lp["klse"] + lpp.abs() + D.abs()
    tD = (t * D).abs()
    kl = (t * D).sum(1)
    tol_row = m64 * (U1 * ((tD * (kt + 1) + t * e_D).sum(1) + (C - 1) * tD.sum(1) + kl.abs()) + C * FLOOR * (1 + D.abs().max(1).values))
    img = torch.arange(M) // P
    num = torch.zeros(B, dtype=torch.float64).index_add_(0, img, kl * m64)
    tnum = torch.zeros(B, dtype=torch.float64).index_add_(0, img, tol_row + acc64(P) * (kl * m64).abs())
    den = torch.zeros(B, dtype=torch.float64).index_add_(0, img, m64) + 1e-7
    loss = (num / den).mean()
    tol_loss = (tnum / den).mean() + U1 * loss.abs() + TINY
    pa = p.double().clone().requires_grad_(True)
    rows = eqv_rows(pa, q.double(), m64)
    (G_EQV * (torch.zeros(B, dtype=torch.float64).index_add_(0, img, rows) / den).mean()).backward()
    w = (G_EQV * m64 / (den[img] * B)).view(-1, 1)
    kp, kq = Lp["ke"] + Lp["ks"] + 1, Lq["ke"] + Lq["ks"] + 1
    tol_dp = U1 * (w.abs() * (Lp["p"] * kp + Lq["p"] * kq + (Lp["p"] - Lq["p"]).abs()) + 4 * pa.grad.abs()) + w.abs() * FLOOR
    return dict(B=B, P=P, C=C, M=M, ldp=C + padp, ldq=C + padq, ldo=C + pado, Pm=padded(p, padp), Qm=padded(q, padq), p=p, q=q, m=m,
                special=special, sat=sat, t=t, ref=dict(loss=loss.view(1), den=den, dp=pa.grad),
                tol=dict(loss=tol_loss.view(1), den=acc64(P + 1) * den, dp=tol_dp))


def emu_eqv(c):
    p, q, m, C, M, P, B = c["p"], c["q"], c["m"], c["C"], c["M"], c["P"], c["B"]
    mp, dp_, ep, sp = emu_lse(p)
    mq, dq_, eq, sq = emu_lse(q)
    lsp, lsq = mp + sp.log(), mq + sq.log()
    kl = torch.zeros((M, 1))
    for k in range(C):
        lt = q[:, k:k + 1] - lsq
        t = lt.exp()
        kl = kl + torch.where(t > 0, t * (lt - (p[:, k:k + 1] - lsp)), torch.zeros(()))
    img = torch.arange(M) // P
    num = torch.zeros(B, dtype=torch.float64).index_add_(0, img, (kl.squeeze(1) * m).double())
    den = torch.zeros(B, dtype=torch.float64).index_add_(0, img, m.double()) + 1e-7
    loss = (num / den).mean().float().view(1)
    rden = c["ref"]["den"]
    w = (torch.tensor(G_EQV) * m / (rden[img] * B).float()).view(-1, 1)
    return dict(loss=loss, den=den, dp=w * (ep / sp - eq / sq))


# ======================================================================================================================================
# (6) arco_entropy_masks, arco_entropy_masks_phase                                                      exact
# ======================================================================================================================================
# float64 restatement of the linear-interpolation percentile over the valid values: virtual index vi = (n - 1) (q / 100), neighbours
# a = sorted[floor(vi)], b = sorted[min(floor(vi) + 1, n - 1)], t = vi - floor(vi), thr = b - (b - a) (1 - t) if t >= 0.5 else
# a + (b - a) t; the threshold is rounded to fp32; low = valid & e <= thr, high = valid & e >= thr; labeled part = lab_l >= 0.
# No valid value: both thresholds NaN (every comparison false).  a + (b - a) t may be contracted to one fused multiply-add on the
# device: thr_alt is the fused value; the masks must equal those of one of the two (they differ only if the two float64 values round
# to different fp32 numbers, which the CPU file shows not to happen for these inputs).
def percentile_thr(vals64, q):
    n = vals64.shape[0]
    if n == 0:
        return math.nan, math.nan
    s = np.sort(vals64)
    nm1 = float(n - 1)
    vi = nm1 * (q / 100.0)
    lo = min(math.floor(vi), nm1)
    hi = min(lo + 1.0, nm1)
    t = vi - lo
    a, b = np.float64(s[int(lo)]), np.float64(s[int(hi)])
    with np.errstate(invalid="ignore"):
        diff = b - a
        thr = b - diff * (1.0 - t) if t >= 0.5 else a + diff * t
        fused = thr
        if math.isfinite(float(a)) and math.isfinite(float(b)):
            from fractions import Fraction as Fr
            ex = (Fr(float(b)) - Fr(float(diff)) * Fr(1.0 - t)) if t >= 0.5 else (Fr(float(a)) + Fr(float(diff)) * Fr(t))
            fused = float(ex)                                      # one rounding of the exact a + diff * t
    return float(thr), fused


def _bytes_values():
    """positive and negative floats whose radix keys differ only in byte 0, 1, 2 or 3"""
    base = 0x3F800000
    bits = [base + i for i in range(0, 256, 5)] + [base + (i << 8) for i in range(0, 256, 7)] + [base + (i << 16) for i in range(0, 128, 3)]
    bits += [(i << 24) | 0x00123456 for i in (0x01, 0x20, 0x3E, 0x40, 0x7E, 0x81, 0xA0, 0xBF, 0xC1, 0xFE)]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def _ent_inputs(name, g):
    r = lambda n: torch.rand(n, generator=g)
    if name in ("n0", "n1", "n2", "n3"):
        k = int(name[1])
        ent, lab = r(300), torch.full((300,), -1, dtype=torch.int64)
        lab[torch.randperm(300, generator=g)[:k]] = 1
        return ent, lab
    if name == "equal":
        return torch.full((257,), 0.625), torch.zeros(257, dtype=torch.int64)
    if name == "half_at_thr":
        ent = torch.cat((torch.full((128,), 0.5), r(64) * 0.25, 0.75 + r(64) * 0.25))      # sorted: 64 below, 128 at 0.5, 64 above
        return ent[torch.randperm(256, generator=g)], torch.zeros(256, dtype=torch.int64)
    if name == "zeros":
        ent = torch.cat((torch.full((100,), -0.0), torch.full((100,), 0.0), r(55)))
        return ent[torch.randperm(255, generator=g)], torch.zeros(255, dtype=torch.int64)
    if name == "special":
        ent = torch.cat((-r(60), r(60), torch.tensor([-0.0, 0.0, math.inf, math.inf]),
                         torch.tensor([1, 2, 3, 0x7FFFFF, 0x400000], dtype=torch.int32).view(torch.float32),
                         -torch.tensor([1, 77], dtype=torch.int32).view(torch.float32)))
        n = ent.shape[0]
        lab = torch.randint(-1, 3, (n,), generator=g)
        lab[120:] = 1                                               # the special values are valid
        perm = torch.randperm(n, generator=g)
        return ent[perm], lab[perm]
    if name == "bytes":
        v = _bytes_values()
        v = torch.cat((v, v[::3]))                                  # with duplicates
        n = v.shape[0]
        return v[torch.randperm(n, generator=g)], torch.randint(-1, 4, (n,), generator=g).clamp_min(-1)
    if name == "big":
        n = 65536 + 300                                             # the selection kernels cap at 256 blocks: a second value per thread
        lab = torch.randint(-1, 4, (n,), generator=g)
        return r(n) * 1.4, lab
    raise KeyError(name)


#               inputs        n_l  q_lo   q_hi
ENT_CASES = [("n0", 0, 20.0, 80.0), ("n0", 5, 20.0, 80.0), ("n1", 3, 20.0, 80.0), ("n2", 0, 20.0, 80.0), ("n2", 0, 50.0, 50.0),
             ("n3", 2, 25.0, 75.0), ("n3", 0, 0.0, 100.0), ("equal", 0, 20.0, 80.0), ("half_at_thr", 4, 50.0, 50.0),
             ("zeros", 0, 30.0, 50.0), ("zeros", 3, 0.0, 78.4), ("special", 7, 50.0, 37.3), ("special", 0, 0.0, 62.0),
             ("bytes", 0, 37.3, 50.0), ("bytes", 9, 12.5, 88.8), ("bytes", 0, 0.0, 100.0),
             ("big", 0, 20.0, 80.0), ("big", 300, 37.3, 62.9), ("big", 0, 0.0, 100.0)]


@functools.lru_cache(maxsize=None)
def ent_case(i):
    name, n_l, q_lo, q_hi = ENT_CASES[i]
    g = gen(26, i)
    ent, lab_u = _ent_inputs(name, g)
    lab_l = torch.randint(-1, 3, (n_l,), generator=g)
    vals = ent[lab_u >= 0].double().numpy()
    thr, alt, fr = [], [], []
    for q in (q_lo, q_hi):
        a, b = percentile_thr(vals, q)
        thr.append(a)
        alt.append(b)
        nm1 = max(vals.shape[0] - 1, 0)
        fr.append(nm1 * (q / 100.0) - math.floor(nm1 * (q / 100.0)))
    t32 = torch.tensor(thr, dtype=torch.float64).float()
    a32 = torch.tensor(alt, dtype=torch.float64).float()
    ok = lab_u >= 0
    lab_part = (lab_l >= 0).float()
    low = torch.cat((lab_part, (ok & (ent <= t32[0])).float()))
    high = torch.cat((lab_part, (ok & (ent >= t32[1])).float()))
    return dict(name=name, ent=ent, lab_u=lab_u, lab_l=lab_l, n_l=n_l, n_u=ent.shape[0], q=(q_lo, q_hi), n_valid=int(ok.sum()),
                thr=thr, thr32=t32, alt32=a32, frac=fr, low=low, high=high)


# ======================================================================================================================================
# (7) arco_mix_unsup, arco_label_presence                                                               exact
# ======================================================================================================================================
MIX_LABELS = (-1, 0, 5, 31, 32, 63, 64, 1000)
#             mode B  Z  Cimg
MIX_CASES = [(m, b, z, ci) for m in (0, 1, 2) for (b, z, ci) in ((1, 1, 1), (2, 3, 3), (33, 1, 3), (33, 3, 1), (2, 1, 1))]
MIX_H, MIX_W = 5, 4


@functools.lru_cache(maxsize=None)
def mix_case(i):
    """desc[i] = {y0, y1, x0, x1, z0, z1, sel_lo, sel_hi}.  Boxes cycle through: empty, the whole image, one pixel at the last row /
    column / slice, random.  Selected sets cycle through {0}, {31}, {32}, {63}, {0, 31, 32, 63}, {5} (sel_hi with bit 31 set is a
    negative int)."""
    mode, B, Z, Cimg = MIX_CASES[i]
    H, W = MIX_H, MIX_W
    g = gen(27, i)
    HW = H * W * Z
    data = torch.randn((B, Cimg, HW), generator=g)
    target = torch.tensor(MIX_LABELS)[torch.randint(0, len(MIX_LABELS), (B, HW), generator=g)]
    logits = torch.rand((B, HW), generator=g)
    for b in range(B):                                              # every selected label occurs, and so do 64 and 1000
        target[b, 0], target[b, 1], target[b, 2] = (0, 31, 32, 63, 0, 5)[b % 6], 64, 1000
    boxes = [(2, 2, 0, W, 0, Z), (0, H, 0, W, 0, Z), (H - 1, H, W - 1, W, Z - 1, Z), (1, 4, 1, 3, 0, Z), (0, 3, 2, W, 0, max(1, Z - 1))]
    sets = [(0,), (31,), (32,), (63,), (0, 31, 32, 63), (5,)]
    desc = torch.zeros((B, 8), dtype=torch.int32)
    keep = torch.zeros((B, HW), dtype=torch.bool)
    p = torch.arange(HW)
    z, q = p % Z, p // Z
    y, x = q // W, q % W
    for b in range(B):
        bx, st = boxes[b % len(boxes)], sets[b % len(sets)]
        sel = sum(1 << s for s in st)
        lo, hi = sel & 0xFFFFFFFF, sel >> 32
        as_int = lambda v: v - (1 << 32) if v >= (1 << 31) else v
        desc[b] = torch.tensor(list(bx) + [as_int(lo), as_int(hi)], dtype=torch.int32)
        if mode == 2:
            t = target[b]
            keep[b] = torch.tensor([0 <= int(v) < 64 and ((sel >> int(v)) & 1) == 1 for v in t])
        else:
            keep[b] = ~((y >= bx[0]) & (y < bx[1]) & (x >= bx[2]) & (x < bx[3]) & (z >= bx[4]) & (z < bx[5]))
    if mode == 1:
        od = torch.where(keep[:, None, :], data, torch.zeros(()))
        ot = torch.where(keep, target, torch.full_like(target, -1))
        ol = torch.where(keep, logits, torch.zeros(()))
    else:
        nxt = (torch.arange(B) + 1) % B
        od = torch.where(keep[:, None, :], data, data[nxt])
        ot = torch.where(keep, target, target[nxt])
        ol = torch.where(keep, logits, logits[nxt])
    return dict(mode=mode, B=B, Z=Z, Cimg=Cimg, H=H, W=W, data=data, target=target, logits=logits, desc=desc, keep=keep,
                odata=od, otarget=ot, ologits=ol)


PRESENCE_HW = (1, 255, 16384 + 5)                      # 64 blocks per image cap at 16 384 pixels


@functools.lru_cache(maxsize=None)
def presence_case(hw):
    """B = 3; image 0: labels from {-1, 0, 63, 64} (+ 7), image 1: only -1 and 64 (empty set), image 2: the single label 63 in its LAST pixel"""
    g = gen(28, hw)
    pool = torch.tensor([-1, 0, 63, 64, 7])
    t = torch.stack((pool[torch.randint(0, 5, (hw,), generator=g)], torch.tensor([-1, 64])[torch.randint(0, 2, (hw,), generator=g)],
                     torch.full((hw,), -1, dtype=torch.int64)))
    t[2, hw - 1] = 63
    ref = []
    for b in range(3):
        m = 0
        for v in torch.unique(t[b]).tolist():
            if 0 <= v < 64:
                m |= 1 << v
        ref.append(m - (1 << 64) if m >= (1 << 63) else m)            # as int64 bit patterns
    return dict(target=t, ref=torch.tensor(ref, dtype=torch.int64))


# ======================================================================================================================================
# (8) arco_overlap_counts                                                                                exact
# ======================================================================================================================================
#                n    C   outside
OVERLAP_CASES = [(1, 1, "none"), (257, 2, "one"), (257, 19, "both"), (257, 32, "both"), (262144 + 300, 2, "both"), (262144 + 300, 32, "one"),
                 (1, 32, "one"), (257, 1, "both")]


@functools.lru_cache(maxsize=None)
def overlap_case(i):
    n, C, outside = OVERLAP_CASES[i]
    g = gen(29, i)
    pred = torch.randint(0, C, (n,), generator=g)
    gt = torch.where(torch.rand(n, generator=g) < 0.6, pred, torch.randint(0, C, (n,), generator=g))
    bad = torch.tensor([-1, C, C + 31, -5])
    if outside in ("one", "both"):
        k = torch.rand(n, generator=g) < 0.2
        pred = torch.where(k, bad[torch.randint(0, 4, (n,), generator=g)], pred)
    if outside == "both":
        k = torch.rand(n, generator=g) < 0.2
        gt = torch.where(k, bad[torch.randint(0, 4, (n,), generator=g)], gt)
        gt[n - 1] = pred[n - 1] = -1 if n > 1 else C              # equal AND outside: must not count
    ref = torch.zeros((C, 3), dtype=torch.int64)
    for c in range(C):
        ref[c, 0], ref[c, 1], ref[c, 2] = (pred == c).sum(), (gt == c).sum(), ((pred == c) & (gt == c)).sum()
    return dict(n=n, C=C, pred=pred, gt=gt, ref=ref.flatten())


# ======================================================================================================================================
# (9) arco_window_accumulate + arco_score_finalize                                                       exact
# ======================================================================================================================================
# scores: the same fp32 additions in launch order and one fp32 division, in numpy float32.  The buffers start from a previous
# accumulation (random scores, counts >= 1), so that no voxel divides by zero.  label = first maximum of the scores.
WINDOW_VOL = (8, 7, 5)
WINDOW_SETS = {1: ((4, 4, 1), [(0, 0, 4), (2, 1, 4), (4, 3, 4)]),          # pz = 1; the last is flush with the far corner (8, 7, 5)
               2: ((5, 4, 2), [(0, 0, 0), (2, 2, 1), (3, 3, 3)])}
WINDOW_C = (1, 2, 5)


@functools.lru_cache(maxsize=None)
def window_case(C, pz):
    ww, hh, dd = WINDOW_VOL
    (px, py, pz_), starts = WINDOW_SETS[pz]
    g = gen(30, C, pz)
    score0 = torch.rand((C, ww, hh, dd), generator=g)
    cnt0 = torch.randint(1, 3, (ww, hh, dd), generator=g).float()
    probs = [torch.rand((C, px, py, pz_), generator=g) for _ in starts]
    if C > 1:                                                      # classes 0 and C - 1 bit-equal (and maximal) in every second voxel of x
        score0[C - 1, ::2] = score0[0, ::2] = score0[0, ::2] + 2.0
        for p in probs:
            p[C - 1] = p[0]
    s, n = score0.numpy().copy(), cnt0.numpy().copy()
    for p, (xs, ys, zs) in zip(probs, starts):
        s[:, xs:xs + px, ys:ys + py, zs:zs + pz_] += p.numpy()
        n[xs:xs + px, ys:ys + py, zs:zs + pz_] += np.float32(1.0)
    acc_s, acc_n = torch.from_numpy(s.copy()), torch.from_numpy(n.copy())
    s = s / n[None]
    assert s.dtype == np.float32
    return dict(C=C, patch=(px, py, pz_), starts=starts, score0=score0, cnt0=cnt0, probs=probs, acc_score=acc_s, acc_cnt=acc_n,
                score=torch.from_numpy(s), label=torch.from_numpy(np.argmax(s, 0)))


# ======================================================================================================================================
# (10) arco_tps_grid
# ======================================================================================================================================
# g = sum_k r_k m_k, k ascending from 0: the first product is added to an exact 0, every term meets one product rounding and at most
# NR - 1 additions (a fused multiply-add: fewer):   tol = gamma(NR) sum_k |r_k m_k|
TPS_NR = (1, 4, 7, 12, 28, 32)
TPS_B = (1, 4, 5, 9)
TPS_HW = (1, 255, 257)


@functools.lru_cache(maxsize=None)
def tps_case(nr, b, hw):
    g = gen(31, nr, b, hw)
    rep = torch.randn((hw, nr), generator=g)
    mapping = torch.randn((b, nr, 2), generator=g)
    ref = torch.einsum("pk,bkc->bpc", rep.double(), mapping.double())
    mag = torch.einsum("pk,bkc->bpc", rep.double().abs(), mapping.double().abs())
    return dict(rep=rep, mapping=mapping, ref=ref, tol=gamma(nr) * mag + TINY)


def emu_tps(c):
    rep, mp = c["rep"], c["mapping"]
    out = torch.zeros((mp.shape[0], rep.shape[0], 2))
    for k in range(rep.shape[1]):
        out = out + rep[None, :, k, None] * mp[:, None, k, :]
    return out


# ======================================================================================================================================
# (11) arco_grid_sample_fwd
# ======================================================================================================================================
# ix = (gx + 1) * 0.5 * (W - 1): the addition and the last product round (the factor 0.5 is exact): ix within 2 u |ix|; the clamp of
# border mode is 1-Lipschitz.  The sample is a continuous piecewise-linear function of (ix, iy) - in zeros mode too, a tap outside
# enters and leaves with weight 0 - so the error of the coordinates costs at most e_ix Sx + e_iy Sy, with Sx (Sy) the largest
# difference of two x- (y-) neighbours of the zero-padded slab.  Weights: wx1 = ix - floor(ix) is exact, wx0 = 1 - wx1 one rounding,
# wx * wy one, value * weight one, at most three additions:   + gamma(6) sum_taps |value weight|.
#            NB H  W  D3 C  padx pady Ho Wo
GS_CASES = [(2, 5, 7, 1, 1, 0, 0, 5, 7), (2, 5, 7, 3, 5, 2, 3, 4, 9), (1, 1, 6, 1, 5, 1, 0, 3, 3), (3, 6, 1, 3, 1, 0, 2, 2, 5),
            (1, 1, 1, 1, 5, 0, 0, 2, 2), (2, 4, 4, 1, 5, 3, 1, 6, 3)]


@functools.lru_cache(maxsize=None)
def gs_case(i, border):
    NB, H, W, D3, C, padx, pady, Ho, Wo = GS_CASES[i]
    g = gen(32, i)
    X = torch.randn((NB, H, W, D3, C), generator=g)
    n_out = NB * Ho * Wo
    grid = torch.rand((n_out, 2), generator=g) * 2.4 - 1.2
    one = torch.tensor(1.0)
    up, dn = torch.nextafter(one, torch.tensor(2.0)), torch.nextafter(one, torch.tensor(0.0))
    special = torch.stack((-one, one, -up, up, -dn, dn, torch.tensor(-3.0), torch.tensor(3.0), torch.tensor(0.0)))
    k = min(n_out, 2 * len(special))
    for j in range(k):                                              # x and y walk through the special values out of step
        grid[j, 0] = special[j % len(special)]
        grid[j, 1] = special[(j // 2 + 3) % len(special)]
    g64 = grid.double().view(NB, Ho, Wo, 2)
    ix, iy = (g64[..., 0] + 1) * 0.5 * (W - 1), (g64[..., 1] + 1) * 0.5 * (H - 1)
    eix, eiy = 2 * U1 * ix.abs(), 2 * U1 * iy.abs()
    if border:
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    fx, fy = ix.floor(), iy.floor()
    X64 = X.double()
    ref = torch.zeros((NB, Ho, Wo, D3, C), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    n_idx = torch.arange(NB).view(NB, 1, 1).expand(NB, Ho, Wo)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = (fx + dx).long(), (fy + dy).long()
            wx = (ix - fx) if dx else 1 - (ix - fx)
            wy = (iy - fy) if dy else 1 - (iy - fy)
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = X64[n_idx, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]                 # [NB][Ho][Wo][D3][C]
            term = v * (wx * wy * inside.double())[..., None, None]
            ref += term
            mag += term.abs()
    Xp = torch.zeros((NB, H + 2, W + 2, D3, C), dtype=torch.float64)
    Xp[:, 1:-1, 1:-1] = X64
    Sx = (Xp[:, :, 1:] - Xp[:, :, :-1]).abs().amax((1, 2))                         # [NB][D3][C]
    Sy = (Xp[:, 1:] - Xp[:, :-1]).abs().amax((1, 2))
    tol = eix[..., None, None] * Sx[:, None, None] + eiy[..., None, None] * Sy[:, None, None] + gamma(6) * mag + TINY
    flat = lambda t: t.reshape(NB * Ho * Wo * D3, C)
    return dict(NB=NB, H=H, W=W, D3=D3, C=C, Ho=Ho, Wo=Wo, ldx=C + padx, ldy=C + pady, X=padded(X.reshape(-1, C), padx), x=X,
                grid=grid, border=border, ref=flat(ref), tol=flat(tol))


def emu_grid_sample(c):
    NB, H, W, D3, C, Ho, Wo = (c[k] for k in ("NB", "H", "W", "D3", "C", "Ho", "Wo"))
    g = c["grid"].view(NB, Ho, Wo, 2)
    ix = (g[..., 0] + 1.0) * 0.5 * torch.tensor(float(W - 1))
    iy = (g[..., 1] + 1.0) * 0.5 * torch.tensor(float(H - 1))
    if c["border"]:
        ix, iy = ix.clamp(0.0, float(W - 1)), iy.clamp(0.0, float(H - 1))
    fx, fy = ix.floor(), iy.floor()
    wx1, wy1 = ix - fx, iy - fy
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    out = torch.zeros((NB, Ho, Wo, D3, C))
    n_idx = torch.arange(NB).view(NB, 1, 1).expand(NB, Ho, Wo)
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            xx, yy = (fx + dx).long(), (fy + dy).long()
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = c["x"][n_idx, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]
            out = out + torch.where(inside[..., None, None], v * (wx * wy)[..., None, None], torch.zeros(()))
    return out.reshape(-1, C)


# ======================================================================================================================================
# (12) arco_field_axpb, arco_field_smooth, arco_field_resize
# ======================================================================================================================================
# base grid: step = 2 / (n - 1) (one rounding), step * i (one), -1 + . or 1 - . (one): within u (2 |step i| + |g|) <= 3 u of the
# exact linspace value (|step i| <= 1 on either end, |g| <= 1); n == 1: exactly -1.  v = beta * g (one), alpha * in + v (two, or one
# fused), v + gamma * in2 (two), the clamp is 1-Lipschitz:
#     tol = U1 (3 |beta| + 5 (|beta g| + |alpha in| + |gamma in2|))       (every partial sum is bounded by the sum of the magnitudes)
AXPB_ALPHA, AXPB_BETA, AXPB_GAMMA = f32(0.8), f32(1.3), f32(-0.45)
#              B  H  W
AXPB_SHAPES = [(2, 1, 6), (1, 5, 1), (2, 4, 7), (1, 7, 4), (1, 1, 1)]


def linspace64(n):
    return torch.full((1,), -1.0, dtype=torch.float64) if n == 1 else -1.0 + 2.0 * torch.arange(n, dtype=torch.float64) / (n - 1)


@functools.lru_cache(maxsize=None)
def axpb_case(i, has_in, has_in2, clamp):
    B, H, W = AXPB_SHAPES[i]
    g = gen(33, i)
    a = torch.randn((B, H, W, 2), generator=g)
    b = torch.randn((B, H, W, 2), generator=g)
    base = torch.stack((linspace64(W).view(1, 1, W).expand(B, H, W), linspace64(H).view(1, H, 1).expand(B, H, W)), -1)
    terms = [AXPB_BETA * base]
    if has_in:
        terms.append(AXPB_ALPHA * a.double())
    if has_in2:
        terms.append(AXPB_GAMMA * b.double())
    ref = sum(terms)
    mag = sum(t.abs() for t in terms)
    if clamp:
        ref = ref.clamp(-1.0, 1.0)
    return dict(B=B, H=H, W=W, a=a if has_in else None, b=b if has_in2 else None, clamp=clamp, ref=ref,
                tol=U1 * (3 * abs(AXPB_BETA) + 5 * mag) + TINY)


def emu_linspace(n):
    if n == 1:
        return torch.tensor([-1.0])
    i = torch.arange(n, dtype=torch.float32)
    step = torch.tensor(2.0) / torch.tensor(float(n - 1))
    return torch.where(torch.arange(n) < n // 2, -1.0 + step * i, 1.0 - step * (float(n - 1) - i))


def emu_axpb(c):
    B, H, W = c["B"], c["H"], c["W"]
    base = torch.stack((emu_linspace(W).view(1, 1, W).expand(B, H, W), emu_linspace(H).view(1, H, 1).expand(B, H, W)), -1)
    v = torch.tensor(AXPB_BETA) * base
    if c["a"] is not None:
        v = torch.tensor(AXPB_ALPHA) * c["a"] + v
    if c["b"] is not None:
        v = v + torch.tensor(AXPB_GAMMA) * c["b"]
    return v.clamp(-1.0, 1.0) if c["clamp"] else v


# smooth: at most ks^2 products added in sequence to an exact 0:   tol = gamma(ks^2) sum |w in|
SMOOTH_KS = (1, 3, 9)
SMOOTH_SHAPES = ((1, 2, 3), (2, 9, 11))


@functools.lru_cache(maxsize=None)
def smooth_case(ks, si):
    B, H, W = SMOOTH_SHAPES[si]
    C = 2
    g = gen(34, ks, si)
    x = torch.randn((B, H, W, C), generator=g)
    w = torch.rand((ks, ks), generator=g)
    w = (w / w.sum()).float()
    r = ks // 2
    xp = torch.zeros((B, H + 2 * r, W + 2 * r, C), dtype=torch.float64)
    xp[:, r:r + H, r:r + W] = x.double()
    ref, mag = torch.zeros((B, H, W, C), dtype=torch.float64), torch.zeros((B, H, W, C), dtype=torch.float64)
    emu = torch.zeros((B, H, W, C))
    xp32 = xp.float()
    for dy in range(ks):
        for dx in range(ks):
            t = float(w[dy, dx]) * xp[:, dy:dy + H, dx:dx + W]
            ref += t
            mag += t.abs()
            emu = emu + w[dy, dx] * xp32[:, dy:dy + H, dx:dx + W]
    return dict(B=B, H=H, W=W, C=C, ks=ks, x=x, w=w.contiguous(), ref=ref, tol=gamma(ks * ks) * mag + TINY, emu=emu)


# resize (bilinear, align_corners = False): sy = h / H (one rounding), fy = sy * (Y + 0.5) - 0.5 (two; Y + 0.5 is exact), clamped at 0:
# fy within u (2 sy (Y + 0.5) + |fy|) + u sy (Y + 0.5) <= 4 u (fy + 1); continuous piecewise linear as in (11): e_fy Sy + e_fx Sx with
# the largest neighbour differences of the (edge-replicated) field.  ly = fy - y0 exact, hy = 1 - ly one rounding, the inner
# hx * a + lx * b three, the outer products and the sum two more:   + gamma(6) sum_taps |value weight|.
# Equal sizes: sy == 1, fy == Y, ly == 0, hy == 1: the output is the input, bit for bit.
#                 B  h  w  H  W
RESIZE_CASES = [(2, 3, 4, 7, 9), (1, 8, 9, 3, 4), (2, 1, 5, 1, 9), (1, 1, 4, 3, 2), (2, 5, 6, 5, 6), (1, 1, 1, 4, 3)]


@functools.lru_cache(maxsize=None)
def resize_case(i):
    B, h, w, H, W = RESIZE_CASES[i]
    C = 2
    g = gen(35, i)
    x = torch.randn((B, h, w, C), generator=g)
    x64 = x.double()

    def axis(n_in, n_out):
        s = n_in / n_out
        f = (s * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5).clamp_min(0.0)
        i0 = f.floor().long()
        i1 = i0 + (i0 < n_in - 1).long()
        return f, i0, i1, f - i0

    fy, y0, y1, ly = axis(h, H)
    fx, x0, x1, lx = axis(w, W)
    ref = torch.zeros((B, H, W, C), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for yi, wy in ((y0, 1 - ly), (y1, ly)):
        for xi, wx in ((x0, 1 - lx), (x1, lx)):
            t = x64[:, yi][:, :, xi] * (wy.view(1, H, 1, 1) * wx.view(1, 1, W, 1))
            ref += t
            mag += t.abs()
    Sy = (x64[:, 1:] - x64[:, :-1]).abs().amax((1, 2)) if h > 1 else torch.zeros((B, C), dtype=torch.float64)
    Sx = (x64[:, :, 1:] - x64[:, :, :-1]).abs().amax((1, 2)) if w > 1 else torch.zeros((B, C), dtype=torch.float64)
    efy, efx = 4 * U1 * (fy + 1), 4 * U1 * (fx + 1)
    tol = efy.view(1, H, 1, 1) * Sy.view(B, 1, 1, C) + efx.view(1, 1, W, 1) * Sx.view(B, 1, 1, C) + gamma(6) * mag + TINY
    return dict(B=B, h=h, w=w, H=H, W=W, C=C, x=x, ref=ref, tol=tol, same=(h == H and w == W))


def emu_resize(c):
    B, h, w, H, W, x = c["B"], c["h"], c["w"], c["H"], c["W"], c["x"]

    def axis(n_in, n_out):
        s = torch.tensor(float(n_in)) / torch.tensor(float(n_out))
        f = (s * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5).clamp_min(0.0)
        i0 = f.long()
        i1 = i0 + (i0 < n_in - 1).long()
        l = f - i0.float()
        return i0, i1, l, 1.0 - l

    y0, y1, ly, hy = axis(h, H)
    x0, x1, lx, hx = axis(w, W)
    tap = lambda yi, xi: x[:, yi][:, :, xi]
    hxv, lxv, hyv, lyv = hx.view(1, 1, W, 1), lx.view(1, 1, W, 1), hy.view(1, H, 1, 1), ly.view(1, H, 1, 1)
    return hyv * (hxv * tap(y0, x0) + lxv * tap(y0, x1)) + lyv * (hxv * tap(y1, x0) + lxv * tap(y1, x1))
