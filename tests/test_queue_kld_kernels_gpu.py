"""arco_queue_kld_fwd / arco_queue_kld_bwd (csrc/queue_kld.hip) through the C ABI against the float64 restatement tests/queue_kld_refs.py
(held to torch float64 autograd by tests/test_queue_kld_cpu.py), with the torch fp32 route KLD()(cs / Ts, ct / Tt) on the same inputs as the
yardstick: the kernels' largest error may be at most max(2 x the torch fp32 route's own, 2^-20 x the largest magnitude of the float64
tensor), the project's bound for a second fp32 evaluation, on every statistic, the loss and both gradients (-m gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import queue_kld_refs as R        # noqa: E402

pytestmark = pytest.mark.gpu
G = 0.75          # the upstream gradient


def _switch():
    """Rows of up to this length take one wave each, longer ones one workgroup each."""
    from arco_amd import _lib as L
    return int(L.query("arco_queue_kld_short_max"))


def _padded(x, ld):
    """[N, ld] on the device, the columns behind L filled with NaN: a kernel that reads one of them shows it in its statistics."""
    out = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device="cuda")
    out[:, :x.shape[1]] = torch.from_numpy(x)
    return out


def fused(cs, ct, L_, Ts, Tt, want_s=True, want_t=True, in_place=False):
    """(stats [N, 3] float64, loss, dcs or None, dct or None) from the two entry points; cs, ct [N, ld] device tensors, L_ columns used.
    Gradients go to fresh [N, L_] tensors, or over copies of the padded matrices (in_place)."""
    from arco_amd import _lib as L
    N, ld = cs.shape
    stats = torch.full((N, 3), float("nan"), dtype=torch.float64, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    shape = (N, L_, ld, ld, 1.0 / Ts, 1.0 / Tt)
    L.call("arco_queue_kld_fwd", L.ptr(cs), L.ptr(ct), *shape, L.ptr(stats), L.ptr(loss))
    g = torch.tensor([G], dtype=torch.float32, device="cuda")
    if in_place:
        cs, ct = cs.clone(), ct.clone()
        dcs, dct, ld_d = (cs if want_s else None), (ct if want_t else None), ld
    else:
        dcs, dct, ld_d = (torch.full((N, L_), 7.0, device="cuda") if want_s else None), (torch.full((N, L_), 7.0, device="cuda") if want_t else None), L_
    L.call("arco_queue_kld_bwd", L.ptr(cs), L.ptr(ct), *shape, L.ptr(stats), L.ptr(g), L.ptr(dcs), ld_d, L.ptr(dct), ld_d)
    torch.cuda.synchronize()
    cut = lambda d: None if d is None else d[:, :L_]          # noqa: E731
    return stats, loss, cut(dcs), cut(dct)


def torch_route(cs, ct, Ts, Tt):
    """The same four from the tensor library in fp32: the literal KLD expression on the logits cs / Ts, ct / Tt and its autograd."""
    from arco_amd.pretrain_2D import KLD
    a, b = cs.clone().requires_grad_(True), ct.clone().requires_grad_(True)
    s, t = a / Ts, b / Tt
    out = KLD()(s, t)
    (out * G).backward()
    with torch.no_grad():
        kl = torch.nn.functional.kl_div(torch.log_softmax(s, 1), torch.softmax(t, 1), reduction="none").sum(1)
        stats = torch.stack([torch.logsumexp(s, 1), torch.logsumexp(t, 1), kl], 1)
    return stats, out.detach().reshape(1), a.grad, b.grad


def _check(name, cs, ct, ld, Ts, Tt):
    """The module docstring's bound on one problem; the ratios are printed.  Returns the fused results."""
    N, L_ = cs.shape
    ref = (R.stats(cs, ct, Ts, Tt), np.array([R.loss(cs, ct, Ts, Tt)]), *R.grads(cs, ct, Ts, Tt, G))
    dcs, dct = _padded(cs, ld), _padded(ct, ld)
    got = fused(dcs, dct, L_, Ts, Tt)
    tor = torch_route(dcs[:, :L_].contiguous(), dct[:, :L_].contiguous(), Ts, Tt)
    names = ["lse_s", "lse_t", "KL", "loss", "dcs", "dct"]
    split = lambda r: [r[0][:, 0], r[0][:, 1], r[0][:, 2], r[1], r[2], r[3]]          # noqa: E731
    for what, r, g, t in zip(names, split(ref), split(got), split(tor)):
        g, t = g.double().cpu().numpy(), t.double().cpu().numpy()
        assert g.shape == r.shape and np.isfinite(g).all(), (name, what)
        floor = 2.0 ** -20 * float(np.abs(r).max())
        lost = ~np.isfinite(t).all(axis=-1) if what == "dct" else np.zeros(r.shape[:1], bool)
        if lost.any():
            # The torch route's own teacher gradient is NaN in a row with an exact zero of p (0 * log 0 in kl_div's backward, spread over the
            # row by the softmax backward): there is no torch error to double.  Such a row's gradient g p ((log p - log q) - KL_i) / (N Tt)
            # is a difference of fp32 quantities of the size of the logits, each good to an ulp or two of ITSELF, so the rows are held to
            # 2^-20 of the largest TERM of that difference instead of the largest result (which is 0 for a one-spike teacher).
            st = ref[0]
            logp, logq = ct.astype(np.float64) / Tt - st[:, 1:2], cs.astype(np.float64) / Ts - st[:, 0:1]
            terms = G * np.exp(logp) * (np.abs(logp - logq) + np.abs(st[:, 2:3])) / (N * Tt)
            e_l, bound = float(np.abs(g - r)[lost].max()), max(floor, 2.0 ** -20 * float(terms[lost].max()))
            print(f"{name} Ts={Ts} Tt={Tt} dct, {int(lost.sum())} rows the torch route loses: fused error {e_l:.3e}, bound {bound:.3e}, floor {floor:.3e}")
            assert e_l <= bound, (name, what, e_l, bound)
            if lost.all():
                continue
            g, t, r = g[~lost], t[~lost], r[~lost]
        e_g, e_t = float(np.abs(g - r).max()), float(np.abs(t - r).max())
        print(f"{name} Ts={Ts} Tt={Tt} {what}: fused error {e_g:.3e}, torch error {e_t:.3e}, ratio {e_g / max(e_t, 1e-300):.2f}, floor {floor:.3e}")
        assert e_g <= max(2 * e_t, floor), (name, what, e_g, e_t, floor)
    return got


@pytest.mark.parametrize("temps", R.TEMPS, ids=lambda t: f"Ts{t[0]}-Tt{t[1]}")
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_float64(shape, temps):
    N, L_, ld = shape
    cs, ct = R.cosines(N, L_, seed=N + L_)
    assert N * L_ < 1000 or (min(cs.min(), ct.min()) < -0.9 and max(cs.max(), ct.max()) > 0.9)          # the cosines reach both ends of [-1, 1]
    _check(f"random{N}x{L_}", cs, ct, ld, *temps)


@pytest.mark.parametrize("temps", R.TEMPS, ids=lambda t: f"Ts{t[0]}-Tt{t[1]}")
@pytest.mark.parametrize("past", [0, 1, 4])          # the longest one-wave row (16-byte accesses), then one-workgroup rows: scalar, 16-byte
def test_kernels_on_both_sides_of_the_short_row_switch(past, temps):
    L_ = _switch() + past
    assert R.SHAPES[4][1] < _switch() < R.SHAPES[5][1] and _switch() % 4 == 0
    cs, ct = R.cosines(3, L_, seed=L_)
    _check(f"switch+{past}", cs, ct, L_, *temps)


@pytest.mark.parametrize("L_", [37, 260, 1031, 2052])          # one wave or one workgroup a row, scalar or 16-byte accesses
@pytest.mark.parametrize("row", sorted(R.hand_made(8)))
def test_hand_made_rows(row, L_):
    cs, ct, Ts, Tt = R.hand_made(L_)[row]
    stats, loss, dcs, dct = _check(f"{row}{L_}", cs, ct, L_ + (-L_) % 4, Ts, Tt)
    if row == "equal":          # cs == ct, equal temperatures: nothing but zeros
        assert float(loss) == 0.0 and not stats[:, 2].any() and not dcs.any() and not dct.any()
        assert torch.equal(stats[:, 0], stats[:, 1])
    if row == "spike":          # every p but the spike's underflows in fp32
        assert (dct == 0).sum() >= dct.numel() - 2 and torch.isfinite(dct).all()


@pytest.mark.parametrize("L_", [36, 4100, 4099])
def test_a_nan_cosine_reaches_the_loss(L_):
    cs, ct = R.cosines(3, L_, seed=5)
    for side in (0, 1):
        bad = [cs.copy(), ct.copy()]
        bad[side][1, L_ // 2] = np.nan
        stats, loss, _, _ = fused(_padded(bad[0], L_), _padded(bad[1], L_), L_, 0.1, 0.1)
        assert not np.isfinite(float(loss))
        assert torch.isfinite(stats[0]).all() and torch.isfinite(stats[2]).all() and not torch.isfinite(stats[1]).all()


@pytest.mark.parametrize("shape", [(6, 36, 36), (4, 257, 260), (2, 4099, 4099), (3, 4100, 4100)], ids=lambda s: "x".join(map(str, s)))
def test_ten_runs_give_the_same_bits(shape):
    N, L_, ld = shape
    cs, ct = (_padded(x, ld) for x in R.cosines(N, L_, seed=9))
    first = fused(cs, ct, L_, 0.1, 0.01)
    for _ in range(9):
        again = fused(cs, ct, L_, 0.1, 0.01)
        assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("shape", [(6, 36, 36), (4, 257, 260), (2, 4099, 4099), (3, 4100, 4100)], ids=lambda s: "x".join(map(str, s)))
def test_a_side_that_needs_no_gradient_is_skipped_and_gradients_may_replace_the_cosines(shape):
    N, L_, ld = shape
    cs, ct = (_padded(x, ld) for x in R.cosines(N, L_, seed=11))
    both = fused(cs, ct, L_, 0.1, 0.07)
    only_s = fused(cs, ct, L_, 0.1, 0.07, want_t=False)
    only_t = fused(cs, ct, L_, 0.1, 0.07, want_s=False)
    assert only_s[3] is None and only_t[2] is None
    assert torch.equal(only_s[2], both[2]) and torch.equal(only_t[3], both[3])
    keep_s, keep_t = cs.clone(), ct.clone()
    over = fused(cs, ct, L_, 0.1, 0.07, in_place=True)
    assert torch.equal(over[2], both[2]) and torch.equal(over[3], both[3])
    over_s = fused(cs, ct, L_, 0.1, 0.07, want_t=False, in_place=True)
    assert torch.equal(over_s[2], both[2])
    for a, b in ((cs, keep_s), (ct, keep_t)):          # the caller's matrices: only the clones inside fused() were written
        assert torch.equal(a[:, :L_], b[:, :L_])


def test_arguments_are_refused_before_any_launch():
    from arco_amd import _lib as L
    cs, ct = (_padded(x, 40) for x in R.cosines(2, 37, seed=1))
    stats = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    loss = torch.full((1,), 5.0, device="cuda")
    g = torch.ones(1, device="cuda")
    ok = (2, 37, 40, 40, 10.0, 10.0)
    for shape in [(0, 37, 40, 40, 10.0, 10.0), (2, 0, 40, 40, 10.0, 10.0), (2, 37, 36, 40, 10.0, 10.0), (2, 37, 40, 36, 10.0, 10.0),
                  (2, 37, 40, 40, 0.0, 10.0), (2, 37, 40, 40, 10.0, -1.0), (2, 37, 40, 40, float("inf"), 10.0), (2, 37, 40, 40, 10.0, float("nan"))]:
        with pytest.raises(RuntimeError, match="arco_queue_kld_fwd"):
            L.call("arco_queue_kld_fwd", L.ptr(cs), L.ptr(ct), *shape, L.ptr(stats), L.ptr(loss))
        with pytest.raises(RuntimeError, match="arco_queue_kld_bwd"):
            L.call("arco_queue_kld_bwd", L.ptr(cs), L.ptr(ct), *shape, L.ptr(stats), L.ptr(g), L.ptr(cs), 40, L.ptr(ct), 40)
    d = torch.zeros(2, 40, device="cuda")
    for dcs, ld_ds, dct, ld_dt in [(None, 40, None, 40), (ct, 40, None, 40), (None, 40, cs, 40), (d, 40, d, 40), (d, 36, None, 40), (cs, 44, None, 40)]:
        with pytest.raises(RuntimeError, match="arco_queue_kld_bwd"):
            L.call("arco_queue_kld_bwd", L.ptr(cs), L.ptr(ct), *ok, L.ptr(stats), L.ptr(g), L.ptr(dcs), ld_ds, L.ptr(dct), ld_dt)
    with pytest.raises(RuntimeError, match="arco_queue_kld_fwd"):
        L.call("arco_queue_kld_fwd", L.ptr(cs), None, *ok, L.ptr(stats), L.ptr(loss))
    torch.cuda.synchronize()
    assert float(loss) == 5.0 and not stats.any() and not d.any()
