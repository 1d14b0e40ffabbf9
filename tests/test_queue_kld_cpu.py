"""The float64 restatement tests/queue_kld_refs.py against torch float64 autograd of the literal KLD / compute_logits expression, and the
places the --kld route is carried that need no GPU: the parser, the constructors, queue_kld's refusal, the header."""
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


def _torch64(cs, ct, Ts, Tt, g):
    """(stats, loss, d cs, d ct) by torch float64 autograd of KLD()(cs / Ts, ct / Tt), times the upstream gradient g."""
    from arco_amd.pretrain_2D import KLD
    a = torch.from_numpy(np.asarray(cs, np.float64)).requires_grad_(True)
    b = torch.from_numpy(np.asarray(ct, np.float64)).requires_grad_(True)
    s, t = a / Ts, b / Tt
    out = KLD()(s, t)
    (out * g).backward()
    with torch.no_grad():
        kl = torch.nn.functional.kl_div(torch.log_softmax(s, 1), torch.softmax(t, 1), reduction="none").sum(1)
        st = torch.stack([torch.logsumexp(s, 1), torch.logsumexp(t, 1), kl], 1)
    return st.numpy(), float(out.detach()), a.grad.numpy(), b.grad.numpy()


def _cases():
    out = [(f"random{i}-{Ts}-{Tt}", *R.cosines(N, L, 10 + i), Ts, Tt) for i, (N, L, _) in enumerate(R.SHAPES[:6]) for Ts, Tt in R.TEMPS]
    for L in (5, 36, 260):
        out += [(f"{k}-{L}", *v) for k, v in R.hand_made(L).items()]
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_refs_against_torch_float64_autograd(case):
    _, cs, ct, Ts, Tt = case
    g = 0.75
    st, lo, ds, dt = _torch64(cs, ct, Ts, Tt, g)
    assert np.isfinite(st).all() and np.isfinite(ds).all()
    bad = ~np.isfinite(dt)
    if bad.any():          # autograd's own target gradient holds 0 * log 0 = NaN where p is exactly 0, and the softmax backward spreads it over
        p_t = np.exp(ct.astype(np.float64) / Tt - st[:, 1:2])          # the row; the restatement keeps kl_div's forward convention: 0
        rt = R.grads(cs, ct, Ts, Tt, g)[1]
        assert case[0].startswith("spike_f64") and (bad.all(axis=1) == (p_t == 0).any(axis=1)).all() and (rt[p_t == 0] == 0).all()
        dt = np.where(bad, rt, dt)
    np.testing.assert_allclose(R.stats(cs, ct, Ts, Tt), st, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.loss(cs, ct, Ts, Tt), lo, rtol=1e-12, atol=1e-13)
    # two float64 evaluations in different orders: logits of size 1 / T = 100 carry 100 * 2^-53 = 1e-14 into every log-probability, and
    # both gradients are differences that may cancel (to exactly 0 in the restatement where cs == ct) - hence a bound relative to the
    # size g / (N T) of a gradient whose probabilities differ by 1
    for r, d, T in zip(R.grads(cs, ct, Ts, Tt, g), (ds, dt), (Ts, Tt)):
        np.testing.assert_allclose(r, d, rtol=1e-9, atol=1e-11 * g / (cs.shape[0] * T))


def test_hand_made_rows_hold_what_they_are_for():
    h = R.hand_made(260)
    cs, ct, Ts, Tt = h["spike"]
    assert Tt == 0.01 and np.exp(np.float32(-2 / Tt)) == 0          # in fp32 every p but the spike's is exactly 0 ...
    cs, ct, Ts, Tt = h["spike_f64"]
    p = np.exp(ct.astype(np.float64) / Tt - R.stats(cs, ct, Ts, Tt)[:, 1:2])
    assert (p == 0).sum() == p.size - 2 and np.isfinite(R.grads(cs, ct, Ts, Tt)[1]).all()      # ... and at T = 0.002 in float64 too: xlogy is in play
    cs, ct, Ts, Tt = h["max_0p05"]
    assert (ct.max(axis=1) == np.float32(0.05)).all() and np.exp(np.float32(0.05 / Tt - 1 / Tt)) < 1e-41       # a fixed shift underflows
    cs, ct, Ts, Tt = h["equal"]
    assert (R.stats(cs, ct, Ts, Tt)[:, 2] == 0).all() and all((g == 0).all() for g in R.grads(cs, ct, Ts, Tt))


def test_queue_kld_torch_route_is_the_literal_expression():
    from arco_amd.pretrain_2D import KLD
    from arco_amd.stage1 import compute_logits, queue_kld
    rs = np.random.RandomState(4)
    zs, zt, q = (torch.from_numpy(rs.standard_normal(s)) for s in ((5, 8), (5, 8), (36, 8)))
    want = KLD()(compute_logits(zs, q, 0.1), compute_logits(zt, q, 0.07))
    assert torch.equal(queue_kld(zs, zt, q, 0.1, 0.07), want) and torch.equal(queue_kld(zs, zt, q, 0.1, 0.07, route="torch"), want)
    cos = lambda z: (torch.nn.functional.normalize(z, dim=1) @ torch.nn.functional.normalize(q, dim=1).T).numpy()      # noqa: E731
    np.testing.assert_allclose(R.loss(cos(zs), cos(zt), 0.1, 0.07), float(want), rtol=1e-12)


def test_unknown_routes_are_refused_before_any_work():
    from arco_amd import pretrain_2D as P2, pretrain_3D as P3
    from arco_amd.model_2D import ISD
    from arco_amd.model_3D import ISD_3d
    from arco_amd.stage1 import queue_kld
    z = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="route"):
        queue_kld(z, z, z, 0.1, 0.1, route="x")          # CPU tensors: the refusal comes before the first GPU call
    for mod in (P2, P3):
        assert mod.build_parser().parse_args([]).kld == "torch"
        assert mod.build_parser().parse_args(["--kld", "fused", "--patch_heads", "fused", "--gpu_ingest", "1"]).kld == "fused"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--kld", "x"])
    for cls in (ISD, ISD_3d):
        with pytest.raises(ValueError, match="kld"):
            cls(K=4, kld="x")
    assert ISD(K=4, num_classes=2, latent_feature_size=8, kld="fused").kld == "fused" and ISD(K=4, num_classes=2, latent_feature_size=8).kld == "torch"


def test_header_declares_the_entry_points():
    from arco_amd import _lib
    P, L, F = _lib._P, _lib._L, _lib._F
    assert _lib._SIGS["arco_queue_kld_fwd"] == [P, P, L, L, L, L, F, F, P, P, P]
    assert _lib._SIGS["arco_queue_kld_bwd"] == [P, P, L, L, L, L, F, F, P, P, P, L, P, L, P]
    assert _lib._QUERIES["arco_queue_kld_short_max"] == ([], L)
    assert 64 < _lib.query("arco_queue_kld_short_max") < 4099          # the shapes of the kernel tests lie on both sides of it
