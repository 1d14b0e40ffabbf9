"""arco_patch_head_fwd / arco_patch_head_bwd / arco_patch_head_wgrad_finish (csrc/patch_head.hip) against their statements of
tests/patch_head_refs.py: y, the pooled tensor and d_0 bit for bit, the parameter gradients within one fp32 rounding plus the worst case
of a float64 sum in any order; run-to-run identity; the refusals (-m gpu)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import patch_head_refs as R        # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _geom(n, patch, pool, B, C):
    return (len(n), B, C) + tuple(n) + (1,) * (3 - len(n)) + (patch, pool)


def _chain(layers_d):
    """(the 8 weight / bias pointers, the 4 widths) of a chain on the device, padded to four layers"""
    from arco_amd import _lib as L
    ptrs, widths = [], []
    for W, b in layers_d:
        ptrs += [L.ptr(W), L.ptr(b)]
        widths.append(W.shape[0])
    pad = 4 - len(layers_d)
    return ptrs + [None] * (2 * pad), widths + [0] * pad


def _forward(xd, case, layers_d):
    from arco_amd import _lib as L
    n, patch, pool, B, widths, _ = case
    P = R.positions(case) // (B * pool ** len(n))
    pooled = torch.full((P, B, widths[0]) + (pool,) * len(n), NAN, device="cuda")
    y = torch.full((P * B, widths[-1]) + (pool,) * len(n), NAN, device="cuda")
    ptrs, w4 = _chain(layers_d)
    L.call("arco_patch_head_fwd", L.ptr(xd), *_geom(n, patch, pool, B, widths[0]), len(layers_d), *ptrs, *w4, L.ptr(pooled), L.ptr(y))
    return pooled, y


def _backward(pooled, gyd, case, layers_d, want_d0=True):
    """(d0 or None, [(weight gradient, bias gradient or None)]), every output NaN before the launches"""
    from arco_amd import _lib as L
    n, patch, pool, B, widths, _ = case
    geom = _geom(n, patch, pool, B, widths[0])
    ptrs, w4 = _chain(layers_d)
    n_bytes = L.query("arco_patch_head_ws_bytes", *geom, len(layers_d), *w4)
    assert n_bytes > 0 and n_bytes % 8 == 0
    ws = torch.full((n_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
    d0 = torch.full(pooled.shape, NAN, device="cuda") if want_d0 else None
    L.call("arco_patch_head_bwd", L.ptr(pooled), L.ptr(gyd), *geom, len(layers_d), *ptrs, *w4, L.ptr(d0), L.ptr(ws))
    grads = [(torch.full(W.shape, NAN, device="cuda"), None if b is None else torch.full(b.shape, NAN, device="cuda")) for W, b in layers_d]
    gptrs = [L.ptr(t) for pair in grads for t in pair] + [None] * (2 * (4 - len(layers_d)))
    L.call("arco_patch_head_wgrad_finish", L.ptr(ws), *geom, len(layers_d), *w4, *gptrs)
    return d0, grads


def _same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32))


@pytest.fixture(scope="module", params=list(range(len(R.CASES))), ids=R.CASE_IDS)
def ref(request):
    case = R.CASES[request.param]
    x, layers, gy = R.case_input(case)
    pooled, y = R.head_fwd_f32(x, case[1], case[2], layers)
    d0, grads = R.head_bwd(pooled, gy, layers)
    return dict(case=case, x=x, layers=layers, gy=gy, pooled=pooled, y=y, d0=d0, grads=grads)


def _device(ref):
    xd, gyd = torch.from_numpy(ref["x"]).cuda(), torch.from_numpy(ref["gy"]).cuda()
    layers_d = [(torch.from_numpy(W).cuda(), None if b is None else torch.from_numpy(b).cuda()) for W, b in ref["layers"]]
    return xd, gyd, layers_d


def test_forward_bit_for_bit(ref):
    from arco_amd import _lib as L
    case = ref["case"]
    n, patch, pool, B, widths, _ = case
    xd, _, layers_d = _device(ref)
    pooled1, y1 = _forward(xd, case, layers_d)
    pooled2, y2 = _forward(xd, case, layers_d)
    assert not torch.isnan(y1).any() and not torch.isnan(pooled1).any()          # NaN before the launch: every element is written
    assert _same_bits(pooled1, ref["pooled"])
    assert _same_bits(y1, ref["y"])
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)) and torch.equal(pooled1.view(torch.int32), pooled2.view(torch.int32))
    alone = torch.empty_like(pooled1)
    L.call("arco_patch_pool_fwd", L.ptr(xd), *_geom(n, patch, pool, B, widths[0]), L.ptr(alone))
    assert torch.equal(pooled1, alone)


def test_backward(ref):
    """d_0 bit for bit.  A parameter gradient g against the float64 reference sum s of its n exact terms (n = the position count):
    |g - s| <= 2^-24 * |s| + n * 2^-53 * sum|terms| - one rounding to fp32, and the worst case of a float64 sum taken in any order."""
    case = ref["case"]
    n_pos = R.positions(case)
    if case is R.CASES[-1]:
        assert n_pos == 143748 > R.BWD_MAX_BLOCKS * R.BWD_THREADS_TIER8 == 131072
    _, gyd, layers_d = _device(ref)
    pooled = torch.from_numpy(ref["pooled"]).cuda()
    d0, grads = _backward(pooled, gyd, case, layers_d)
    d0_b, grads_b = _backward(pooled, gyd, case, layers_d)
    none, grads_c = _backward(pooled, gyd, case, layers_d, want_d0=False)
    assert none is None and not torch.isnan(d0).any()
    assert _same_bits(d0, ref["d0"])
    assert torch.equal(d0.view(torch.int32), d0_b.view(torch.int32))
    for k, (gw, gb) in enumerate(grads):
        want = ref["grads"][k]
        for name, g, g_b, g_c, s, mag in (("weight", gw, grads_b[k][0], grads_c[k][0], want["w"], want["w_abs"]),
                                          ("bias", gb, grads_b[k][1], grads_c[k][1], want["b"], want["b_abs"])):
            if g is None:
                assert name == "bias" and ref["layers"][k][1] is None
                continue
            got = g.cpu().numpy().astype(np.float64).reshape(s.shape)
            assert np.isfinite(got).all()
            bound = 2.0 ** -24 * np.abs(s) + n_pos * 2.0 ** -53 * mag
            err = np.abs(got - s)
            print(f"layer {k} {name}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all(), (k, name)
            assert torch.equal(g.view(torch.int32), g_b.view(torch.int32))       # two runs, the same bits
            assert torch.equal(g.view(torch.int32), g_c.view(torch.int32))       # ... and with or without d_0


def test_finish_leaves_unwanted_gradients_alone():
    """A null gradient pointer is skipped, the others are written as before."""
    from arco_amd import _lib as L
    case = R.CASES[0]
    n, patch, pool, B, widths, _ = case
    x, layers, gy = R.case_input(case)
    layers_d = [(torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda()) for W, b in layers]
    pooled, _ = _forward(torch.from_numpy(x).cuda(), case, layers_d)
    _, full = _backward(pooled, torch.from_numpy(gy).cuda(), case, layers_d)
    geom = _geom(n, patch, pool, B, widths[0])
    ptrs, w4 = _chain(layers_d)
    ws = torch.empty(L.query("arco_patch_head_ws_bytes", *geom, 4, *w4) // 8, dtype=torch.float64, device="cuda")
    L.call("arco_patch_head_bwd", L.ptr(pooled), L.ptr(torch.from_numpy(gy).cuda()), *geom, 4, *ptrs, *w4, None, L.ptr(ws))
    gw2, gb3 = torch.full_like(full[1][0], NAN), torch.full_like(full[2][1], NAN)
    L.call("arco_patch_head_wgrad_finish", L.ptr(ws), *geom, 4, *w4, None, None, L.ptr(gw2), None, None, L.ptr(gb3), None, None)
    assert torch.equal(gw2, full[1][0]) and torch.equal(gb3, full[2][1])


def test_refusals():
    """Width 33, 5 layers (and 0), an axis shorter than the patch, a missing weight, a weight behind the last layer, null tensors: an error
    that names the entry point, before any launch - the outputs keep their fill."""
    from arco_amd import _lib as L
    B, C, n, patch, pool = 1, 2, (8, 8, 8), 4, 2
    geom = dict(nd=3, B=B, C=C, n0=8, n1=8, n2=8, patch=patch, pool=pool)
    w = torch.zeros(33 * 33, device="cuda")
    src = torch.zeros(27 * B * 33 * 8 + B * C * 512, device="cuda")
    fill = torch.full((27 * B * 33 * 8,), 7.0, device="cuda")
    out1, out2 = fill.clone(), fill.clone()
    ws = torch.full((512 * 4 * (32 * 32 + 32),), 7.0, dtype=torch.float64, device="cuda")
    ws0 = ws.clone()
    good = dict(layers=2, ptrs=[L.ptr(w), L.ptr(w), L.ptr(w), None, None, None, None, None], widths=[4, 2, 0, 0])
    bad = [dict(widths=[33, 2, 0, 0]), dict(widths=[4, 33, 0, 0]), dict(widths=[0, 2, 0, 0]), dict(layers=5), dict(layers=0),
           dict(ptrs=[L.ptr(w), None, None, None, None, None, None, None]),                       # the second layer's weight is missing
           dict(ptrs=[L.ptr(w), None, L.ptr(w), None, L.ptr(w), None, None, None]),               # a weight behind the last layer
           dict(geom=dict(geom, n1=3)), dict(geom=dict(geom, C=33)), dict(geom=dict(geom, nd=4))]

    def calls(a):
        g = list(a.get("geom", geom).values())
        lay, ptrs, widths = a.get("layers", good["layers"]), a.get("ptrs", good["ptrs"]), a.get("widths", good["widths"])
        return {"arco_patch_head_fwd": (L.ptr(src), *g, lay, *ptrs, *widths, L.ptr(out1), L.ptr(out2)),
                "arco_patch_head_bwd": (L.ptr(src), L.ptr(src), *g, lay, *ptrs, *widths, L.ptr(out1), L.ptr(ws))}
    for change in bad:
        for entry, args in calls(change).items():
            with pytest.raises(RuntimeError, match=entry):
                L.call(entry, *args)
        if "ptrs" not in change:
            a = dict(good, **change)
            assert L.query("arco_patch_head_ws_bytes", *a.get("geom", geom).values(), a["layers"], *a["widths"]) == -1
            with pytest.raises(RuntimeError, match="arco_patch_head_wgrad_finish"):
                L.call("arco_patch_head_wgrad_finish", L.ptr(ws), *a.get("geom", geom).values(), a["layers"], *a["widths"],
                       L.ptr(out1), None, None, None, None, None, None, None)
    g = list(geom.values())
    for args in ((None, *g, 2, *good["ptrs"], *good["widths"], L.ptr(out1), L.ptr(out2)),
                 (L.ptr(src), *g, 2, *good["ptrs"], *good["widths"], None, L.ptr(out2)),
                 (L.ptr(src), *g, 2, *good["ptrs"], *good["widths"], L.ptr(out1), None)):
        with pytest.raises(RuntimeError, match="arco_patch_head_fwd"):
            L.call("arco_patch_head_fwd", *args)
    with pytest.raises(RuntimeError, match="arco_patch_head_bwd"):
        L.call("arco_patch_head_bwd", L.ptr(src), L.ptr(src), *g, 2, *good["ptrs"], *good["widths"], L.ptr(out1), None)
    with pytest.raises(RuntimeError, match="arco_patch_head_wgrad_finish"):        # a gradient pointer of an absent layer
        L.call("arco_patch_head_wgrad_finish", L.ptr(ws), *g, 2, *good["widths"], None, None, None, None, L.ptr(out1), None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(out1, fill) and torch.equal(out2, fill) and torch.equal(ws, ws0)
    L.call("arco_patch_head_fwd", *calls({})["arco_patch_head_fwd"])               # the good call goes through and writes
    torch.cuda.synchronize()
    assert not torch.equal(out1, fill) and not torch.equal(out2, fill)
