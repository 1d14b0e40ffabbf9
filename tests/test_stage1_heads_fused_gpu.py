"""tests/test_stage1_heads_gpu.py restated for the fused route (stage1.patch_heads(route="fused"), ISD / ISD_3d patch_heads="fused",
pretrain_2D / pretrain_3D --patch_heads fused): the heads alone against float64, the two golden iterations of tests/test_pretrain_gpu.py
at its tolerances, one step at a geometry whose pooling windows overlap, the trainers end to end (-m gpu).  The steppers, module builders
and golden files are that file's."""
import copy
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import fixture_inputs as fx               # noqa: E402
import test_stage1_heads_gpu as H         # noqa: E402

pytestmark = pytest.mark.gpu


def _run(route, x, patch, head, predictor, w, x_grad):
    """(output stacked, {name: gradient}) of sum(w * patch_heads(...)) on fresh leaves."""
    from arco_amd.stage1 import patch_heads
    x = x.detach().clone().requires_grad_(x_grad)
    mods = [head] + ([predictor] if predictor is not None else [])
    for m in mods:
        m.zero_grad(set_to_none=True)
    out = patch_heads(x, patch, head, predictor, route)
    assert torch.is_tensor(out) == (route == "fused")
    out = out if torch.is_tensor(out) else torch.cat(out)
    (out * w.to(out.dtype)).sum().backward()
    grads = {f"{i}.{k}": p.grad.detach().clone() for i, m in enumerate(mods) for k, p in m.named_parameters()}
    if x_grad:
        grads["x"] = x.grad.detach().clone()
    return out.detach(), grads


@pytest.mark.parametrize("side", ["student", "teacher"])
@pytest.mark.parametrize("nd", [2, 3])
def test_patch_heads_fused_route_against_float64(nd, side):
    """Both fp32 routes against the torch route on float64 copies of the same modules.  The fused route's largest error may be at most
    max(2 x the fp32 torch route's own, 2^-20 x the largest magnitude of the float64 tensor), the project's bound for a second fp32
    evaluation of the same chain.  Output and every gradient; the ratios are printed."""
    n, C = ((64, 64), 4) if nd == 2 else ((32, 32, 32), 2)
    patch, pool, B = 10, 4, 2
    head, predictor = H._heads(nd, C, pool, seed=5 + nd)
    predictor = predictor if side == "student" else None
    rs = np.random.RandomState(70 + nd)
    x = torch.from_numpy(rs.standard_normal((B, C) + n).astype(np.float32)).cuda()
    P = int(np.prod([(s - patch) // (patch // 2) + 1 for s in n]))
    assert P == (121 if nd == 2 else 125)
    w = torch.from_numpy(rs.standard_normal((P * B, C) + (pool,) * nd).astype(np.float32)).cuda()
    x_grad = side == "student"                    # the teacher's map comes out of no_grad
    head64 = copy.deepcopy(head).double()
    pred64 = copy.deepcopy(predictor).double() if predictor is not None else None
    ref, ref_g = _run("torch", x.double(), patch, head64, pred64, w.double(), x_grad)
    tor, tor_g = _run("torch", x, patch, head, predictor, w, x_grad)
    fus, fus_g = _run("fused", x, patch, head, predictor, w, x_grad)
    assert fus.shape == ref.shape == w.shape and fus.dtype == torch.float32
    assert set(fus_g) == set(ref_g) and len(fus_g) == (4 if side == "teacher" else 9)
    for name, r, t, g in [("output", ref, tor, fus)] + [(k, ref_g[k], tor_g[k], fus_g[k]) for k in sorted(ref_g)]:
        assert g.shape == r.shape, name
        e_t, e_g = float((t.double() - r).abs().max()), float((g.double() - r).abs().max())
        floor = 2.0 ** -20 * float(r.abs().max())
        print(f"nd={nd} {side} {name}: fused error {e_g:.3e}, torch error {e_t:.3e}, ratio {e_g / max(e_t, 1e-300):.2f}, floor {floor:.3e}")
        assert e_g <= max(2 * e_t, floor), (name, e_g, e_t, floor)


def test_teacher_side_skips_the_input_gradient():
    """A map that needs no gradient: the backward neither allocates d_0 nor runs the pooling's backward kernel, and the parameter
    gradients are those of the run that does (the same bits)."""
    from arco_amd.stage1 import patch_heads
    head, _ = H._heads(3, 2, 4, seed=9)
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.standard_normal((1, 2, 20, 20, 20)).astype(np.float32)).cuda()
    res = []
    for x_grad in (False, True):
        head.zero_grad(set_to_none=True)
        leaf = x.clone().requires_grad_(x_grad)
        out = patch_heads(leaf, 10, head, None, "fused")
        assert out.shape == (27, 2, 4, 4, 4)
        out.square().sum().backward()
        assert (leaf.grad is not None) == x_grad
        res.append([p.grad.clone() for p in head.parameters()])
    assert len(res[0]) == 4 and all(torch.equal(a, b) for a, b in zip(*res))
    with torch.no_grad():
        assert not patch_heads(x, 10, head, None, "fused").requires_grad


@pytest.mark.parametrize("nd", [2, 3])
def test_stage1_two_iterations_vs_reference_golden_fused_route(nd):
    """tests/test_pretrain_gpu.py::test_stage1_two_iterations_vs_reference_golden with patch_heads="fused": the same golden files, the
    same tolerances."""
    cfg = fx.STAGE1_CFG if nd == 2 else fx.STAGE1_CFG_3D
    G = H.GOLD[nd]
    st = H._stepper(cfg, nd, "fused")
    sd0 = {k: v.clone() for k, v in st.model.state_dict().items()}
    bn1 = "encoder.in_conv.conv_conv.1" if nd == 2 else "block_one.conv.1"
    for it in range(cfg["steps"]):
        im_q, im_k, lab = (fx.stage1_batch if nd == 2 else fx.stage1_batch_3d)(40, it)
        torch.manual_seed(100 + it)
        if it == 0:
            st.model.zero_grad()
        st.step(im_q.cuda(), lab.cuda(), im_k.cuda())
        t = st.last_terms
        got = [float(t[k]) for k in ("loss", "ce", "dice", "latent", "output")]
        np.testing.assert_allclose(got, G[f"s{it}_terms"], rtol=1e-3, err_msg=f"iteration {it}")
    sd = st.model.state_dict()
    assert int(sd["queue_ptr"]) == int(G["final::queue_ptr"][0]) and int(sd["mask_queue_ptr"]) == int(G["final::mask_queue_ptr"][0])
    np.testing.assert_allclose(sd["queue"].cpu().numpy(), G["final::queue"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(sd["queue_mask"].cpu().numpy(), G["final::queue_mask"], rtol=1e-3, atol=1e-4)
    assert int(sd[f"ema_model.{bn1}.num_batches_tracked"]) == int(G[f"final::ema_model.{bn1}.num_batches_tracked"]) == 4
    for pre in ("model", "ema_model"):
        for n, ref_abs in zip((str(x) for x in G[f"final_{pre}.names"]), G[f"final_{pre}.abs"]):
            v = sd[n].float()
            np.testing.assert_allclose(float(v.double().abs().sum()), ref_abs, rtol=1e-3, atol=1e-5, err_msg=n)
    changed = 0
    for k in G.files:
        if not k.startswith("final::") or k.split("::")[1].startswith(("queue", "mask_queue")):
            continue
        name = k.split("::")[1]
        v = sd[name].detach().cpu()
        if v.dtype == torch.long:
            continue
        changed += int(not torch.equal(v, sd0[name].cpu()))
        v = v if v.numel() <= 20000 else v[::4, ::4]
        err = float(np.abs(v.numpy() - G[k]).max()) / max(1e-6, float(np.abs(G[k]).max()))
        assert err < 2e-3, (name, err)
    assert changed >= 20


def test_one_step_at_overlapping_windows_3d_fused():
    """32^3, 10-voxel head patches pooled to 4 (125 patches, overlapping windows: the torch route takes its patch-by-patch fallback): two
    steppers with equal seeds, one per route, at the stage-1 tests' tolerances."""
    cfg = H.CFG_3D_OVERLAP
    res = {}
    for route in ("torch", "fused"):
        st = H._stepper(cfg, 3, route)
        assert st.model.queue_mask.shape[1] == 125
        im_q, im_k, lab = fx.stage1_batch_3d(40, 0, cfg)
        torch.manual_seed(100)
        st.model.zero_grad()
        st.step(im_q.cuda(), lab.cuda(), im_k.cuda())
        sd = st.model.state_dict()
        res[route] = dict(terms=[float(st.last_terms[k]) for k in ("loss", "ce", "dice", "latent", "output")],
                          queue=sd["queue"].cpu().numpy().copy(), queue_mask=sd["queue_mask"].cpu().numpy().copy(),
                          grads={n: p.grad.detach().cpu().numpy().copy() for n, p in st.model.named_parameters() if p.grad is not None})
    a, b = res["torch"], res["fused"]
    assert all(np.isfinite(b["terms"]))
    np.testing.assert_allclose(b["terms"], a["terms"], rtol=1e-3)
    np.testing.assert_allclose(b["queue"], a["queue"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(b["queue_mask"], a["queue_mask"], rtol=1e-3, atol=1e-4)
    assert set(a["grads"]) == set(b["grads"]) and len(a["grads"]) > 20
    assert any(n.startswith("k_outputs_head") for n in a["grads"]) and any(n.startswith("outputs_predictor") for n in a["grads"])
    for n, g in a["grads"].items():
        assert float(np.abs(b["grads"][n] - g).max()) <= 5e-3 * float(np.abs(g).max()), n


def test_pretrain3d_trainer_runs_fused_route(tmp_path):
    """pretrain_3D --synthetic 1 --patch_heads fused, 2 iterations at 32^3 with 10-voxel head patches pooled to 4; the checkpoints load
    into the stage-2 V-Net."""
    from arco_amd import pretrain_3D as P3
    from arco_amd.model_3D import create_model_3d
    import arco_amd.model_3D as M3
    snap = str(tmp_path)
    args = P3.build_parser().parse_args(["--synthetic", "1", "--max_iterations", "2", "--save_every", "2", "--K", "4", "--patch_heads", "fused",
                                         "--output_pooling_size", "4", "--latent_feature_size", "16", "--snapshot_path", snap])
    args.patch_size, args.head_patch = [32, 32, 32], 10
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    real = H._with_patch_count(M3.ISD_3d, 125, args.num_classes * 64, -1)
    try:
        assert P3.train(args, snap) == "Training Finished!"
    finally:
        M3.ISD_3d.__init__ = real
    for tag in ("", "_ema"):
        sd = torch.load(os.path.join(snap, f"iter_2{tag}.pth"), map_location="cpu")
        create_model_3d(num_classes=2).load_state_dict(sd, strict=True)
        assert all(torch.isfinite(v.float()).all() for v in sd.values())


def test_pretrain2d_trainer_runs_fused_route(tmp_path):
    """pretrain_2D --synthetic 1 --patch_heads fused, 2 iterations at 64 x 64 with cut size 10 pooled to 4 (121 patches)."""
    from arco_amd import pretrain_2D as P
    from arco_amd.model_2D import create_model
    import arco_amd.model_2D as M2
    snap = str(tmp_path)
    argv = ["--synthetic", "1", "--max_iterations", "2", "--save_every", "2", "--batch_size", "4", "--labeled_bs", "2", "--K", "12",
            "--cut_size", "10", "--output_pooling_size", "4", "--latent_feature_size", "32", "--snapshot_path", snap, "--patch_heads", "fused"]
    args = P.build_parser().parse_args(argv)
    args.patch_size = [64, 64]
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    real = H._with_patch_count(M2.ISD, 121, args.num_classes * 16, 0)
    try:
        assert P.train(args, snap) == "Training Finished!"
    finally:
        M2.ISD.__init__ = real
    for tag in ("", "_ema"):
        sd = torch.load(os.path.join(snap, f"iter_2{tag}.pth"), map_location="cpu")
        create_model(num_classes=4).load_state_dict(sd, strict=True)
        assert all(torch.isfinite(v.float()).all() for v in sd.values())
