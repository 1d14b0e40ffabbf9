"""The KL-divergence-to-queue terms of stage 1 on the fused route (stage1.queue_kld(route="fused"), ISD / ISD_3d kld="fused", pretrain_2D /
pretrain_3D --kld fused) with the steppers, goldens and helpers of tests/test_stage1_heads_gpu.py: the two golden iterations at that file's
tolerances, one step against the torch route at a geometry with overlapping pooling windows, the trainers end to end, the drop-in 6-tuple
(-m gpu)."""
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


def _count_routes(monkeypatch):
    """Every stage1.queue_kld call's route, in order."""
    from arco_amd import stage1
    real, seen = stage1.queue_kld, []

    def counted(zs, zt, q, Ts, Tt, route="torch"):
        seen.append(route)
        return real(zs, zt, q, Ts, Tt, route)
    monkeypatch.setattr(stage1, "queue_kld", counted)
    return seen


@pytest.mark.parametrize("nd", [2, 3])
def test_stage1_two_iterations_vs_reference_golden_fused_kld(nd, monkeypatch):
    """tests/test_stage1_heads_gpu.py::test_stage1_two_iterations_vs_reference_golden_gpu_route, its body and tolerances, on a stepper whose
    model has kld="fused" (patch heads on the torch route): both terms of both iterations come from the two kernels."""
    real, made = H._stepper, []

    def fused_kld_stepper(cfg, nd_, route):
        st = real(cfg, nd_, "torch")
        st.model.kld = "fused"
        made.append(st)
        return st
    monkeypatch.setattr(H, "_stepper", fused_kld_stepper)
    seen = _count_routes(monkeypatch)
    H.test_stage1_two_iterations_vs_reference_golden_gpu_route(nd)
    assert len(made) == 1 and made[0].model.kld == "fused" and seen == ["fused"] * 4


def test_one_step_torch_against_fused_kld_3d(monkeypatch):
    """CFG_3D_OVERLAP (32^3, 125 patches): two steppers with equal seeds, one per kld route.  Terms at rtol 1e-3, every parameter gradient
    within 5e-3 of its largest element - the key heads' among them: the teacher side's gradient is live."""
    cfg = H.CFG_3D_OVERLAP
    seen = _count_routes(monkeypatch)
    res = {}
    for route in ("torch", "fused"):
        st = H._stepper(cfg, 3, "torch")
        st.model.kld = route
        im_q, im_k, lab = fx.stage1_batch_3d(40, 0, cfg)
        torch.manual_seed(100)
        st.model.zero_grad()
        st.step(im_q.cuda(), lab.cuda(), im_k.cuda())
        sd = st.model.state_dict()
        res[route] = dict(terms=[float(st.last_terms[k]) for k in ("loss", "ce", "dice", "latent", "output")],
                          queue=sd["queue"].cpu().numpy().copy(), queue_mask=sd["queue_mask"].cpu().numpy().copy(),
                          ptrs=(int(sd["queue_ptr"]), int(sd["mask_queue_ptr"])),
                          grads={n: p.grad.detach().cpu().numpy().copy() for n, p in st.model.named_parameters() if p.grad is not None})
    assert seen == ["fused"] * 2          # the torch route goes through the model's 6-tuple, as before
    a, b = res["torch"], res["fused"]
    assert all(np.isfinite(b["terms"])) and b["terms"][3] > 0 and b["terms"][4] > 0
    np.testing.assert_allclose(b["terms"], a["terms"], rtol=1e-3)
    assert a["ptrs"] == b["ptrs"] and np.array_equal(a["queue"], b["queue"]) and np.array_equal(a["queue_mask"], b["queue_mask"])      # the enqueue is the same code
    assert set(a["grads"]) == set(b["grads"]) and len(a["grads"]) > 20
    for head in ("k_outputs_head", "k_latent_head", "outputs_predictor", "latent_predictor"):
        assert any(n.startswith(head) and np.abs(g).max() > 0 for n, g in a["grads"].items()), head
    for n, g in a["grads"].items():
        assert float(np.abs(b["grads"][n] - g).max()) <= 5e-3 * float(np.abs(g).max()), n


@pytest.mark.parametrize("nd", [2, 3])
def test_the_six_tuple_is_the_torch_routes_on_fused_kld(nd):
    """ISD.forward / ISD_3d.forward for drop-in users: true logits whatever kld says, bit for bit the torch route's."""
    cfg = fx.STAGE1_CFG if nd == 2 else fx.STAGE1_CFG_3D
    outs = {}
    for route in ("torch", "fused"):
        st = H._stepper(cfg, nd, "torch")
        st.model.kld = route
        im_q, im_k, _ = (fx.stage1_batch if nd == 2 else fx.stage1_batch_3d)(40, 0)
        torch.manual_seed(100)
        with torch.no_grad():
            outs[route] = st.model(im_q.cuda(), im_k.cuda())
        outs[route] += (st.model.queue.clone(), st.model.queue_mask.clone())
    assert len(outs["torch"]) == 8 and outs["torch"][5].dim() == 2
    assert all(torch.equal(a, b) for a, b in zip(outs["torch"], outs["fused"]))


def _z(seed, n, L, dim=8):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda() for s in ((n, dim), (n, dim), (L, dim))]


@pytest.mark.parametrize("shape", [(6, 36), (5, 1027)])
@pytest.mark.parametrize("teacher_grad", [True, False])
def test_queue_kld_fused_against_float64(shape, teacher_grad):
    """stage1.queue_kld from the embeddings: loss and the gradients of both row sets against the torch route in float64, the fused error at
    most max(2 x the fp32 torch route's own, 2^-20 x the largest magnitude of the float64 tensor).  A detached teacher gets no gradient."""
    from arco_amd.stage1 import queue_kld
    zs, zt, q = _z(3, *shape)
    res = {}
    for name, route, dt in (("ref", "torch", torch.float64), ("torch", "torch", torch.float32), ("fused", "fused", torch.float32)):
        a, b = zs.to(dt).clone().requires_grad_(True), zt.to(dt).clone().requires_grad_(teacher_grad)          # fresh leaves: .to() of the same dtype is no copy
        out = queue_kld(a, b, q.to(dt), 0.1, 0.07, route)
        (out * 0.5).backward()
        assert (b.grad is not None) == teacher_grad
        res[name] = [out.detach().reshape(1).double(), a.grad.double()] + ([b.grad.double()] if teacher_grad else [])
    for what, r, t, g in zip(("loss", "d student", "d teacher"), res["ref"], res["torch"], res["fused"]):
        e_t, e_g, floor = float((t - r).abs().max()), float((g - r).abs().max()), 2.0 ** -20 * float(r.abs().max())
        print(f"{shape} {what}: fused error {e_g:.3e}, torch error {e_t:.3e}, ratio {e_g / max(e_t, 1e-300):.2f}, floor {floor:.3e}")
        assert e_g <= max(2 * e_t, floor), (what, e_g, e_t, floor)


def test_a_second_backward_through_the_fused_node_raises():
    from arco_amd.stage1 import queue_kld
    zs, zt, q = _z(4, 6, 36)
    zs.requires_grad_(True)
    out = queue_kld(zs, zt, q, 0.1, 0.1, "fused")
    out.backward(retain_graph=True)
    first = zs.grad.clone()
    assert torch.isfinite(first).all() and first.abs().max() > 0
    with pytest.raises(RuntimeError, match="second"):
        out.backward(retain_graph=True)
    assert torch.equal(zs.grad, first)


def test_pretrain3d_trainer_runs_fused_kld(tmp_path):
    """pretrain_3D --synthetic 1 --kld fused --patch_heads fused, 2 iterations at 32^3 with 10-voxel head patches pooled to 4; the
    checkpoints load into the stage-2 V-Net."""
    from arco_amd import pretrain_3D as P3
    from arco_amd.model_3D import create_model_3d
    import arco_amd.model_3D as M3
    snap = str(tmp_path)
    args = P3.build_parser().parse_args(["--synthetic", "1", "--max_iterations", "2", "--save_every", "2", "--K", "4", "--patch_heads", "fused",
                                         "--kld", "fused", "--output_pooling_size", "4", "--latent_feature_size", "16", "--snapshot_path", snap])
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


def test_pretrain2d_trainer_runs_fused_kld(tmp_path):
    """pretrain_2D --synthetic 1 --kld fused --patch_heads fused, 2 iterations at 64 x 64 with cut size 10 pooled to 4 (121 patches)."""
    from arco_amd import pretrain_2D as P
    from arco_amd.model_2D import create_model
    import arco_amd.model_2D as M2
    snap = str(tmp_path)
    argv = ["--synthetic", "1", "--max_iterations", "2", "--save_every", "2", "--batch_size", "4", "--labeled_bs", "2", "--K", "12",
            "--cut_size", "10", "--output_pooling_size", "4", "--latent_feature_size", "32", "--snapshot_path", snap, "--patch_heads", "fused",
            "--kld", "fused"]
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
