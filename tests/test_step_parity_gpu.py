"""Whole training step on the HIP path vs the CPU oracle step (oracle/cpu_step.py): same weights, same CPU-generator
seed, dropout off, two chained steps.  Checks every loss term, the banks and the updated student/teacher weights (-m gpu)."""
import random

import numpy as np
import pytest
import torch

import cpu_step
import fixture_inputs as fx

pytestmark = pytest.mark.gpu


def _generators():
    """the three host generators' states (python, numpy, torch CPU) as one comparable value"""
    ns = np.random.get_state()
    return (random.getstate(), ns[0], ns[1].tobytes(), ns[2:], torch.get_rng_state().numpy().tobytes())


def _drop_off(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0


@pytest.mark.parametrize("variant", [dict(dense_head=1, k2=0.0, apply_aug="none"),
                                     dict(dense_head=0, head_levels=2, dense_teacher=0, k2=0.0, apply_aug="cutmix"),
                                     dict(dense_head=0, head_levels=2, dense_teacher=0, k2=1.0, apply_aug="cutmix"),
                                     dict(dense_head=0, head_levels=2, dense_teacher=0, k2=1.0, apply_aug="cutout"),
                                     dict(dense_head=0, head_levels=2, dense_teacher=0, k2=0.0, apply_aug="classmix"),
                                     dict(revisit=1, K=4, topk=2, k2=0.0, apply_aug="cutmix"),
                                     dict(dense_head=0, head_levels=2, dense_teacher=0, k2=1.0, apply_aug="cutmix", batch_transform=1),
                                     dict(dense_head=0, head_levels=3, dense_teacher=0, k2=1.0, apply_aug="cutmix"),
                                     # the loss's degenerate-batch path (loss_helper_3d.py:417-424: <= 1 valid class -> `0.0 * rep.sum()`):
                                     # every head parameter gets a ZERO gradient, and SGD still applies weight decay / momentum to it
                                     dict(dense_head=0, head_levels=3, dense_teacher=0, k2=0.0, apply_aug="none", zero_path=1),
                                     dict(dense_head=1, k2=0.0, apply_aug="none", zero_path=1),
                                     # the SHIPPED schedule against the oracle directly (every variant above runs
                                     # --graphs 0 and reaches the default only through graph == eager and two-stream == single-stream):
                                     # trainer-default graph capture + replay and the two-stream pass schedule; three warm-up steps on
                                     # other data make every graph exist, the state is rolled back, the two compared steps REPLAY
                                     dict(dense_head=0, head_levels=3, dense_teacher=0, k2=1.0, apply_aug="cutmix", graphs=1, warm=1),
                                     dict(dense_head=0, head_levels=3, dense_teacher=0, k2=1.0, apply_aug="cutout", graphs=1, warm=1,
                                          batch_transform=1)])
def test_two_steps_vs_cpu_oracle(variant):
    from arco_amd import train_arco_2d as T
    b, patch, C, Q, Nn, qs = 2, (64, 64), 4, 64, 32, 300
    unet_sd, fe_sd = fx.unet_state(21, 1, C), fx.fe_state(31)
    variant = dict(variant)
    zero_path = bool(variant.pop("zero_path", 0))
    warm = bool(variant.pop("warm", 0))
    if zero_path:       # both nets predict class 0 everywhere and the labels are all background: one valid class
        unet_sd["decoder.out_conv.weight"] = unet_sd["decoder.out_conv.weight"] * 0.0
        unet_sd["decoder.out_conv.bias"] = torch.tensor([6.0, 0.0, 0.0, 0.0])
    qrep_w = [fx.fe_state(32)["fea4.weight"], fx.fe_state(33)["fea4.weight"]]
    argv = ["--batch_size", str(b), "--queue_size", str(qs), "--synthetic", "1", "--num_queries", str(Q),
            "--num_negatives", str(Nn), "--k1", "1.0", "--base_lr", "0.01", "--graphs", "0"]
    variant = dict(variant)
    bt = variant.setdefault("batch_transform", 0)        # the reference's batch_transform: its own variant (AdvMorph's velocity
    for k, v in variant.items():                         # field comes from the device generator: both sides get the same one)
        argv += [f"--{k}", str(v)]
    from arco_amd.adv_morph import AdvMorph
    vel = lambda B, h, w: torch.from_numpy(np.random.RandomState(17).uniform(-1, 1, size=(B, 2, h, w)).astype(np.float32))
    real_velocity = AdvMorph.init_velocity
    if bt:
        AdvMorph.init_velocity = lambda self, batch_size, height, width, use_zero=False: self.unit_normalize(vel(batch_size, height, width).cuda())
    args = T.build_parser().parse_args(argv)
    args.patch_size = list(patch)
    st_g = T.ArcoStep2D(args, "cuda:0")
    st_g.model.load_state_dict(unet_sd, strict=True)
    st_g.ema_model.load_state_dict(unet_sd, strict=True)
    st_g.q_feature_extractor.load_state_dict(fe_sd, strict=True)
    st_g.k_feature_extractor.load_state_dict(fe_sd, strict=True)
    with torch.no_grad():
        st_g.q_representation[0].weight.copy_(qrep_w[0])
        st_g.q_representation[1].weight.copy_(qrep_w[1])
    for m in (st_g.model, st_g.ema_model):
        _drop_off(m)
    if warm:
        import test_configs_at_size_gpu as TC
        assert args.graphs == 1 and T.TEACHER_SIDE >= 3
        snap = TC._snapshot(st_g)
        heads0 = [p.detach().clone() for m in (st_g.q_feature_extractor, st_g.q_representation) for p in m.parameters()]
        wr = np.random.RandomState(99)
        for w in range(3):
            random.seed(50 + w); np.random.seed(50 + w); torch.manual_seed(50 + w)
            st_g.step(torch.from_numpy(wr.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda(),
                      torch.from_numpy(fx.blob_labels(wr, b, patch, C)).cuda(),
                      torch.from_numpy(wr.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda())
        torch.cuda.synchronize()
        assert st_g.s_train_lu.captured == bool(st_g.args.graph_train) and len(st_g.t_fwd_lu.graphs) > 0      # the compared steps replay
        TC._restore(st_g, snap)
        with torch.no_grad():                           # (the rollback is complete: the heads are back at their seed values)
            for p0, p in zip(heads0, [p for m in (st_g.q_feature_extractor, st_g.q_representation) for p in m.parameters()]):
                assert torch.equal(p0, p)
        if st_g.random_pool is not None:
            raise AssertionError("warm variants do not roll the revisiting pool back")
    st_o = cpu_step.make_state(unet_sd, fe_sd, qrep_w)
    bank_o, ptr_o, qsz = fx.fresh_bank(C, 496, qs, 'zeros')
    pool_o = None
    if variant.get("revisit"):              # the oracle starts from the trainer's pool (reference flattening order)
        assert st_g.random_pool is not None and args.dense_head == 1 and args.dense_teacher == 1
        rows0 = st_g.random_pool.channels_first().cpu().clone()
        np.testing.assert_allclose(rows0.norm(dim=1).numpy(), 1.0, rtol=1e-5)
        pool_o = dict(rows=rows0, ptr=torch.zeros(1, dtype=torch.long))
    rs = np.random.RandomState(3)
    all_same = True
    for it in range(2):
        l = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32))
        u = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32))
        lab = torch.from_numpy(fx.blob_labels(rs, b, patch, C))
        if zero_path:
            lab = torch.zeros_like(lab)
        random.seed(10 + it); np.random.seed(10 + it); torch.manual_seed(10 + it)
        cpu_step.step(st_o, l, lab, u, bank_o, ptr_o, qsz, C, k1=1.0, lr=0.01, nq=Q, nn_=Nn, k2=variant["k2"],
                      apply_aug=variant["apply_aug"], pool=pool_o, topk=variant.get("topk", 5), bt=bool(bt), morph_velocity=vel)
        gen_o = _generators()
        random.seed(10 + it); np.random.seed(10 + it); torch.manual_seed(10 + it)
        st_g.step(l.cuda(), lab.cuda(), u.cuda())
        to, tg = st_o["last_terms"], st_g.last_terms
        # Did both sides consume the host generators identically, i.e. make the same data-dependent decisions?  Always, except
        # behind batch_transform from the second step on: its 8-bit round trips quantise the teacher's confidences to k/255 and the
        # morphed images agree to ~1e-4 only, so a value within rounding of a quantisation / threshold boundary may land on either
        # side; a key more or less moves every later draw of the CPU generator - incl. the TPS warp of the equivariance term
        # (seen when round 5 made the bilinear source weights bit-equal to torch's: step 1 of this variant drew another warp,
        # eqv 3.8e-3 off, all earlier module outputs of the step within 1e-5: tools/debug/parity_trace.py)
        same_draws = gen_o == _generators()
        assert same_draws or (bt and it > 0)
        all_same = all_same and same_draws
        if pool_o is not None:
            np.testing.assert_allclose(float(tg["loss_q"]), to["loss_q"], rtol=1e-3, err_msg=f"step {it} loss_q")
            np.testing.assert_allclose(st_g.random_pool.channels_first().cpu().numpy(), pool_o["rows"].numpy(), rtol=2e-3, atol=2e-6)
            assert int(st_g.random_pool.ptr) == int(pool_o["ptr"]) == (b * (it + 1)) % 4
        for k in ("ce", "dice", "unsup", "reco") + (("eqv",) if variant["k2"] else ()):
            np.testing.assert_allclose(float(tg[k]), to[k], rtol=1e-3 if (same_draws or k != "eqv") else 0.25, atol=1e-5,
                                       err_msg=f"step {it} {k}")      # north_star: loss within 1e-3 (eqv under ANOTHER warp: same batch, loosely)
        for bo, bg in zip(bank_o, st_g.memobank):
            if bt and bo[0].shape != bg[0].shape:
                # AdvMorph'ed images agree to ~1e-4 (fp32 association of eight grid compositions): a pixel sitting on a
                # threshold may flip, i.e. one key more or less
                assert abs(int(bo[0].shape[0]) - int(bg[0].shape[0])) <= 2
                continue
            assert bo[0].shape == bg[0].shape
            np.testing.assert_allclose(bg[0].cpu().numpy(), bo[0].numpy(), rtol=1e-3, atol=2e-4)      # rows of magnitude ~2: 1e-4 of the row
        if not bt:
            assert [int(p) for p in ptr_o] == [int(p) for p in st_g.queue_ptrlis]
    AdvMorph.init_velocity = real_velocity
    if zero_path:
        assert to["reco"] == 0.0 and float(tg["reco"]) == 0.0
        # the heads moved by weight decay + momentum alone - and they did move (a skipped parameter would sit at its seed value)
        for k, v in st_o["q_fe"].items():
            got = st_g.q_feature_extractor.state_dict()[k].cpu()
            assert float((got - fe_sd[k]).abs().max()) > 0
            np.testing.assert_allclose(got.numpy(), v.detach().numpy(), rtol=1e-6, atol=1e-9)
        for i in range(2):
            np.testing.assert_allclose(st_g.q_representation[i].weight.detach().cpu().numpy(), st_o["q_rep"][i].detach().numpy(),
                                       rtol=1e-6, atol=1e-9)
    # updated weights: student U-Net (by name), heads, teacher
    sd_g = st_g.model.state_dict()
    worst, worst_key = 0.0, None
    for k, v in st_o["student"].items():
        if not v.requires_grad:
            continue
        ref = v.detach()
        err = float((sd_g[k].cpu() - ref).abs().max()) / max(1e-6, float(ref.abs().max()))
        if err > worst:
            worst, worst_key = err, k
    # (behind batch_transform the two sides' INPUT images agree to ~1e-4 only - fp32 association of AdvMorph's eight grid compositions -
    #  and the deepest BatchNorm sees 2 x 4 x 4 values per channel at this patch size: 1.1e-3 measured on one gamma, 2e-3 allowed;
    #  a step that drew another warp optimised another equivariance term)
    wtol = (2e-3 if bt else 1e-3) if all_same else 3e-2
    assert worst < wtol, (worst, worst_key)
    for k, v in st_o["q_fe"].items():
        ref = v.detach()
        got = st_g.q_feature_extractor.state_dict()[k].cpu()
        assert float((got - ref).abs().max()) / float(ref.abs().max()) < wtol, k
    for i in range(2):
        ref = st_o["q_rep"][i].detach()
        got = st_g.q_representation[i].weight.detach().cpu()
        assert float((got - ref).abs().max()) / float(ref.abs().max()) < wtol
    sd_t = st_g.ema_model.state_dict()
    for k, v in st_o["teacher"].items():
        if v.is_floating_point() and "running" not in k:
            assert float((sd_t[k].cpu() - v).abs().max()) / max(1e-6, float(v.abs().max())) < wtol, k
    # BatchNorm running statistics: the momentum updates of the train-mode forwards must land in the reference's order
    # (student: l, cj2_l, u [, tps]; teacher: u, l, u_aug) although the trainer runs the forwards in another order
    for name, sd_ref, sd_got in (("student", st_o["student"], sd_g), ("teacher", st_o["teacher"], sd_t)):
        for k, v in sd_ref.items():
            if "running" in k:
                np.testing.assert_allclose(sd_got[k].cpu().numpy(), v.numpy(), rtol=3e-4 if all_same else 5e-2, atol=(1e-4 if all_same else 2e-2) * float(v.abs().max()),
                                           err_msg=f"{name} {k}")


def test_cityscapes_shaped_step_runs():
    """BASELINE config 4 shape at reduced size: RGB input, 19 classes, non-square image; 3 steps, finite, banks fill."""
    from arco_amd import train_arco_2d as T
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    args = T.build_parser().parse_args(["--batch_size", "2", "--queue_size", "128", "--synthetic", "1", "--num_classes", "19",
                                        "--in_chns", "3", "--num_queries", "32", "--num_negatives", "16", "--k1", "1.0"])
    args.patch_size = [32, 64]
    st = T.ArcoStep2D(args, "cuda:0")
    for i in range(3):
        l_img, l_lab = T.synthetic_batch(2, args.patch_size, 19, 5 + i, "cuda:0", in_chns=3)
        u_img, _ = T.synthetic_batch(2, args.patch_size, 19, 50 + i, "cuda:0", in_chns=3)
        loss, reco = st.step(l_img, l_lab, u_img)
        assert torch.isfinite(loss).item()
    assert len(st.memobank) == 19 and all(b[0].shape[1] == 496 for b in st.memobank)


def _trainer(graphs, seed_state, extra=()):
    from arco_amd import train_arco_2d as T
    b, patch, C = 2, (64, 64), 4
    unet_sd, fe_sd, qrep_w = seed_state
    argv = ["--batch_size", str(b), "--queue_size", "300", "--synthetic", "1", "--num_queries", "64",
            "--num_negatives", "32", "--k1", "1.0", "--base_lr", "0.01", "--graphs", str(graphs), "--graph_train", str(graphs), *extra]
    args = T.build_parser().parse_args(argv)
    args.patch_size = list(patch)
    st = T.ArcoStep2D(args, "cuda:0")
    st.model.load_state_dict(unet_sd, strict=True)
    st.ema_model.load_state_dict(unet_sd, strict=True)
    st.q_feature_extractor.load_state_dict(fe_sd, strict=True)
    st.k_feature_extractor.load_state_dict(fe_sd, strict=True)
    with torch.no_grad():
        st.q_representation[0].weight.copy_(qrep_w[0])
        st.q_representation[1].weight.copy_(qrep_w[1])
    for m in (st.model, st.ema_model):
        _drop_off(m)
    from arco_amd import ops
    ops.bump_weight_epoch()
    return st


def _sync_state(dst, src):
    """dst <- src: weights, momentum, BN buffers, teacher, banks (so that ONE step is compared from equal state;
    whole trajectories diverge chaotically from 1-ulp differences of the atomics-based scatters)."""
    from arco_amd import ops
    with torch.no_grad():
        dst.optimizer.flat_p.copy_(src.optimizer.flat_p)
        dst.optimizer.flat_buf.copy_(src.optimizer.flat_buf)
        dst.optimizer._started = list(src.optimizer._started)
        for g_d, g_s in zip(dst.optimizer.param_groups, src.optimizer.param_groups):
            g_d['lr'] = g_s['lr']
        for md, ms in ((dst.model, src.model), (dst.ema_model, src.ema_model),
                       (dst.k_feature_extractor, src.k_feature_extractor)):
            for (kd, vd), (ks, vs) in zip(md.state_dict().items(), ms.state_dict().items()):
                assert kd == ks
                vd.copy_(vs)
        for c in range(len(src.memobank)):
            dst.memobank[c] = [t.clone() for t in src.memobank[c]]
            dst.queue_ptrlis[c] = src.queue_ptrlis[c].clone() if torch.is_tensor(src.queue_ptrlis[c]) else src.queue_ptrlis[c]
    dst.iter_num = src.iter_num
    ops.bump_weight_epoch()


def test_graphed_student_passes_match_eager():
    """From equal state, a step whose student passes replay as HIP graphs (graphs.GraphedTrain; steps 3..) gives
    the losses, weights and banks of the eager step."""
    b, patch, C = 2, (64, 64), 4
    seed_state = (fx.unet_state(21, 1, C), fx.fe_state(31), [fx.fe_state(32)["fea4.weight"], fx.fe_state(33)["fea4.weight"]])
    st_e, st_g = _trainer(0, seed_state), _trainer(1, seed_state)
    rs = np.random.RandomState(5)
    for it in range(6):
        l = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda()
        u = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda()
        lab = torch.from_numpy(fx.blob_labels(rs, b, patch, C)).cuda()
        _sync_state(st_g, st_e)
        terms = []
        for st in (st_e, st_g):
            random.seed(10 + it); np.random.seed(10 + it); torch.manual_seed(10 + it)
            st.step(l, lab, u)
            terms.append({k: float(v) for k, v in st.last_terms.items()})
        for k in terms[0]:
            np.testing.assert_allclose(terms[1][k], terms[0][k], rtol=2e-5, atol=1e-6, err_msg=f"step {it} {k}")
        pe, pg = st_e.optimizer.flat_p, st_g.optimizer.flat_p
        assert float((pe - pg).abs().max()) <= 1e-5 * float(pe.abs().max()), it
        for (k, ve), (_, vg) in zip(st_e.model.state_dict().items(), st_g.model.state_dict().items()):
            if ve.is_floating_point():
                np.testing.assert_allclose(vg.cpu().numpy(), ve.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=f"{it} {k}")
            else:
                assert int(ve) == int(vg), k                      # num_batches_tracked
        for be, bg in zip(st_e.memobank, st_g.memobank):
            np.testing.assert_allclose(bg[0].cpu().numpy(), be[0].cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert st_g.s_train_lu.captured        # the labelled + unlabelled halves run as one grouped pass
    # the replayed steps took the gradient-sink path (prediction halves + the head's three feature-map scatters per step)
    assert st_g.s_train_lu.sink_uses >= 4 * 3 and st_g.s_train_lu.cleanup == [] and not any(st_g.s_train_lu.sink_busy)


def test_graphed_unet_pass_is_bit_exact_even_with_a_live_eager_graph():
    """GraphedTrain(U-Net): outputs and every parameter gradient equal the eager pass bit for bit; the capture
    happens while an eager autograd graph over the same parameters is alive (as in the step: u pass, then l pass)."""
    from arco_amd import graphs
    from arco_amd.networks import unetWithArgs as U
    torch.manual_seed(0)
    m = U.UNet(1, 4).cuda().train()
    _drop_off(m)
    gt = graphs.GraphedTrain(m, warmup=0)
    for it in range(3):
        x = torch.rand(2, 1, 64, 64, device="cuda")
        bufs = {k: v.clone() for k, v in m.state_dict().items()}
        pe, _, fe = m(x)
        ge = torch.autograd.grad([pe.sum() + sum(f.sum() for f in fe)], list(m.parameters()), allow_unused=True,
                                 retain_graph=True)
        m.load_state_dict(bufs)                                   # undo the running-stat update
        pg, _, fg = gt(x)                                         # eager graph (pe, fe) still alive here
        for p_ in m.parameters():
            p_.grad = None
        (pg.sum() + sum(f.sum() for f in fg)).backward()
        assert torch.equal(pg.detach(), pe.detach())
        for a, b_ in zip(fg, fe):
            assert torch.equal(a.detach(), b_.detach())
        for p_, g in zip(m.parameters(), ge):
            if g is not None:
                assert torch.equal(p_.grad, g)
        del pg, fg, pe, fe, ge
    assert gt.captured


def test_graphed_dropout_mask_is_fresh_and_shared_with_backward():
    """Dropout inside a captured forward/backward pair: every replay draws a new mask (device salt) and the
    backward replay uses the mask of ITS forward."""
    from arco_amd import graphs, ops

    class Drop(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1, device="cuda"))

        def forward(self, x):
            z = x * self.w                                  # something with a parameter: autograd reaches backward
            return ops.bn_act(z, None, None, None, None, slope=1.0, p=0.5, drop_mode=1)

    m = Drop()
    gt = graphs.GraphedTrain(m, warmup=1)
    masks = []
    for it in range(5):
        x = (torch.rand(2, 16, 8, 8, device="cuda") + 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        a = gt(x)
        a.backward(torch.ones_like(a))
        a = a.detach()                                      # no autograd graph may survive into the next call
        keep_f = (a != 0)
        keep_b = (x.grad != 0)
        assert torch.equal(keep_f, keep_b), it
        frac = float(keep_f.float().mean())
        assert 0.35 < frac < 0.65
        np.testing.assert_allclose(a[keep_f].cpu().numpy(), (2.0 * x.detach())[keep_f].cpu().numpy(), rtol=1e-6)
        masks.append(keep_f.cpu())
    assert gt.captured
    assert not torch.equal(masks[-1], masks[-2]) and not torch.equal(masks[-2], masks[-3])


def test_training_reduces_the_supervised_loss():
    """Functional check of the whole path (forward, losses, backward, flat SGD, EMA, graphs): 40 steps on one fixed
    synthetic batch drive CE + Dice down and keep every quantity finite."""
    from arco_amd import train_arco_2d as T
    b, patch, C = 4, (64, 64), 4
    argv = ["--batch_size", str(b), "--queue_size", "512", "--synthetic", "1", "--num_queries", "64",
            "--num_negatives", "64", "--base_lr", "0.01", "--graphs", "1"]
    args = T.build_parser().parse_args(argv)
    args.patch_size = list(patch)
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    st = T.ArcoStep2D(args, "cuda:0")
    l, lab = T.synthetic_batch(b, patch, C, 1, "cuda:0")
    u, _ = T.synthetic_batch(b, patch, C, 2, "cuda:0")
    sup = []
    for it in range(40):
        loss, reco = st.step(l, lab, u)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(reco)), it
        sup.append(float(st.last_terms["ce"]) + float(st.last_terms["dice"]))
    first, last = sum(sup[:5]) / 5, sum(sup[-5:]) / 5
    assert last < 0.8 * first, (first, last)
    for p in st.model.parameters():
        assert bool(torch.isfinite(p).all())


def test_batched_passes_match_separate_passes_and_ragged_batches_run():
    """One step from equal state: the grouped-BN batched passes (default) give the losses and weights of the separate
    labelled / unlabelled passes (--batched_passes 0); a step whose labelled and unlabelled batches differ in size
    takes the separate-pass route and stays finite."""
    from arco_amd import train_arco_2d as T
    b, patch, C = 2, (64, 64), 4
    seed_state = (fx.unet_state(21, 1, C), fx.fe_state(31), [fx.fe_state(32)["fea4.weight"], fx.fe_state(33)["fea4.weight"]])
    st_a, st_b = _trainer(0, seed_state), _trainer(0, seed_state)
    st_b.batched_passes = False
    rs = np.random.RandomState(9)
    for it in range(3):
        l = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda()
        u = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda()
        lab = torch.from_numpy(fx.blob_labels(rs, b, patch, C)).cuda()
        _sync_state(st_b, st_a)
        terms = []
        for st in (st_a, st_b):
            random.seed(20 + it); np.random.seed(20 + it); torch.manual_seed(20 + it)
            st.step(l, lab, u)
            terms.append({k: float(v) for k, v in st.last_terms.items()})
        for k in terms[0]:
            np.testing.assert_allclose(terms[1][k], terms[0][k], rtol=5e-4, atol=1e-6, err_msg=f"step {it} {k}")
        pa, pb = st_a.optimizer.flat_p, st_b.optimizer.flat_p
        assert float((pa - pb).abs().max()) <= 1e-4 * float(pa.abs().max()), it
    # ragged: 2 labelled + 3 unlabelled images
    st_r = _trainer(0, seed_state)
    st_r.args.k2 = 0.0                                   # (the warp of the equivariance term is built per batch size)
    l = torch.from_numpy(rs.uniform(size=(2, 1, *patch)).astype(np.float32)).cuda()
    u = torch.from_numpy(rs.uniform(size=(3, 1, *patch)).astype(np.float32)).cuda()
    lab = torch.from_numpy(fx.blob_labels(rs, 2, patch, C)).cuda()
    loss, reco = st_r.step(l, lab, u)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(reco))


@pytest.mark.parametrize("three_d", [False, True])
def test_default_trainer_keeps_the_reference_generator_sequence_without_the_pool(three_d):
    """with --revisit 0 (default) the reference's `torch.randn(K, D, *patch)` pool draw (train_arco_2d.py:156,
    train_arco_3d.py:153) is not materialised, but its generator consumption is reproduced (samplers.skip_randn): the
    trainer built with and without the pool initialises identical weights and leaves the CPU generator in the same
    state, i.e. a seeded default run draws the reference's sequence from step 0."""
    from arco_amd import train_arco_2d as T, train_arco_3d as T3
    mod, Step = (T3, T3.ArcoStep3D) if three_d else (T, T.ArcoStep2D)
    out = []
    for revisit in (1, 0):
        argv = ["--batch_size", "2", "--queue_size", "64", "--synthetic", "1", "--K", "4", "--revisit", str(revisit), "--graphs", "0"]
        if three_d:
            argv += ["--num_classes", "2"]
        args = mod.build_parser().parse_args(argv)
        args.patch_size = [16, 16, 16] if three_d else [32, 32]
        random.seed(5); np.random.seed(5); torch.manual_seed(5)
        st = Step(args, "cuda:0")
        out.append((torch.get_rng_state().clone(), {k: v.detach().cpu().clone() for k, v in st.model.state_dict().items()},
                    [p.detach().cpu().clone() for p in st.q_representation.parameters()]))
        del st
    assert torch.equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
    for a, b in zip(out[0][2], out[1][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("variant", ["default", "k2_0", "classmix"])
def test_pass_concurrency_equals_the_single_stream_step(variant):
    """The concurrent schedule (train_arco_2d.TEACHER_SIDE = 4, the default) against the single-stream step (0).  The default step runs
    the statistics-only pass from the step's start, the teacher's grouped pass and the warped student pass on a second stream (forward
    AND backward of the warped pass beside the main pass's, started before the main stream's row lists / bank appends, parameter
    gradients in a second flat buffer merged once), and the image side of the mixing on a third.  From equal state, steps 1-6 (graphs
    captured at the third call, replayed afterwards) must give the losses, weights, BatchNorm buffers and banks of the single-stream
    step - the passes were independent already, only their order in time changed.
    `k2_0`: no warped pass - the statistics pass and the image mixing beside the teacher only (what bench.py's k2_0 run times).
    `classmix`: the masks are the pseudo-labels', so the mixing stays in line behind the teacher's first pass, while the statistics
    pass and the warped pass stay on the side stream."""
    extra = {"default": (), "k2_0": ("--k2", "0.0"), "classmix": ("--apply_aug", "classmix")}[variant]
    side_mode, warped = 4, variant != "k2_0"
    from arco_amd import train_arco_2d as T
    b, patch, C = 2, (64, 64), 4
    seed_state = (fx.unet_state(21, 1, C), fx.fe_state(31), [fx.fe_state(32)["fea4.weight"], fx.fe_state(33)["fea4.weight"]])
    prev = T.TEACHER_SIDE
    try:
        T.TEACHER_SIDE = 0
        st_a = _trainer(1, seed_state, extra)
        T.TEACHER_SIDE = side_mode
        st_b = _trainer(1, seed_state, extra)
        assert st_a.args.k2 == st_b.args.k2 == (1.0 if warped else 0.0) and st_b.args.apply_aug == ("classmix" if variant == "classmix" else "cutmix")
        if warped:
            assert st_b._tps_side and not st_a._tps_side
        rs = np.random.RandomState(5)
        for it in range(6):
            l = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda()
            u = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda()
            lab = torch.from_numpy(fx.blob_labels(rs, b, patch, C)).cuda()
            _sync_state(st_b, st_a)
            terms = []
            for st, mode in ((st_a, 0), (st_b, side_mode)):
                T.TEACHER_SIDE = mode
                random.seed(10 + it); np.random.seed(10 + it); torch.manual_seed(10 + it)
                st.step(l, lab, u)
                torch.cuda.synchronize()
                terms.append({k: float(v) for k, v in st.last_terms.items()})
            for k in terms[0]:
                np.testing.assert_allclose(terms[1][k], terms[0][k], rtol=2e-5, atol=1e-6, err_msg=f"step {it} {k}")
            pa, pb = st_a.optimizer.flat_p, st_b.optimizer.flat_p
            assert float((pa - pb).abs().max()) <= 1e-5 * float(pa.abs().max()), it
            for (k, va), (_, vb) in zip(st_a.model.state_dict().items(), st_b.model.state_dict().items()):
                if va.is_floating_point():
                    np.testing.assert_allclose(vb.cpu().numpy(), va.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=f"{it} {k}")
                else:
                    assert int(va) == int(vb), k
            for (k, va), (_, vb) in zip(st_a.ema_model.state_dict().items(), st_b.ema_model.state_dict().items()):
                if va.is_floating_point():
                    np.testing.assert_allclose(vb.cpu().numpy(), va.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=f"teacher {it} {k}")
            for ba, bb in zip(st_a.memobank, st_b.memobank):
                np.testing.assert_allclose(bb[0].cpu().numpy(), ba[0].cpu().numpy(), rtol=1e-4, atol=1e-6)
        if warped:
            assert st_b.s_train_tps.captured and st_b.s_train_tps.grad_views is not None
            assert float(st_b.optimizer.flat_g2.abs().max()) == 0.0            # merged and cleared
    finally:
        T.TEACHER_SIDE = prev


@pytest.mark.parametrize("schedule", ["eager_two_stream", "graph_replay"])
def test_cfg1_step_vs_cpu_oracle_at_256(schedule):
    """BASELINE.json configs[0] at ITS OWN size against the CPU oracle step: 2 labelled + 2 unlabelled images of
    256 x 256, D = 496, 256 queries x 512 negatives, 4096-key queues, every trainer flag at its default (k1 0.01, k2 1, cutmix, the
    three-level row-sparse head, lazy teacher, batched passes, two streams) except batch_transform (its 8-bit round trips make the two
    sides' data-dependent draws diverge by design: own variants at 64 x 64 above) and dropout (different generators).  Two chained steps:
    every loss term to north_star's 1e-3, bank lengths / pointers / host-generator positions (i.e. every sampled index) equal, bank
    rows and updated weights to 1e-3.  `graph_replay`: three warm-up steps on other data build every graph, the state is rolled back,
    and the two compared steps REPLAY the student / teacher graphs - the schedule bench.py times."""
    from arco_amd import train_arco_2d as T
    import test_configs_at_size_gpu as TC
    b, patch, C, Q, Nn, qs = 2, (256, 256), 4, 256, 512, 4096
    unet_sd, fe_sd = fx.unet_state(21, 1, C), fx.fe_state(31)
    qrep_w = [fx.fe_state(32)["fea4.weight"], fx.fe_state(33)["fea4.weight"]]
    replay = schedule == "graph_replay"
    argv = ["--batch_size", str(b), "--queue_size", str(qs), "--synthetic", "1", "--batch_transform", "0",
            "--graphs", "1" if replay else "0"]
    args = T.build_parser().parse_args(argv)
    assert (args.num_queries, args.num_negatives, args.k1, args.k2, args.apply_aug, args.head_levels) == (Q, Nn, 0.01, 1.0, "cutmix", 3)
    args.patch_size = list(patch)
    st_g = T.ArcoStep2D(args, "cuda:0")
    st_g.model.load_state_dict(unet_sd, strict=True)
    st_g.ema_model.load_state_dict(unet_sd, strict=True)
    st_g.q_feature_extractor.load_state_dict(fe_sd, strict=True)
    st_g.k_feature_extractor.load_state_dict(fe_sd, strict=True)
    with torch.no_grad():
        st_g.q_representation[0].weight.copy_(qrep_w[0])
        st_g.q_representation[1].weight.copy_(qrep_w[1])
    for m in (st_g.model, st_g.ema_model):
        _drop_off(m)
    st_g.keep_debug = True
    if replay:
        snap = TC._snapshot(st_g)
        heads0 = [p.detach().clone() for m in (st_g.q_feature_extractor, st_g.q_representation) for p in m.parameters()]
        wr = np.random.RandomState(99)
        for w in range(3):
            random.seed(50 + w); np.random.seed(50 + w); torch.manual_seed(50 + w)
            st_g.step(torch.from_numpy(wr.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda(),
                      torch.from_numpy(fx.blob_labels(wr, b, patch, C)).cuda(),
                      torch.from_numpy(wr.uniform(size=(b, 1, *patch)).astype(np.float32)).cuda())
        torch.cuda.synchronize()
        assert st_g.s_train_lu.captured and len(st_g.t_fwd_lu.graphs) > 0
        TC._restore(st_g, snap)
        with torch.no_grad():
            for p0, p in zip(heads0, [p for m in (st_g.q_feature_extractor, st_g.q_representation) for p in m.parameters()]):
                p.copy_(p0)
    st_o = cpu_step.make_state(unet_sd, fe_sd, qrep_w)
    bank_o, ptr_o, qsz = fx.fresh_bank(C, 496, qs, 'zeros')
    rs = np.random.RandomState(3)
    for it in range(2):
        l = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32))
        u = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32))
        lab = torch.from_numpy(fx.blob_labels(rs, b, patch, C))
        random.seed(10 + it); np.random.seed(10 + it); torch.manual_seed(10 + it)
        st_g.step(l.cuda(), lab.cuda(), u.cuda())
        gen_g = _generators()
        # The oracle takes the step's gradient-free DECISION inputs (pseudo-labels, entropy masks, teacher probabilities) from the HIP
        # step after comparing them with its own: at 4 x 65 536 pixels a few always sit within fp32 rounding of a threshold, and one
        # flipped pixel changes a sampler argument and with it every later draw of the CPU generator (seen in the first version of
        # this test: step 0 equal draw for draw, step 1 not).  Everything continuous is then compared strictly.
        force = {k: t.detach().cpu() for k, t in st_g.decisions.items()}
        random.seed(10 + it); np.random.seed(10 + it); torch.manual_seed(10 + it)
        cpu_step.step(st_o, l, lab, u, bank_o, ptr_o, qsz, C, k1=0.01, lr=0.01, nq=Q, nn_=Nn, k2=1.0, apply_aug="cutmix", force=force)
        ag = st_o["agree"]
        for k in ("pseudo_logits", "prob_l_t", "prob_u_t"):
            assert ag[k]["max_abs_diff"] < 1e-3, (it, k, ag[k])
        for k in ("pseudo_labels", "low", "high"):
            assert ag[k]["n_diff"] <= max(2, 1e-3 * ag[k]["n"]), (it, k, ag[k])
        assert gen_g == _generators(), f"step {it}: the two sides consumed the host generators differently (a sampled index differs)"
        to, tg = st_o["last_terms"], st_g.last_terms
        for k in ("ce", "dice", "unsup", "reco", "eqv"):
            np.testing.assert_allclose(float(tg[k]), to[k], rtol=1e-3, atol=1e-5, err_msg=f"step {it} {k}")
        assert [int(p) for p in ptr_o] == [int(p) for p in st_g.queue_ptrlis]
        for bo, bg in zip(bank_o, st_g.memobank):
            assert bo[0].shape == bg[0].shape
            np.testing.assert_allclose(bg[0].cpu().numpy(), bo[0].numpy(), rtol=1e-3, atol=2e-4)
    sd_g = st_g.model.state_dict()
    for k, v in st_o["student"].items():
        if v.requires_grad:
            ref = v.detach()
            assert float((sd_g[k].cpu() - ref).abs().max()) / max(1e-6, float(ref.abs().max())) < 1e-3, k
    for k, v in st_o["q_fe"].items():
        ref = v.detach()
        assert float((st_g.q_feature_extractor.state_dict()[k].cpu() - ref).abs().max()) / float(ref.abs().max()) < 1e-3, k
    for i in range(2):
        ref = st_o["q_rep"][i].detach()
        assert float((st_g.q_representation[i].weight.detach().cpu() - ref).abs().max()) / float(ref.abs().max()) < 1e-3
    sd_t = st_g.ema_model.state_dict()
    for k, v in st_o["teacher"].items():
        if v.is_floating_point() and "running" not in k:
            assert float((sd_t[k].cpu() - v).abs().max()) / max(1e-6, float(v.abs().max())) < 1e-3, k
    for name, sd_ref, sd_got in (("student", st_o["student"], sd_g), ("teacher", st_o["teacher"], sd_t)):
        for k, v in sd_ref.items():
            if "running" in k:
                np.testing.assert_allclose(sd_got[k].cpu().numpy(), v.numpy(), rtol=3e-4, atol=1e-4 * float(v.abs().max()), err_msg=f"{name} {k}")
