"""Stage-2 ARCO trainer, 3-D (LA heart V-Net 112x112x80), on MI355X - drop-in for the reference's
code/train_arco_3d.py.  Every flag of train_arco_3d.py:26-87 is accepted with the same name / type /
default (they equal the 2-D trainer's except --patch_size [112,112,80], --func asmc, --k5 0.1).

`ArcoStep3D.step` follows train_arco_3d.py:257-415: V-Net student / teacher forwards, FeatureExtractor_3d, the two
1x1x1 q_representation convs (D=16), the 5-D contrastive loss (arco_amd.loss_helper), CE + Dice, unsupervised CE, the
mixing strategy of --apply_aug, the equivariance block (--eqv_pass), the opt-in revisiting loss (--revisit),
SGD-Nesterov, EMA.  batch_transform is the identity in the reference's 3-D pipeline (augment_3d.py:133-159).
--synthetic 0 trains from an LA dataset directory (build_loaders); --conv_mma selects reduced-precision MFMA operands.
"""
import contextlib
import os

import numpy as np
import torch
import torch.nn as nn

from . import _contrast as C_
from . import dist as adist
from . import augment, glue, graphs, head, ops, stepper
from .stepper import ArcoStepBase
from .tps.rand_tps_3d import RandTPS as RandTPS3D
from .model_3D import ISD_3d, FeatureExtractor_3d
from .train_arco_2d import build_parser as _build_parser_2d

# The step's two schedules (see train_arco_2d.TEACHER_SIDE; same variable, ARCO_TEACHER_SIDE).  PASS_SIDE is read every time the step
# runs, and only its truth matters there:
#   3 (default), the concurrent schedule.  On the second stream `_side`: the teacher - with cutout / cutmix (the mixed images need the
#     host-drawn boxes only) its first pass and its grouped pass as ONE pass over cat(u, l, u_aug) with three BatchNorm groups (running
#     statistics updated group after group: u, l, u_aug - the reference's order, train_arco_3d.py:260-262, 286-287), with classmix (its
#     masks are the pseudo-labels') the grouped pass alone, behind the first pass in line - beside the student's grouped pass (joined
#     behind it); behind the teacher's pass its FeatureExtractor, then the row lists / prototypes, beside the masks and the student's
#     FeatureExtractor (joined before the loss forwards); after iteration 0 the gradient-free warped pass, from the moment the host has
#     drawn the warp (separate passes / ragged batch: behind everything queued so far), bank appends queued after it, joined before the
#     optimiser changes the weights.
#   0, the single-stream schedule (ARCO_TEACHER_SIDE=0): every pass in line; the reference of the parity tests, bench.py's kernel timing.
# Measurements, and the schedules in between that lost theirs: profiles/r04_notes.md to profiles/r06_notes.md (section 20).
PASS_SIDE = stepper.SCHEDULE[1]
# lazy levels of the row-sparse heads: 2 = fea3 / fea4 on rows over the dense 56x56x40 map of fea2 (rounds 2-5), 3 = fea2 on rows too - the
# 224-channel map at 56x56x40 (450 MB at the LA size) is never written (head.LazyHead3dFn with three maps, round 6)
HEAD_LEVELS = int(os.environ.get("ARCO_HEAD3D_LEVELS", "3"))
FM_ROWS_HALF = int(os.environ.get("ARCO_FM_ROWS_HALF", "1"))     # --act_dtype f16: heads read the full-resolution maps as f16 (ops.fm_rows_half)
FEA_DIM_3D = [128, 64, 32, 16, 16]
REP_DIM_3D = 16                                  # train_arco_3d.py:148,207


def build_parser():
    p = _build_parser_2d()
    p.set_defaults(patch_size=[112, 112, 80], func='asmc', k5=0.1, exp='LA/example_training', model='vnet', max_iterations=6000,
                   root_path='/home/weicheng/selfLearning/DTC/data/2018LA_Seg_Training Set')       # train_arco_3d.py:27-36
    next(a for a in p._actions if a.dest == 'conv_mma').choices = ['f32x3', 'f32', 'f16', 'bf16']   # the volume kernels' extra modes
    next(a for a in p._actions if a.dest == 'act_dtype').help = (
        "f16: the V-Net's activations and activation gradients are stored as f16 (BASELINE configs[4], 'fp16 MFMA "
        "conv'): f16 matrix cores with fp32 accumulation, fp32 weights / BatchNorm statistics / loss / optimizer; "
        "the heads keep fp32 tensors, their GEMM operands follow --head_mma")
    p.add_argument('--head_mma', type=str, default='auto', choices=['auto', 'f32x3', 'f16', 'bf16'],
                   help="matrix-core operands of the heads' GEMMs (FeatureExtractor_3d, q_representation, the row-sparse heads).  auto: f16 "
                        "with --act_dtype f16 (BASELINE configs[4] 'fp16 MFMA conv + contrastive': operands rounded to f16 in registers, "
                        "fp32 accumulate, gradient operands bf16; the full-resolution maps are read as stored f16 rows), else --conv_mma's mode")
    p.add_argument('--eqv_pass', type=int, default=1,
                   help='1: run the equivariance block of train_arco_3d.py:368-388 (warp + one more student forward); '
                        'its loss only enters the objective at iteration 0 there (:390-393), afterwards it is a logged '
                        'value and a BatchNorm running-statistics update')
    return p


def _lowres(fe, fm):
    """(lo, maps, fea weights) of FeatureExtractor_3d `fe` as the row-sparse head and the lazy teacher of HEAD_LEVELS levels take them."""
    lo, *maps = (fe.forward_lowres1 if HEAD_LEVELS == 3 else fe.forward_lowres2)(fm)
    return lo, maps, [f.weight for f in (fe.fea2, fe.fea3, fe.fea4)[HEAD_LEVELS != 3:]]


class ArcoStep3D(ArcoStepBase):
    """State + one training step of the 3-D hot path (train_arco_3d.py:144-151,195-232,257-415)."""

    def __init__(self, args, device="cuda"):
        self.args = args
        self.dev = torch.device(device)
        half = getattr(args, "act_dtype", "f32") == "f16"
        # weight gradients on the side stream behind their data gradient: -0.3 .. -0.5 ms on the LA step with round 6's 3x3x3 kernels
        # (level on LiTS-f16; the 2-D step loses 1 ms with it and sets 0)
        self._set_modes(conv_mma={"f32": 0, "f16": 1, "bf16": 2, "f32x3": 3}[getattr(args, "conv_mma", "f32x3")], act_half=half,
                        head_mma={"auto": 1 if half else 0, "f32x3": 0, "f16": 1, "bf16": 2}[getattr(args, "head_mma", "auto")],
                        wgrad_side=3)
        # The torch CPU generator is consumed in the reference's order: banks (randn), pool, models, heads, one warp.
        self._build_banks(lambda: torch.randn(1, REP_DIM_3D))             # :144-151
        self.random_pool = None
        if getattr(args, "revisit", 0):                                   # :153-156 (drawn right after the banks)
            args.dense_head = 1
            assert args.K % args.batch_size == 0, "--K must be a multiple of --batch_size (train_arco_3d.py:110)"
            self.random_pool = glue.RevisitPool(args.K, REP_DIM_3D, args.patch_size, self.dev)
        else:      # the pool's normals are not needed, its place in the CPU-generator sequence is (weight init, samplers, warps)
            from . import samplers
            samplers.skip_randn(args.K * REP_DIM_3D * int(np.prod(args.patch_size)))
        self.isd = ISD_3d(K=args.K, m=0.99, Ts=0.01, Tt=0.1, num_classes=args.num_classes,
                          latent_pooling_size=args.latent_pooling_size, latent_feature_size=args.latent_feature_size,
                          output_pooling_size=args.output_pooling_size, train_encoder=True, train_decoder=True).to(self.dev)
        self._build_heads(nn.Conv3d, FeatureExtractor_3d, FEA_DIM_3D, REP_DIM_3D)
        self.tps = self._make_tps(2 * args.batch_size, device) if getattr(args, "eqv_pass", 1) else None    # :231-237
        self._side, self._tps_pending = None, False      # side stream, created on first use (self._stream)
        use_graphs, _ = self._build_graphs()
        self.t_fwd_ulu = graphs.GraphedForward(self.ema_model, enabled=use_graphs)      # (u, l, u_aug) as one three-group pass
        # the warped student pass carries no gradient after iteration 0 (:390-393): replayed as one graph - its ~300 eager
        # launches sat right behind the sampler stage, the stretch of the step where the GPU waits for the host
        self.s_fwd_tps = graphs.GraphedForward(self.model, enabled=use_graphs)

    def _make_tps(self, batch_size, device):
        """:231-237 (the constructor of RandTPS draws one warp, like the reference)."""
        a = self.args
        return RandTPS3D(a.patch_size[0], a.patch_size[1], a.patch_size[2], batch_size=batch_size, sigma=a.tps_sigma,
                         border_padding=False, random_mirror=True, random_scale=(0.8, 1.2), mode='affine', device=device)

    @staticmethod
    def _lazy_teacher(kfe, fm_t):
        return head.LazyTeacher(*_lowres(kfe, fm_t))

    def step(self, l_data, l_label, u_data, epoch_num=0, max_epoch=1):
        a = self.args
        C = a.num_classes
        self._step_head()
        # f16 activation storage with the row-sparse heads: the two full-resolution feature maps are consumed as stored (f16 rows,
        # f16 row-sparse gradients) - no dense cast of a full-resolution map in either direction (ops.fm_rows_half)
        rows_half = ops.ACT_HALF and FM_ROWS_HALF and not getattr(a, "dense_head", 0) and self.random_pool is None
        fm_ctx = ops.fm_rows_half if rows_half else contextlib.nullcontext
        # The teacher's first pass (pseudo-labels, :260-262) would run ALONE at the head of the step (2.2 of 20.8 ms at the LA size).
        # With cutout / cutmix the mixed IMAGES need only the boxes - host draws -, not the pseudo-labels: the boxes are drawn at the
        # reference's point of the generator order, the images are mixed at once, the grouped student pass starts on this stream while
        # the teacher's first pass, merged into its grouped pass, runs beside it on the second; labels and logits are mixed with the
        # same boxes once the teacher is done.  classmix (its masks are the pseudo-labels') keeps the serial order.
        t_merge = bool(PASS_SIDE and a.apply_aug in ("cutout", "cutmix") and self.batched_passes and l_data.shape == u_data.shape)
        if t_merge:
            self._stream("_side")
            mix_desc = augment.draw_boxes(int(u_data.shape[0]), tuple(int(v) for v in u_data.shape[2:]))
            u_aug = augment.mix_images(u_data, a.apply_aug, mix_desc)
        else:
            with torch.no_grad(), ops.logits_only():                         # :260-262
                pred_u0, _, _ = self.t_fwd_u0(u_data)
                pseudo_logits, pseudo_labels = glue.softmax_max(pred_u0)
            if self.keep_debug:      # tests: the teacher's decisions before the mixing (cutout writes -1 into the labels in place)
                dbg_pseudo = (pseudo_labels.clone(), pseudo_logits.clone())
            # :268-278: the mixing strategy of --apply_aug on the GPU (train_arco_3d.py:270-271); the PIL transforms are identity
            u_aug, u_aug_label, u_aug_logits = augment.generate_unsup_data_3d(u_data, pseudo_labels, pseudo_logits, mode=a.apply_aug)
        self.k_fe_ema.update(0.99)                                      # :279-281
        batched = self.batched_passes and l_data.shape == u_aug.shape
        lazy_t_side = None
        if batched:     # labelled + unlabelled volumes as one pass with two BatchNorm groups (see train_arco_2d.py)
            lu = torch.cat((l_data, u_aug))
            nb_l = int(l_data.shape[0])
            t_side = None
            if PASS_SIDE:      # concurrent: the teacher's grouped pass on a second stream, beside the student forward (see train_arco_2d.TEACHER_SIDE)
                t_side = self._stream("_side")
                t_side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(t_side), torch.no_grad():
                    if t_merge:
                        nb_u = int(u_data.shape[0])
                        with ops.bn_groups(3), fm_ctx():
                            pred_ulu, _, fm_ulu = self.t_fwd_ulu(torch.cat((u_data, lu)))      # :260-262 and :286-287 in one pass
                        pred_u0, pred_t, fm_t = pred_ulu[:nb_u], pred_ulu[nb_u:], [f[nb_u:] for f in fm_ulu]
                        pseudo_logits, pseudo_labels = glue.softmax_max(pred_u0)
                    else:
                        with ops.bn_groups(2), fm_ctx():
                            pred_t, _, fm_t = self.t_fwd_lu(lu)              # :286-287
                    t_done = t_side.record_event()
                    if not getattr(a, "dense_head", 0):   # :292-293 (the teacher's heads: joined before the row lists)
                        kfe = self.k_feature_extractor
                        lazy_t_side = self._lazy_teacher(kfe, fm_t)
            with ops.bn_groups(2), fm_ctx():
                pred_all, _, fm_s = self.s_train_lu(lu)                  # :283-284
            if t_side is not None:
                torch.cuda.current_stream().wait_event(t_done)
            if t_merge:          # (t_done lies behind the teacher's merged pass)
                if self.keep_debug:
                    dbg_pseudo = (pseudo_labels.clone(), pseudo_logits.clone())
                _, u_aug_label, u_aug_logits = augment.generate_unsup_data_3d(u_data, pseudo_labels, pseudo_logits, mode=a.apply_aug, desc=mix_desc)
            pred_l, pred_u = ops.split_batch(pred_all, nb_l)
            if PASS_SIDE:     # the warped pass's inputs (volumes, mixed labels, the grouped pass's logits) exist from here on
                self._fwd_ready = torch.cuda.current_stream().record_event()
        else:
            with ops.bn_defer(0), fm_ctx():                              # running statistics: l first (:283), then u
                pred_u, _, u_fm = self.s_train_u(u_aug)                  # :284
        with torch.no_grad():
            if batched:
                if not PASS_SIDE:
                    with ops.bn_groups(2), fm_ctx():
                        pred_t, _, fm_t = self.t_fwd_lu(lu)              # :286-287
                pred_l_t, pred_u_t = pred_t[:nb_l], pred_t[nb_l:]
            else:
                with fm_ctx():
                    pred_l_t, _, l_fm_t = self.t_fwd_l(l_data)           # :286
                    pred_u_t, _, u_fm_t = self.t_fwd_u(u_aug)            # :287
            alpha_t = 20 * (1 - epoch_num / max_epoch)
            label_l = glue.label_onehot(l_label, C)
            label_u = glue.label_onehot(u_aug_label, C)
            prob_l_t = glue.softmax(pred_l_t)
            prob_u_t = glue.softmax(pred_u_t)
            low_mask_all, high_mask_all = glue.entropy_masks(pred_u, l_label, u_aug_label, alpha_t)
        plan = C_.contrast_masks(label_l, label_u, prob_l_t, prob_u_t, low_mask_all, high_mask_all,
                                 delta_n=a.strong_threshold_u2pl)
        lists_done = None
        if lazy_t_side is not None:
            # row lists and prototypes need the masks and the TEACHER's heads only: on the side stream (behind those heads), beside
            # the student's FeatureExtractor on this one, instead of in line behind it
            self._side.wait_event(torch.cuda.current_stream().record_event())
            with torch.cuda.stream(self._side):
                C_.contrast_lists_protos(plan, None, lazy_t_side)
                lists_done = self._side.record_event()
        if self.keep_debug:      # tests: the step's gradient-free decision inputs (tests/test_step3d_parity_gpu.py)
            self.decisions = dict(pseudo_labels=dbg_pseudo[0], pseudo_logits=dbg_pseudo[1], low=low_mask_all, high=high_mask_all,
                                  prob_l_t=prob_l_t, prob_u_t=prob_u_t)
        dense = getattr(a, "dense_head", 0)
        if not batched:
            with fm_ctx():
                pred_l, _, l_fm = self.s_train_l(l_data)                 # :283
            ops.apply_deferred_bn()
            fm_t = [torch.cat((x, y)) for x, y in zip(l_fm_t, u_fm_t)]
            fm_s = [torch.cat((x, y)) for x, y in zip(l_fm, u_fm)]
        kfe, qfe = self.k_feature_extractor, self.q_feature_extractor
        with torch.no_grad():                                            # :292-293
            if dense:
                rep_all_teacher, lazy_t = kfe(fm_t), None
            elif lazy_t_side is not None:
                rep_all_teacher, lazy_t = None, lazy_t_side
            else:       # teacher rows are only needed as class means (prototypes) and <= queue_size keys per class
                rep_all_teacher, lazy_t = None, self._lazy_teacher(kfe, fm_t)
        fm_s = adist.mark_heads_done(fm_s, self.optimizer, self.heads_start)     # data parallel: heads' gradient bucket reduced early
        if dense:
            rep_all = self.q_rep(qfe(fm_s))                              # :289-296,301
        else:
            s_low = _lowres(qfe, fm_s)
        if lists_done is not None:
            torch.cuda.current_stream().wait_event(lists_done)
        else:       # (dense heads, separate passes, single-stream: in line)
            C_.contrast_lists_protos(plan, rep_all_teacher, lazy_t)     # row lists, prototypes: device-side inputs only
        # the loss forwards need neither counters nor samples: queued before the host blocks (see train_arco_2d.py)
        loss_ce, loss_dice = glue.supervised_loss(pred_l, l_label)       # :306-310
        unsup_loss = glue.compute_unsupervised_loss(pred_u, u_aug_label, u_aug_logits, a.strong_threshold)
        # counters -> [sample-independent GPU work] -> sampler replay on the host -> anchors (see train_arco_2d.py)
        C_.contrast_counts(plan, self.memobank, self.queue_size,
                           adist.anchors_for_rank(a.num_queries, getattr(a, "anchors_per_rank", "split")), a.num_negatives)
        # concurrent, after iteration 0: the gradient-free warped pass (a graph) runs on the second stream; batched: queued first
        warp_side = bool(PASS_SIDE and getattr(a, "eqv_pass", 1) and self.iter_num > 0 and self.s_fwd_tps.enabled)
        warp_first = bool(warp_side and batched)

        def enqueue():                     # teacher key rows -> banks (no generator draws, no use of the sampled indices)
            C_.contrast_enqueue(plan, rep_all_teacher, self.memobank, self.queue_ptrlis, self.queue_size, lazy_teacher=lazy_t,
                                defer_anchor_pix=True)
        if not warp_first:
            enqueue()
        C_.contrast_draw(plan, a.func, defer=True)     # indices collected by contrast_anchor_pix below
        loss_eqv = None
        if getattr(a, "eqv_pass", 1):
            # :368-388.  The warp is drawn after the samplers (same torch-generator order as the reference).
            nb2 = int(l_data.shape[0]) + int(u_aug.shape[0])
            if self.tps is None or self.tps.batch_size != nb2:
                self.tps = self._make_tps(nb2, l_data.device)

            def warp_inputs():
                with torch.no_grad():
                    eq_mask = glue.eqv_mask(torch.cat((l_label, u_aug_label)),
                                            torch.cat((u_aug_logits.new_ones(l_label.shape), u_aug_logits)), a.weak_threshold)
                    self.tps.reset_control_points()                      # :377
                    return (self.tps(torch.cat((l_data, u_aug))), self.tps(eq_mask, padding_mode='zeros'),
                            self.tps(torch.cat((pred_l.detach(), pred_u.detach())), padding_mode='zeros'))
            if warp_side:
                self._stream("_side")
            if warp_first:
                # after iteration 0 the warped pass is a logged value and a running-statistics update (:390-393): nothing of this
                # step waits for it.  Warps, pass and loss run on the second stream from the moment the host has drawn the warp -
                # beside the heads' forwards, row lists and loss forwards of the main stream (a stretch of small launches), the
                # InfoNCE and the start of the backward pass - behind the grouped pass (running statistics: l, u, then this pass),
                # and are joined before the optimiser touches the weights.
                self._side.wait_event(self._fwd_ready)
                with torch.cuda.stream(self._side), torch.no_grad(), ops.logits_only():
                    images_tps, mask_tps, pred_tps_org = warp_inputs()
                    pred_tps = self.s_fwd_tps(images_tps)[0]
                    loss_eqv = glue.eqv_loss(pred_tps, pred_tps_org, mask_tps)
                self._tps_pending = True
                enqueue()
            else:
                images_tps, mask_tps, pred_tps_org = warp_inputs()
                if warp_side:    # (concurrent and not batched: behind everything queued on the main stream so far, beside InfoNCE and backward)
                    self._side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(self._side), torch.no_grad(), ops.logits_only():
                        pred_tps = self.s_fwd_tps(images_tps)[0]
                        loss_eqv = glue.eqv_loss(pred_tps, pred_tps_org, mask_tps)
                    self._tps_pending = True
                else:
                    with torch.set_grad_enabled(self.iter_num == 0), ops.logits_only():   # only iteration 0 back-propagates it (:390-393)
                        pred_tps = (self.model if self.iter_num == 0 else self.s_fwd_tps)(images_tps)[0]                 # :380
                        loss_eqv = glue.eqv_loss(pred_tps, pred_tps_org, mask_tps)
        C_.contrast_anchor_pix(plan)
        zero_path = plan.valid_seg <= 1 or not plan.entries
        if zero_path:
            reco_loss = self.q_representation[1].weight.sum() * 0.0
        elif dense:
            A_all = C_.GatherRowsFn.apply(rep_all, plan.anchor_pix)
            reco_loss, _ = C_.contrast_infonce(plan, A_all, self.memobank, temp=0.5)
        else:
            A_all = head.lazy_head3d(*s_low, self.q_representation[0].weight, self.q_representation[1].weight, plan.anchor_pix)
            reco_loss, _ = C_.contrast_infonce(plan, A_all, self.memobank, temp=0.5)
        if self.keep_debug and plan.valid_seg > 1 and plan.entries:
            self.debug = dict(plan=plan, A_all=A_all.detach(), banks=[m[0] for m in self.memobank])
        first = self.iter_num == 0 and loss_eqv is not None
        if first:
            ws, terms = [1.0, 1.0, 1.0, 1.0], [unsup_loss, loss_dice, loss_ce, loss_eqv]      # :393 (iter_num / max_iterations == 0)
        else:                                                                               # :391 (k4*loss_q only with --revisit 1)
            ws = [a.k1 * adist.anchor_weight(a.num_queries, getattr(a, "anchors_per_rank", "split")), a.k3, 1.0, 1.0]
            terms = [reco_loss, unsup_loss, loss_dice, loss_ce]
        loss_q = None
        if self.random_pool is not None:      # :304 (before the pool update) and :365; constant w.r.t. every parameter
            nb_l = int(l_data.shape[0])
            loss_q = glue.get_revisiting_loss(self.random_pool, rep_all[nb_l:], rep_all_teacher[nb_l:], topk=a.topk)
            glue.revisit_enqueue(rep_all_teacher[nb_l:], self.random_pool)
            if not first:
                ws.append(a.k4); terms.append(loss_q)
        return self._step_tail(ws, terms, zero_path and not first, loss_ce, loss_dice, unsup_loss, reco_loss, loss_eqv, loss_q)

    def _after_backward(self):
        if self._tps_pending:               # the warped pass on the second stream reads the weights the optimiser is about to change
            torch.cuda.current_stream().wait_stream(self._side)
            self._tps_pending = False


def synthetic_volume_batch(b, patch, n_cls, seed, device):
    """LA-shaped synthetic batch: volumes U[0,1), ellipsoid labels."""
    rs = np.random.RandomState(seed)
    img = torch.from_numpy(rs.uniform(size=(b, 1, *patch)).astype(np.float32))
    lab = np.zeros((b, *patch), dtype=np.int64)
    g = np.mgrid[0:patch[0], 0:patch[1], 0:patch[2]]
    for i in range(b):
        for c in range(1, n_cls):
            ctr = [rs.randint(p // 4, 3 * p // 4) for p in patch]
            r = [max(2, rs.randint(p // 8, p // 3)) for p in patch]
            lab[i][sum(((g[d] - ctr[d]) / r[d]) ** 2 for d in range(3)) < 1.0] = c
    return img.to(device), torch.from_numpy(lab).to(device)


def build_loaders(args, generator=None):
    """The two training loaders of train_arco_3d.py:158-190: LAHeartWithIndex (first --labeled_num cases labeled, the
    rest unlabeled) with RandomRotFlip -> RandomCrop(patch) -> ToTensor, drawn with replacement, last batch dropped."""
    from .dataloaders import Compose
    from .dataloaders.la_heart import LAHeartWithIndex, RandomCrop, RandomRotFlip, ToTensor
    tf = lambda: Compose([RandomRotFlip(), RandomCrop(args.patch_size), ToTensor()])
    db_l = LAHeartWithIndex(base_dir=args.root_path, split="train", num=None, transform=tf(), index=args.labeled_num, label_type=1)
    db_u = LAHeartWithIndex(base_dir=args.root_path, split="train", num=None, transform=tf(), index=args.labeled_num, label_type=0)
    return stepper.paired_loaders(db_l, db_u, args.batch_size, generator)      # :171-190


def train(args, snapshot_path):
    return stepper.train(args, snapshot_path, ArcoStep3D, synthetic_volume_batch, build_loaders)


def main(argv=None):
    return stepper.main(argv, build_parser, train)


if __name__ == "__main__":
    main()
