"""Stage-2 ARCO trainer, 2-D, on MI355X - drop-in for the reference's code/train_arco_2d.py.

Plugin surface kept identical: every command-line flag of train_arco_2d.py:26-87 (names,
types, defaults; the dead ones are accepted and ignored exactly like the reference),
`--exp` substring dataset dispatch (:91-106), snapshot directory
../model/{exp}_{labeled_num}_labeledfinal/{model} and `iter_N.pth` = state_dict of the
student U-Net with the reference's key names (:462-470, :509-511).

The step itself (train_arco_2d.py:284-435) is `ArcoStep2D.step`: hot path (SURVEY §8a rows
N1-N5, T1, L1-L6, O1) on hand-written HIP kernels.  One process per GPU; with WORLD_SIZE>1
gradients are all-reduced and new negative keys all-gathered over RCCL (arco_amd/dist.py).
Every loss term of the reference step is here: contrastive (k1), unsupervised CE (k3), CE + Dice, the TPS
equivariance term (k2) and - opt-in, --revisit 1, it has no gradient path - the revisiting loss (k4); so is the mixing
strategy of --apply_aug (arco_amd/augment.py) and, with --synthetic 0, the ACDC / MM slice loaders (build_loaders).
Also built: batch_transform (PIL round trip, ColorJitter, GaussianBlur, AdvMorph; --batch_transform).
"""
import argparse
import logging
import contextlib
import os

import numpy as np
import torch
import torch.nn as nn

from . import dist as adist
from . import _contrast as C_
from . import augment, glue, graphs, head, ops, stepper
from .stepper import ArcoStepBase
from .tps import RandTPS
from .model_2D import ISD, FeatureExtractor

FEA_DIM = [256, 128, 64, 32, 16]
REP_DIM = sum(FEA_DIM)          # 496 (train_arco_2d.py:151,232)


def build_parser():
    """Every add_argument of train_arco_2d.py:26-87, same names/types/defaults."""
    p = argparse.ArgumentParser()
    p.add_argument('--root_path', type=str, default='../data/ACDC', help='Name of Experiment')
    p.add_argument('--exp', type=str, default='ACDC/example_training', help='experiment_name')
    p.add_argument('--model', type=str, default='unet', help='model_name')
    p.add_argument('--max_iterations', type=int, default=30000, help='maximum epoch number to train')
    p.add_argument('--batch_size', type=int, default=4, help='batch_size per gpu')
    p.add_argument('--deterministic', type=int, default=1, help='whether use deterministic training')
    p.add_argument('--base_lr', type=float, default=0.01, help='segmentation network learning rate')
    p.add_argument('--patch_size', type=list, default=[256, 256], help='patch size of network input')
    p.add_argument('--seed', type=int, default=1337, help='random seed')
    p.add_argument('--num_classes', type=int, default=4, help='output channel of network')
    p.add_argument('--consistency', type=float, default=0.1, help='consistency')
    p.add_argument('--consistency_rampup', type=float, default=200.0, help='consistency_rampup')
    p.add_argument('--labeled_bs', type=int, default=2, help='labeled_batch_size per gpu')
    p.add_argument('--labeled_num', type=int, default=7, help='labeled data')
    p.add_argument('--strong_threshold', default=0.97, type=float)
    p.add_argument('--strong_threshold_u2pl', default=0.97, type=float)
    p.add_argument('--weak_threshold', default=0.7, type=float)
    p.add_argument('--temp', default=0.5, type=float)
    p.add_argument('--num_negatives', default=512, type=int, help='number of negative keys')
    p.add_argument('--num_queries', default=256, type=int, help='number of queries per segment per image')
    p.add_argument('--mona_feature_size', type=int, default=512, help='the feature size of latent vectors')
    p.add_argument('--apply_aug', default='cutmix', type=str, help='apply semi-supervised method: cutout cutmix classmix')
    p.add_argument('--resume', type=str, default='ACDC/training_pool_latentF512_K36', help='if we should resume from checkpoint')
    p.add_argument('--K', type=int, default=36, help='the size of cache')
    p.add_argument('--k1', type=float, default=0.01, help='the weights for contrastive loss')
    p.add_argument('--k2', type=float, default=1.0, help='the weights for eqv loss')
    p.add_argument('--k3', type=float, default=1.0, help='the weights for unsup loss')
    p.add_argument('--k4', type=float, default=1.0, help='the weights for nn loss')
    p.add_argument('--k5', type=float, default=1.0, help='the weights for nn loss')
    p.add_argument('--topk', type=int, default=5, help='the size of cache')
    p.add_argument('--latent_pooling_size', type=int, default=1, help='the pooling size of latent vector')
    p.add_argument('--latent_feature_size', type=int, default=512, help='the feature size of latent vectors')
    p.add_argument('--output_pooling_size', type=int, default=8, help='the pooling size of output head')
    p.add_argument('--combinations', type=int, default=0, help='0: all, 1: no reco, 2: no unsup')
    p.add_argument('--mask', type=int, default=0, help='0: no mask, 1: use pre_u')
    p.add_argument('--func', type=str, default='smc', help='asmc or smc')
    p.add_argument('--ref_net', type=str, default='vgg19', help='ref_net')
    p.add_argument('--ref_norm', type=bool, default=False, help='ref_norm')
    p.add_argument('--ref_layer1', type=str, default='relu3_2', help='ref_layer1')
    p.add_argument('--ref_layer2', type=str, default='relu5_4', help='ref_layer2')
    p.add_argument('--ref_weight1', type=float, default=0.33, help='ref_weight1')
    p.add_argument('--ref_weight2', type=float, default=1.0, help='ref_weight2')
    p.add_argument('--temperature', type=float, default=.19, help='temperature')
    p.add_argument('--layer_len', type=int, default=-1, help='layer_len')
    p.add_argument('--tps_sigma', type=float, default=0.01, help='tps_sigma')
    # additions of this implementation (not in the reference)
    p.add_argument('--queue_size', type=int, default=0, help='override per-class bank size (0 = reference 50000/30000)')
    p.add_argument('--synthetic', type=int, default=0, help='1: train on synthetic ACDC-shaped tensors')
    p.add_argument('--gpu_ingest', type=int, default=0, choices=[0, 1],
                   help='1 (with --synthetic 0): hold both datasets in device memory and build every batch with one HIP launch from the '
                        'transform parameters drawn on the host - the same draws, the same batches bit for bit, no scipy per sample '
                        '(dataloaders/gpu_ingest.py); 0: the host loaders')
    p.add_argument('--in_chns', type=int, default=1, help='input channels (reference: 1)')
    p.add_argument('--graphs', type=int, default=1, help='1: replay the no-grad U-Net forwards as HIP graphs')
    p.add_argument('--batched_passes', type=int, default=1,
                   help='1: labelled + unlabelled student (and teacher) forwards as one pass with two BatchNorm groups')
    p.add_argument('--graph_train', type=int, default=1,
                   help='1 (with --graphs 1): the student forward+backward passes are HIP graphs too (a third of the '
                        'host launch work per step, results identical); 0: eager launches')
    p.add_argument('--dense_teacher', type=int, default=0, help='1: materialise the dense teacher representation')
    p.add_argument('--teacher_levels', type=int, default=2,
                   help='lazy teacher depth: 2 = dense fea2 output, prototypes pushed through two bilinear adjoints (measured as '
                        'fast as 3); 3 = no dense fea2 output either')
    p.add_argument('--head_levels', type=int, default=3, help='row-sparse head depth: 1 = from the 128x128 level, 2 = from 64x64, 3 = from 32x32')
    p.add_argument('--dense_head', type=int, default=0, help='1: materialise the dense 496-ch student rep (reference dataflow)')
    p.add_argument('--list_dir', type=str, default='', help='list directory of the npz experiments (default: the reference\'s hard-wired paths)')
    p.add_argument('--dp_local_thresholds', type=int, default=0,
                   help='data parallel only. 0: entropy percentiles of the global batch (5 small all-reduces per step); '
                        '1: every rank thresholds its own batch')
    p.add_argument('--batch_transform', type=int, default=1,
                   help='1 (reference behaviour): batch_transform of train_arco_2d.py:287-304 - 8-bit PIL round trip of the '
                        'images / confidences, ColorJitter + GaussianBlur + AdvMorph on the unlabeled stream - on the GPU; '
                        '0: the identity (no generator draws)')
    p.add_argument('--conv_mma', type=str, default='f32x3', choices=['f32x3', 'f32'],
                   help='matrix-core mode of the convolutions / GEMMs (forward and data gradient).  f32x3 (default): fp32-accurate '
                        'products on the bf16 matrix cores - each fp32 operand is split exactly into three bf16 terms, six bf16 '
                        'MFMAs per 32 k instead of eight fp32 MFMAs per 16 k (2.7x fewer matrix-core cycles, error per product '
                        '<= 2^-23); f32: the native fp32 MFMA (bitwise an fma chain).  The 3-D trainer '
                        'adds f16 / bf16: operands of the 3x3x3 convolutions rounded to f16 / bf16, fp32 accumulate (BASELINE '
                        'configs[4], tolerance 1e-2) - the 2-D kernels have no such mode and this parser rejects it')
    p.add_argument('--act_dtype', type=str, default='f32', choices=['f32', 'f16'],
                   help="f16: the U-Net's activations and activation gradients are stored as f16: f16 matrix cores with fp32 "
                        "accumulation, fp32 weights / BatchNorm statistics / loss / optimizer; the heads keep fp32 tensors on fp32 "
                        "feature maps (--fm_rows f16: on f16 rows of the finest maps).  Training-mode passes only (evaluation stays fp32).  Measured 9.04 against 10.87 ms per step at 16 x "
                        "256^2 on one box (profiles/f16_2d_notes.md).  Runs without the fused ConvBlock / pooled "
                        "BatchNorm passes of the default mode; not combined with --dense_head 1 / --revisit 1")
    p.add_argument('--fm_rows', type=str, default='f32', choices=['f32', 'f16'],
                   help="f16 (with --act_dtype f16): the row-sparse heads read the U-Net's finest feature maps as stored - f16 rows, "
                        "f16 row-sparse gradients rounded once from fp32 sums - instead of dense fp32 copies (the student's --head_levels "
                        "finest maps; the teacher's finest --teacher_levels, 1 with --head_levels 1), and the three passes of the step that "
                        "read only the logits cast no map at all.  The low-resolution maps and the logits stay fp32.  Not combined with "
                        "--dense_head 1 / --dense_teacher 1 / --revisit 1.  Figures: profiles/f16_2d_notes.md")
    p.add_argument('--loss_scale', type=float, default=16384.0,
                   help='--act_dtype f16: gradients enter the f16 region multiplied by this power of two')
    p.add_argument('--anchors_per_rank', type=str, default='split', choices=['split', 'full'],
                   help='data parallel only (SURVEY 8e). split: every rank samples num_queries/world anchors per class, so the '
                        'world draws the same total number of queries as the single-process reference; full: num_queries per rank')
    p.add_argument('--revisit', type=int, default=0,
                   help='1: also compute k4*loss_q, the revisiting loss (train_arco_2d.py:126-136,334,398-400). It has no '
                        'gradient path (it only changes the logged loss) and needs the dense student and teacher '
                        'representations, so it switches --dense_head and --dense_teacher on; --K must be a multiple of '
                        '--batch_size, as in the reference')
    return p


def patients_to_slices(dataset, patiens_num):
    """train_arco_2d.py:91-106."""
    ref_dict = None
    if "ACDC" in dataset:
        ref_dict = {"1": 23, "3": 68, "7": 136, "14": 256, "21": 396, "28": 512, "35": 664, "140": 1312}
    elif "MM" in dataset:
        ref_dict = {"1": 38, "2": 76, "5": 191, "10": 382}
    elif "Syn" in dataset or "syn" in dataset:
        ref_dict = {"1": 44, "3": 66, "5": 111, "10": 221}
    elif "Lits" in dataset or "LiTS" in dataset:
        ref_dict = {"1": 167, "5": 835, "10": 1668, "20": 3336, "50": 8340}
    elif "jhu" in dataset or "JHU" in dataset:
        ref_dict = {"1": 57, "5": 275, "10": 568, "100": 5675}
    else:
        print("Error")
    return ref_dict[str(patiens_num)]


# The step's two schedules.  The step is a dependent chain of ~870 kernels, most of them 5-40 us: a kernel rarely fills the chip for its
# whole duration, and one launch floor (~5 us) per link adds up to a third of the step.  Running two INDEPENDENT passes side by side
# fills those gaps.  TEACHER_SIDE is read every time the step runs, and only its truth matters there:
#   4 (default), the concurrent schedule.  On the side stream `_t_stream`: the statistics-only student pass (cj2_l) from the step's
#     start, beside the teacher's first pass (its running-statistics updates postponed into slot 1 of ops.bn_defer, so they still land
#     between l and u; joined before the grouped passes); the teacher's grouped pass beside the student's (joined behind it); the
#     warps and the warped student pass of the equivariance term (when the pass replays its captured graph, --graph_train 1; an
#     eager one stays in line) from the moment the host has drawn the warp - forward beside the
#     heads / InfoNCE (joined before its loss), backward beside the main pass's backward, parameter gradients into a second flat
#     buffer (joined and summed once after backward(): a + b, bit-identical to accumulating in sequence); the bank appends are queued
#     after that pass.  On a third stream `_img_stream`, with cutout / cutmix: the image side of the mixing strategy and of the two
#     batch_transform calls beside the teacher's first pass (joined behind it).
#   0, the single-stream schedule (ARCO_TEACHER_SIDE=0): every pass in line.  bench.py times kernels under it; the parity tests hold
#     the concurrent schedule to it - the passes were independent already, only their order in time is free.
# Measurements, and the schedules in between that lost theirs: profiles/r04_notes.md section 7 to profiles/r06_notes.md.
TEACHER_SIDE = stepper.SCHEDULE[0]
# SIDE_SYNC (round 4's host-side wait in front of loss.backward()) is OFF since round 5: the non-reproducible gradient it hid was a
# gfx950 erratum in ONE compiler-generated instruction of arco_lerp4_cat_rows_bwd, fixed in the kernel (csrc/elementwise.hip,
# tests/test_isa_lint.py, profiles/r05_notes.md section 1).  ARCO_SIDE_SYNC=1 restores the wait (A/B only).
SIDE_SYNC = int(os.environ.get("ARCO_SIDE_SYNC", "0"))


class ArcoStep2D(ArcoStepBase):
    """State + one training step of the 2-D hot path (train_arco_2d.py:147-154,220-253,284-435)."""

    def __init__(self, args, device="cuda"):
        self.args = args
        self.dev = torch.device(device)
        mma = getattr(args, "conv_mma", "f32x3")
        if mma not in ("f32", "f32x3"):      # no silent fp32 run under a reduced-precision label (the modes exist in 3-D only)
            raise ValueError(f"--conv_mma {mma}: the 2-D step computes in f32x3 or f32; f16 / bf16 operands are a 3-D trainer mode")
        half = getattr(args, "act_dtype", "f32") == "f16"           # f16 activation storage of the U-Net
        rows16 = getattr(args, "fm_rows", "f32") == "f16"
        if rows16 and not half:
            raise ValueError("--fm_rows f16 needs --act_dtype f16: with fp32 activation storage there is no f16 feature map to read rows of")
        if rows16:
            for flag in ("dense_head", "revisit", "dense_teacher"):
                if getattr(args, flag, 0):
                    raise ValueError(f"--fm_rows f16 is not combined with --{flag} 1: the dense heads read whole fp32 feature maps "
                                     f"(use --fm_rows f32)")
        if half and (getattr(args, "dense_head", 0) or getattr(args, "revisit", 0)):
            raise ValueError("--act_dtype f16 is not combined with --dense_head 1 / --revisit 1: the dense heads and the revisiting "
                             "term have not been run on the f16 U-Net (use --act_dtype f32)")
        # no reduced-precision heads in 2-D; no side-stream weight gradients (11.0-11.2 -> 12.2-12.3 ms on this step)
        self._set_modes(conv_mma={"f32": 0, "f32x3": 3}[mma], act_half=half, head_mma=0, wgrad_side=0)
        # The torch CPU generator is consumed in the reference's order: pool, banks (zeros: no draw), models, heads, one warp.
        self.random_pool = None
        if getattr(args, "revisit", 0):
            # random_pool (:156-159) is drawn before the models are created, like the reference (same CPU-generator order)
            args.dense_head = args.dense_teacher = 1
            assert args.K % args.batch_size == 0, "--K must be a multiple of --batch_size (train_arco_2d.py:113)"
            self.random_pool = glue.RevisitPool(args.K, 256 + 128 + 64 + 32 + 16, args.patch_size, self.dev)
        else:
            # --revisit 0 (default): the pool's 4.7 GB of normals are not needed, but their place in the CPU-generator
            # sequence is - the weight initialisation below, the samplers and the warps then draw what the reference draws
            # for the same seed (samplers.skip_randn: 0.4 s of state regeneration for K = 36 at 256 x 256)
            from . import samplers
            samplers.skip_randn(args.K * REP_DIM * int(args.patch_size[0]) * int(args.patch_size[1]))
        self._build_banks(lambda: torch.zeros(1, REP_DIM))
        self.isd = ISD(K=args.K, m=0.99, Ts=0.01, Tt=0.1, num_classes=args.num_classes,
                       latent_pooling_size=args.latent_pooling_size, latent_feature_size=args.latent_feature_size,
                       output_pooling_size=args.output_pooling_size, train_encoder=True, train_decoder=True,
                       in_chns=args.in_chns)
        self.isd = self.isd.to(self.dev)
        self._build_heads(nn.Conv2d, FeatureExtractor, FEA_DIM, REP_DIM)
        # RandTPS of the equivariance term: built here like the reference (:255-261; the constructor draws one warp
        # from the generators), rebuilt in step() only if the batch size differs
        self.tps = self._make_tps(2 * args.batch_size, device) if getattr(args, "k2", 0) != 0 else None
        # --fm_rows f16: how many of its finest maps a pass hands out as stored (ops.fm_rows_half(k)) - exactly those its consumer
        # reads as rows only (FeatureExtractor.forward_lowres / _lowres2 / _lowres1 run fp32 GEMMs on the others); the passes that
        # read nothing but the logits cast no map (ops.logits_only).  --fm_rows f32: every pass casts all five, as before.
        hl = getattr(args, "head_levels", 3)
        self.fm_keep_s = (1 if hl == 1 else 3 if hl == 3 else 2) if rows16 else 0
        self.fm_keep_t = (1 if hl == 1 else 3 if getattr(args, "teacher_levels", 2) == 3 else 2) if rows16 else 0
        self._fm_s = (lambda: ops.fm_rows_half(self.fm_keep_s)) if rows16 else contextlib.nullcontext
        self._fm_t = (lambda: ops.fm_rows_half(self.fm_keep_t)) if rows16 else contextlib.nullcontext
        self._fm_none = ops.logits_only if rows16 else contextlib.nullcontext
        # HIP-event timing of the three contrastive-loss segments: only when a profiler asks for it (bench.py sets
        # profile_loss); a training run records no events (no stream bubbles, nothing accumulates)
        self.profile_loss = False
        self.loss_events = []
        self._t_stream = self._img_stream = None     # side streams, created on first use (self._stream)
        self._tps_on_side = False
        use_graphs, g_train = self._build_graphs()
        # the equivariance term's student pass (:415).  Concurrent schedule: replayed on the side stream - its forward beside the
        # heads / InfoNCE, its backward beside the main pass's backward - with a gradient buffer of its own (optim.second_grad_views).
        # Fixed here: the captured graph writes into that buffer whatever TEACHER_SIDE says when the step runs
        self._tps_side = bool(TEACHER_SIDE) and g_train
        self.s_train_tps = graphs.GraphedTrain(self.model, enabled=g_train,
                                               grad_views=self.optimizer.second_grad_views() if self._tps_side else None)
        self.s_fwd_stats = graphs.GraphedForward(self.model, enabled=use_graphs)

    def _make_tps(self, batch_size, device):
        """:255-261 (the constructor of RandTPS draws one warp, like the reference)."""
        a = self.args
        return RandTPS(a.patch_size[0], a.patch_size[1], batch_size=batch_size, sigma=a.tps_sigma, border_padding=False,
                       random_mirror=True, random_scale=(0.8, 1.2), mode='affine', device=device)

    def fm_rows_note(self):
        """Which feature maps the heads read as f16 rows (for the log line of the f16 mode)."""
        if not self.fm_keep_s:
            return "--fm_rows f32: the heads read fp32 copies of all five feature maps"
        names = ["f0", "f1", "f2", "f3", "f4"]
        return ("--fm_rows f16: f16 rows of %s (student) and %s (teacher), no map cast in the logits-only passes"
                % (", ".join(names[5 - self.fm_keep_s:]), ", ".join(names[5 - self.fm_keep_t:])))

    def _teacher_heads(self, fm_t, dense):
        """(dense teacher representation or None, lazy teacher or None): the teacher's FeatureExtractor (:321-322) in the form the
        loss front end consumes - rows are only needed as class means (prototypes) and <= queue_size keys per class."""
        a, kfe = self.args, self.k_feature_extractor
        if getattr(a, "dense_teacher", 0) or dense:
            return kfe(fm_t), None
        levels = 1 if getattr(a, "head_levels", 3) == 1 else 3 if getattr(a, "teacher_levels", 2) == 3 else 2
        return None, head.LazyTeacher(*self._lowres(kfe, fm_t, levels))

    @staticmethod
    def _lowres(fe, fm, levels):
        """(lo, maps, fea weights) of FeatureExtractor `fe` as the row-sparse head and the lazy teacher of `levels` levels take them."""
        lo, *maps = (fe.forward_lowres, fe.forward_lowres2, fe.forward_lowres1)[levels - 1](fm)
        return lo, maps, [f.weight for f in (fe.fea2, fe.fea3, fe.fea4)[3 - levels:]]

    def step(self, l_data, l_label, u_data, epoch_num=0, max_epoch=1):
        """One iteration.  The mixing strategy of --apply_aug (augment.generate_unsup_data) and batch_transform (8-bit PIL
        round trip, ColorJitter, GaussianBlur, AdvMorph: augment.batch_transform) run on the GPU with the reference's host draws.

        Same operations and results as train_arco_2d.py:284-435 restricted to the hot-path loss term;
        the ORDER is arranged for the GPU: everything the host sampler needs (3*C counters) is
        produced first and copied asynchronously, the large teacher/student GEMMs are queued behind
        it, and the torch-CPU-generator index replay runs on the host while they execute."""
        a = self.args
        C = a.num_classes
        self._step_head()
        dense = getattr(a, "dense_head", 0)
        # randomGeneratorWithLogits (:292-293) is a same-size zoom(order=0) = the identity; then the mixing strategy
        # (:296-297) on the GPU with the reference's host draws; other --apply_aug values leave the batch unchanged
        bt = bool(getattr(a, "batch_transform", 1))
        cj2_l = l_data
        if bt:      # :287-290: two calls without augmentation - images_cj1_logits_l (the constant 255 -> 1.0) and images_cj2_l
            # (queued in front of the teacher's pass below, which consumes nothing of the torch CPU generator: the host draws keep
            # the reference's order)
            augment.draw_batch_transform_params(int(l_data.shape[0]), False)         # (only its generator draws matter)
            cj2_l, _, _ = augment.batch_transform(l_data, l_label, torch.ones_like(l_label, dtype=torch.float32), a.patch_size,
                                                  (1.0, 1.0), False)
        stats_early = bool(TEACHER_SIDE and self.batched_passes and l_data.shape == u_data.shape)      # concurrent and batched
        if stats_early:
            # The statistics-only student pass on images_cj2_l (:311) depends on nothing but the weights - it runs on the
            # side stream beside the teacher's first pass (two 8-image passes, neither of which fills the chip alone).  Its
            # running-statistics updates are postponed (slot 1) and land between those of the l and the u half of the grouped
            # student pass below: the reference's order l, cj2_l, u.
            self._stream("_t_stream").wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._t_stream), torch.no_grad(), ops.bn_defer(0, 1), self._fm_none():
                self.s_fwd_stats(cj2_l)
        # img_early (concurrent and batched, cutout / cutmix): the IMAGE side of the mixing strategy and of the two batch_transform calls (:296-304) reads no
        # pseudo-label - the boxes, ColorJitter / blur parameters and AdvMorph fields are host / generator draws, labels pass through
        # batch_transform unchanged and the confidences are only quantised (augment.batch_transform) - so it is queued on a third stream
        # NOW, beside the teacher's first pass and the statistics pass, instead of alone between them and the grouped passes (0.4 ms of
        # small launches).  Same host draws in the same order (the teacher's pass draws nothing); labels and confidences are mixed with
        # the same boxes once the pseudo-labels exist.
        img_early = stats_early and a.apply_aug in ("cutout", "cutmix")
        if img_early:
            mix_desc = augment.draw_boxes(int(u_data.shape[0]), tuple(int(v) for v in u_data.shape[2:]))
            self._stream("_img_stream").wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._img_stream):
                u_mix = augment.mix_images(u_data, a.apply_aug, mix_desc)
                cj2_u = u_aug = u_mix
                if bt:
                    zl = torch.zeros(u_mix.shape[:1] + u_mix.shape[2:], dtype=torch.int64, device=u_mix.device)
                    zg = torch.zeros(u_mix.shape[:1] + u_mix.shape[2:], dtype=torch.float32, device=u_mix.device)
                    cj2_u = augment.batch_transform(u_mix, zl, zg, a.patch_size, (1.0, 1.0), True)[0]
                    u_aug = augment.batch_transform(u_mix, zl, zg, a.patch_size, (1.0, 1.0), True)[0]
        with torch.no_grad(), self._fm_none():                           # :284-286 (reads the logits only)
            pred_u0, _, _ = self.t_fwd_u0(u_data)
            pseudo_logits, pseudo_labels = glue.softmax_max(pred_u0)
            if self.keep_debug:      # tests: the teacher's decisions before the mixing (cutout writes -1 into the labels in place)
                dbg_pseudo = (pseudo_labels.clone(), pseudo_logits.clone())
        if img_early:
            torch.cuda.current_stream().wait_stream(self._img_stream)
            _, u_aug_label, u_aug_logits = augment.generate_unsup_data(u_data, pseudo_labels, pseudo_logits, mode=a.apply_aug, desc=mix_desc)
            if bt:      # batch_transform's 8-bit round trip of the confidences
                lg = u_aug_logits.to(torch.float32).contiguous()
                u_aug_logits = torch.empty_like(lg)
                ops.L.call("arco_quantize8", ops.L.ptr(lg), lg.numel(), ops.L.ptr(u_aug_logits))
        else:
            u_aug, u_aug_label, u_aug_logits = augment.generate_unsup_data(u_data, pseudo_labels, pseudo_logits, mode=a.apply_aug)
            cj2_u = u_aug
            if bt:      # :299-304: two independent strong augmentations of the mixed unlabeled batch
                cj2_u, _, _ = augment.batch_transform(u_aug, u_aug_label, u_aug_logits, a.patch_size, (1.0, 1.0), True)
                u_aug, u_aug_label, u_aug_logits = augment.batch_transform(u_aug, u_aug_label, u_aug_logits, a.patch_size, (1.0, 1.0), True)
        self.k_fe_ema.update(0.99)                                      # :306-308
        batched = self.batched_passes and l_data.shape == u_aug.shape
        if stats_early:           # (the student's BatchNorm buffers - num_batches_tracked - belong to the passes below from here on)
            torch.cuda.current_stream().wait_stream(self._t_stream)
        if batched:
            # the labelled and the unlabelled student forward (:310,312) as ONE batch-2b pass with two BatchNorm
            # groups (ops.bn_groups: per-half batch statistics, running statistics updated half after half) - same
            # results as two passes, every conv / BN / pooling launch works on twice the pixels (the mid and deep
            # U-Net levels are too small to fill the GPU at b images: 20-35 % less kernel time), one backward.
            lu = torch.cat((l_data, u_aug))
            # The u half postpones its running-statistics update (ops.bn_defer) until the images_cj2_l pass below has
            # made its own: the momentum updates then land in the reference's order l, cj2_l, u (:310-312).
            t_side = None
            if TEACHER_SIDE:      # concurrent: the teacher's grouped pass (independent of the student's) on a second stream, beside the student forward
                t_side = self._stream("_t_stream")
                t_side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(t_side), torch.no_grad(), ops.bn_groups(2), self._fm_t():
                    pred_t, _, fm_t = self.t_fwd_lu(lu)
            with ops.bn_groups(2), ops.bn_defer(1), self._fm_s():
                pred_all, _, fm_all = self.s_train_lu(lu)
            if t_side is not None:
                torch.cuda.current_stream().wait_stream(t_side)
            nb_l = int(l_data.shape[0])
            pred_l, pred_u = ops.split_batch(pred_all, nb_l)    # (views; one gradient buffer for both halves in the backward)
        else:
            with ops.bn_defer(0), self._fm_s():                          # running statistics: applied after l and cj2_l
                pred_u, _, u_fm = self.s_train_u(u_aug)                  # :312 (needed first: entropy masks)
        with torch.no_grad():                                            # teacher params carry no grad (:158-160)
            if batched:
                if not TEACHER_SIDE:
                    with ops.bn_groups(2), self._fm_t():
                        pred_t, _, fm_t = self.t_fwd_lu(lu)              # :314-315 as one grouped pass
                pred_l_t, pred_u_t = pred_t[:nb_l], pred_t[nb_l:]
            else:
                with self._fm_t():
                    pred_l_t, _, l_fm_t = self.t_fwd_l(l_data)           # :314
                    pred_u_t, _, u_fm_t = self.t_fwd_u(u_aug)            # :315
            alpha_t = 20 * (1 - epoch_num / max_epoch)                   # :342-393
            label_l = glue.label_onehot(l_label, C)
            label_u = glue.label_onehot(u_aug_label, C)
            prob_l_t = glue.softmax(pred_l_t)
            prob_u_t = glue.softmax(pred_u_t)
            low_mask_all, high_mask_all = glue.entropy_masks(pred_u, l_label, u_aug_label, alpha_t)
            if self.keep_debug:      # the step's gradient-free decision inputs (oracle/cpu_step.py `force=`)
                self.decisions = dict(pseudo_labels=dbg_pseudo[0], pseudo_logits=dbg_pseudo[1], low=low_mask_all, high=high_mask_all,
                                      prob_l_t=prob_l_t, prob_u_t=prob_u_t)
        prof = self.profile_loss
        ev = ev2 = ev3 = None
        if prof:
            ev, ev2, ev3 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3)]
            ev[0].record()
        plan = C_.contrast_masks(label_l, label_u, prob_l_t, prob_u_t, low_mask_all, high_mask_all,
                                 delta_n=a.strong_threshold_u2pl)       # :341-401 (counts -> async D2H)
        if prof:
            ev[1].record()
        # ---- large GPU work queued while the host waits for the counters and samples
        if not batched:
            with self._fm_s():
                pred_l, _, l_fm = self.s_train_l(l_data)                 # :310
        with torch.no_grad():
            # images_cj2_l forward (:311): BN running statistics only - its FE/q_rep outputs (l_feature_map_2,
            # :319,326) are never read.  One graph launch (~1 ms of GPU work) queued BEFORE the host sync: work for
            # the GPU while the host replays the samplers (14.8 vs 15.1 ms/step when queued after the sync).
            if stats_early:
                ops.apply_deferred_bn(1)                                 # cj2_l (ran beside the teacher's first pass), then
                ops.apply_deferred_bn()                                  # the u half / pass
            else:
                with self._fm_none():
                    self.s_fwd_stats(cj2_l)
                ops.apply_deferred_bn()                                  # the u pass's running-statistics update (:312)
            # FeatureExtractor is per-image -> run it once on the batch-concatenated maps (:321-322)
            if not batched:
                fm_t = [torch.cat((x, y)) for x, y in zip(l_fm_t, u_fm_t)]
            rep_all_teacher, lazy_t = self._teacher_heads(fm_t, dense)
        if not batched:
            fm_all = [torch.cat((x, y)) for x, y in zip(l_fm, u_fm)]     # :317-318
        # data parallel: the heads' gradient bucket is all-reduced as soon as the heads' backward is done, under the U-Net's
        fm_all = adist.mark_heads_done(fm_all, self.optimizer, self.heads_start)
        if dense:
            rep_all = self.q_rep(self.q_feature_extractor(fm_all))       # :324-325,330
        else:
            hl = getattr(a, "head_levels", 3)
            s_low = self._lowres(self.q_feature_extractor, fm_all, hl if hl in (1, 3) else 2)
        # supervised CE + Dice and confidence-weighted unsupervised CE (:336-340): they need neither the
        # counters nor the samples - queued before the host blocks.  The equivariance term follows the sampler draw below.
        # k4*loss_q (revisiting loss; no gradient path to any parameter) only with --revisit 1.
        loss_ce, loss_dice = glue.supervised_loss(pred_l, l_label)
        unsup_loss = glue.compute_unsupervised_loss(pred_u, u_aug_label, u_aug_logits, a.strong_threshold)
        eqv_in, tps_on_side = None, False
        if a.k2 != 0:
            # inputs of the equivariance term that depend neither on the counters nor on the warp: queued BEFORE the host
            # blocks on the counters (the stretch between the counters' arrival and the warped student pass is the part
            # of the step where the GPU can run dry: tools/draw_critical.py)
            with torch.no_grad():
                labels_all = torch.cat((l_label, u_aug_label))
                # images_cj1_logits_l (:287-288) is the constant 255 pushed through ToTensor = 1.0 everywhere
                logits_all = torch.cat((u_aug_logits.new_ones(l_label.shape), u_aug_logits))
                eqv_in = (glue.eqv_mask(labels_all, logits_all, a.weak_threshold), torch.cat((cj2_l, cj2_u)),
                          pred_all.detach() if batched else torch.cat((pred_l.detach(), pred_u.detach())))
            # Where the warped pass runs is decided by how the stepper was BUILT: its captured graph writes its parameter gradients
            # into the second buffer, so a replay belongs on the side stream and has to set optimizer._g2_dirty even when a stepper
            # built under the concurrent schedule is stepped with TEACHER_SIDE = 0 (bench.py and the tests turn the graph off
            # before they do that, so neither reaches this corner; without it that gradient would never be merged).
            with self._fm_none():          # (the mode the warped pass is captured under: GraphedTrain replays under no other)
                tps_on_side = self._tps_side and self.s_train_tps.will_replay(eqv_in[1])
            if tps_on_side:                # the warps and the warped pass start from here on the side stream
                self._eqv_in_ready = torch.cuda.Event()
                self._eqv_in_ready.record()
        # per-class row lists and prototypes need the class codes / totals on the DEVICE only: queued before the host blocks
        evp = None
        if prof:
            evp = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            evp[0].record()
        C_.contrast_lists_protos(plan, rep_all_teacher, lazy_t)
        if prof:
            evp[1].record()
        # ---- host: wait for the counters; everything that needs the COUNTS but not the sampled INDICES is queued
        #      first (row lists, prototypes, key rows, bank append, the supervised / unsupervised loss forwards), so the
        #      GPU has work while the host replays the samplers (bit-exact torch-CPU-generator sequence, ~2 ms)
        C_.contrast_counts(plan, self.memobank, self.queue_size,
                           adist.anchors_for_rank(a.num_queries, getattr(a, "anchors_per_rank", "split")), a.num_negatives)
        def enqueue():                     # key rows of the teacher -> banks (no generator draws, no use of the sampled indices)
            if prof:
                ev2[0].record()
            C_.contrast_enqueue(plan, rep_all_teacher, self.memobank, self.queue_ptrlis, self.queue_size,
                                lazy_teacher=lazy_t, defer_anchor_pix=True)
            if prof:
                ev2[1].record()
        warp_first = bool(TEACHER_SIDE and a.k2 != 0)     # concurrent: the warped pass is on the step's critical path - queue it first
        if not warp_first:
            enqueue()
        C_.contrast_draw(plan, a.func, defer=True)     # indices collected by contrast_anchor_pix below
        loss_eqv = None
        if a.k2 != 0:
            # equivariance term (:404-423).  The warp is drawn AFTER the samplers, as in the reference: both consume
            # the torch CPU generator, and the sampled indices must not depend on whether this term is on.
            nb2 = int(l_data.shape[0]) + int(u_aug.shape[0])
            if self.tps is None or self.tps.batch_size != nb2:
                self.tps = self._make_tps(nb2, l_data.device)            # :255-261 (draws one warp, like the reference)
            eq_mask, images_cj2, pred_all_d = eqv_in
            if tps_on_side:
                # The warps and the warped pass do not queue behind the main stream's row lists / bank appends / index uploads:
                # they run on the side stream from the moment the host has drawn the warp, behind `eqv_in` on the main stream
                # (which is behind the grouped pass and the running-statistics updates above).
                self._stream("_t_stream").wait_event(self._eqv_in_ready)
            with torch.cuda.stream(self._t_stream) if tps_on_side else contextlib.nullcontext():
                with torch.no_grad():
                    self.tps.reset_control_points()                      # :412
                    images_tps = self.tps(images_cj2)                    # :411-413 images_cj2
                    mask_tps = self.tps(eq_mask, padding_mode='zeros')
                    pred_tps_org = self.tps(pred_all_d, padding_mode='zeros')
                with self._fm_none():                                    # (reads the logits only)
                    pred_tps = self.s_train_tps(images_tps)[0]           # :415 one more student pass (one BN batch)
            if tps_on_side:
                self.optimizer._g2_dirty = True
            else:
                loss_eqv = glue.eqv_loss(pred_tps, pred_tps_org, mask_tps)   # :419-423
        if warp_first:
            enqueue()
        if prof:
            ev3[0].record()
        C_.contrast_anchor_pix(plan)
        zero_path = plan.valid_seg <= 1 or not plan.entries
        if zero_path:
            reco_loss = self.q_representation[1].weight.sum() * 0.0      # :417-424 zero attached to the graph
        else:
            if dense:
                A_all = C_.GatherRowsFn.apply(rep_all, plan.anchor_pix)
            else:
                A_all = head.lazy_head2d(*s_low, self.q_representation[0].weight, self.q_representation[1].weight, plan.anchor_pix)
            reco_loss, _ = C_.contrast_infonce(plan, A_all, self.memobank, temp=0.5)   # :394-398 (temp default)
            if self.keep_debug:
                self.debug = dict(plan=plan, A_all=A_all.detach(), banks=[m[0] for m in self.memobank])
        if prof:
            ev3[1].record()
            self.loss_events.append((ev, ev2, ev3, evp))  # masks | keys, banks | anchors, head, InfoNCE | lists, prototypes
        if tps_on_side:                    # the heads and the InfoNCE above ran beside the warped pass's forward
            torch.cuda.current_stream().wait_stream(self._t_stream)
            loss_eqv = glue.eqv_loss(pred_tps, pred_tps_org, mask_tps)   # :419-423
        # :426 - one launch for the weighted sum (and one for its backward) instead of a chain of 0-d multiplies and adds
        ws = [a.k1 * adist.anchor_weight(a.num_queries, getattr(a, "anchors_per_rank", "split")), a.k3, 1.0, 1.0]
        terms = [reco_loss, unsup_loss, loss_dice, loss_ce]
        if loss_eqv is not None:
            ws.append(a.k2); terms.append(loss_eqv)
        loss_q = None
        if self.random_pool is not None:
            # :334 (computed before the pool is updated) and :398-400; a constant w.r.t. every parameter
            nb_l = int(l_data.shape[0])
            loss_q = glue.get_revisiting_loss(self.random_pool, rep_all[nb_l:], rep_all_teacher[nb_l:], topk=a.topk)
            glue.revisit_enqueue(rep_all_teacher[nb_l:], self.random_pool)
            ws.append(a.k4); terms.append(loss_q)
        self._tps_on_side = tps_on_side
        return self._step_tail(ws, terms, zero_path, loss_ce, loss_dice, unsup_loss, reco_loss, loss_eqv, loss_q)

    def _before_backward(self):
        if self._tps_on_side and SIDE_SYNC:
            # Round 4 shipped this host-side wait as a workaround: without it 1-3 % of steps had a gradient off by 1e-3..1e-2.  Round 5
            # found the cause - with the host ahead of the GPU the row-sparse head's backward runs BESIDE the warped pass's backward
            # graph (the overlap this schedule wants), and one packed-fp32 instruction the compiler had put into
            # lerp4_cat_rows_bwd_kernel (`v_pk_mul_f32 ... op_sel:[0,1]`, src0 != src1) returns a wrong low half in lanes 48-63 while
            # another wave of the SIMD executes a K-doubled 16x16 MFMA (gfx950 erratum, torch-free reproducer tools/debug/pkmul_repro.hip).
            # The wait only removed the overlap at that point.  The kernel no longer contains the form; 0 of 1200 amplified trials
            # without the wait against 43 of 400 with the old code object on the same box (profiles/r05_notes.md section 1).
            self._t_stream.synchronize()

    def _after_backward(self):
        if self._tps_on_side:
            # the warped pass's backward graph was replayed on the side stream and hands nothing back to autograd (its parameter
            # gradients go straight into the second buffer), so the engine has no leaf stream to synchronise with at the end of
            # backward(): wait for it here.  (Found as a 1-in-3 flake of test_cfg2_graph_replay_equals_eager_at_full_size: the LAST
            # gradient of that backward, the first layer's weight, was merged before it was complete.)
            torch.cuda.current_stream().wait_stream(self._t_stream)
        self.optimizer.merge_second(self.heads_start)      # the warped pass's parameter gradients (replayed on the side stream)

    def log_mode(self):
        if ops.ACT_HALF and (self.iter_num == 1 or self.iter_num % 50 == 0 or self.iter_num == self.args.max_iterations):
            logging.info('iteration %d : --act_dtype f16, loss scale %g, %d overflowed step(s) so far; %s'
                         % (self.iter_num, ops.LOSS_SCALE, self.overflow_steps, self.fm_rows_note()))

    def log_saved(self, path):
        logging.info("save model to {}".format(path))


def synthetic_batch(b, patch, n_cls, seed, device, in_chns=1):
    """ACDC-shaped synthetic batch: images U[0,1), blob labels with ACDC-like imbalance."""
    rs = np.random.RandomState(seed)
    img = torch.from_numpy(rs.uniform(size=(b, in_chns, *patch)).astype(np.float32))
    lab = np.zeros((b, *patch), dtype=np.int64)
    yy, xx = np.mgrid[0:patch[0], 0:patch[1]]
    for i in range(b):
        for c in range(1, n_cls):
            cy, cx = rs.randint(patch[0] // 4, 3 * patch[0] // 4), rs.randint(patch[1] // 4, 3 * patch[1] // 4)
            r = rs.randint(patch[0] // 16, patch[0] // 6)
            lab[i][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = c
    return img.to(device), torch.from_numpy(lab).to(device)


def build_loaders(args, generator=None):
    """The two training loaders of train_arco_2d.py:161-215 (ACDC / MM slice datasets): the first
    patients_to_slices(exp, labeled_num) slices are the labeled stream, the rest the unlabeled one; RandomGenerator per
    sample; each loader draws with replacement and drops the last incomplete batch.  The Synapse / LiTS / JHU branches
    use the npz slice dataset with the reference's hard-wired list directories (--list_dir overrides them)."""
    from .build_dataset import BaseDataSetsWithIndex, Synapse_datasetWithIndex
    from .dataloaders import Compose
    from .dataloaders.dataset import RandomGenerator
    n_lab = patients_to_slices(args.exp, args.labeled_num)
    tf = lambda: Compose([RandomGenerator(args.patch_size)])
    # npz experiments (:162-187): (sub-directory of --root_path, the reference's hard-wired list directory)
    npz = None
    if "Syn" in args.exp or "syn" in args.exp:
        npz = ('/data/Synapse/train_npz', '/data/data/Synapse/data/lists_Synapse')
    elif "Lits" in args.exp or "LiTS" in args.exp:
        npz = ('/train_npz_40', '/data/data/Lits')
    elif "jhu" in args.exp or "JHU" in args.exp:
        npz = ('', '/data/data/JHUData')
    if npz is not None:
        list_dir = getattr(args, "list_dir", "") or npz[1]
        sets = [Synapse_datasetWithIndex(base_dir=args.root_path + npz[0], split="train", transform=tf(), index=n_lab, label_type=t,
                                         list_dir=list_dir) for t in (1, 0)]
    else:
        sets = [BaseDataSetsWithIndex(base_dir=args.root_path, split="train", num=None, transform=tf(), index=n_lab, label_type=t)
                for t in (1, 0)]
    return stepper.paired_loaders(*sets, args.batch_size, generator)           # :196-215


def train(args, snapshot_path):
    return stepper.train(args, snapshot_path, ArcoStep2D, synthetic_batch, build_loaders)


def main(argv=None):
    return stepper.main(argv, build_parser, train)


if __name__ == "__main__":
    main()
