"""What the 2-D and the 3-D stage-2 trainer share: `ArcoStepBase`, the rank-independent parts of a stepper (the one writer of the
process-wide mode switches, memory banks, heads / optimizer / PackPlans, the graphed passes both ranks have, head and tail of a
step, the lazily created side streams), and the drivers `train`, `main`, `paired_loaders`.

train_arco_2d.ArcoStep2D / train_arco_3d.ArcoStep3D derive from the base and keep what differs: flag validation, the order in
which their constructor consumes the torch CPU generator (spelled out there, piece by piece), and the middle of step() - the tuned
stream choreography of each rank."""
import logging
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

from . import dist as adist
from . import glue, graphs, ops, optim
from .loss_scale import LossScaleGuard


def schedule_levels(value):
    """(train_arco_2d.TEACHER_SIDE, train_arco_3d.PASS_SIDE) for ARCO_TEACHER_SIDE = `value` (None: unset).  The step has two
    schedules: the concurrent one (unset or "4": independent passes side by side on a second stream) and the single-stream one
    ("0": the reference of the parity tests, bench.py's per-kernel timing).  The levels in between are retired: no run under an
    old label on another schedule."""
    if value is None or value == "4":
        return 4, 3
    if value == "0":
        return 0, 0
    raise ValueError(f"ARCO_TEACHER_SIDE={value}: the step has two schedules, 4 (or unset: concurrent) and 0 (single-stream)")


SCHEDULE = schedule_levels(os.environ.get("ARCO_TEACHER_SIDE"))      # the one read of the variable, for both trainers


class ArcoStepBase(LossScaleGuard):
    def _set_modes(self, conv_mma, act_half, head_mma, wgrad_side):
        """THE place that writes the process-wide switches of arco_amd.ops, all five together: called once by each constructor, after
        its flag validation (a refused constructor changes none), before the PackPlans (they carry the f16 packs).  Every switch is
        set both ways, so a stepper built after another one in the same process inherits nothing from it; they persist after the
        constructor."""
        ops.CONV_MMA, ops.ACT_HALF, ops.HEAD_MMA = conv_mma, act_half, head_mma
        ops.LOSS_SCALE = float(getattr(self.args, "loss_scale", 16384.0))
        if ops._WGRAD_SIDE_ENV is None:        # ARCO_WGRAD_SIDE, when given, overrides the trainer's choice
            ops.WGRAD_SIDE = wgrad_side

    def _build_banks(self, first_row):
        """Memory banks (train_arco_2d.py:147-154, train_arco_3d.py:144-151); device resident from the first enqueue on.
        first_row() is each class's initial row - it may draw from the torch CPU generator."""
        args = self.args
        self.memobank, self.queue_ptrlis, self.queue_size = [], [], []
        for i in range(args.num_classes):
            self.memobank.append([first_row()])
            self.queue_size.append(args.queue_size if args.queue_size > 0 else 30000)
            self.queue_ptrlis.append(torch.zeros(1, dtype=torch.long))
        if args.queue_size <= 0:
            self.queue_size[0] = 50000

    def _build_heads(self, conv, extractor, fea_dim, rep_dim):
        """The heads, the optimizer, the teacher copies and the PackPlans around self.isd (train_arco_2d.py:231-267,
        train_arco_3d.py:206-232); draws the heads' weights from the torch CPU generator."""
        args = self.args
        self.model, self.ema_model = self.isd.model, self.isd.ema_model
        self.q_representation = nn.Sequential(conv(rep_dim, rep_dim, kernel_size=1, bias=False),
                                              conv(rep_dim, rep_dim, kernel_size=1, bias=False)).to(self.dev)
        self.k_feature_extractor = extractor(fea_dim=fea_dim, output_dim=rep_dim).to(self.dev)
        self.q_feature_extractor = extractor(fea_dim=fea_dim, output_dim=rep_dim).to(self.dev)
        adist.broadcast_module_states([self.isd, self.q_representation, self.q_feature_extractor,
                                       self.k_feature_extractor])
        params = [p for p in self.model.parameters() if p.requires_grad]
        params_rep = [p for p in self.q_representation.parameters() if p.requires_grad]
        params_fea = [p for p in self.q_feature_extractor.parameters() if p.requires_grad]
        self.heads_start = sum(p.numel() for p in params)     # flat_g[heads_start:] = the heads' gradient bucket (dist.mark_heads_done)
        self.optimizer = optim.SGDNesterov(params + params_rep + params_fea, lr=args.base_lr, weight_decay=0.0001,
                                           momentum=0.9, nesterov=True)
        with torch.no_grad():                                            # 2-D :250-253
            for t, s in zip(self.k_feature_extractor.parameters(), self.q_feature_extractor.parameters()):
                t.data.copy_(s.data)
                t.requires_grad = False
        self.k_fe_ema = optim.EmaPair(self.q_feature_extractor, self.k_feature_extractor)
        for m in (self.model, self.ema_model, self.q_representation, self.k_feature_extractor,
                  self.q_feature_extractor):
            m.train()                                                   # 2-D :263-267
        # packed conv weights: one launch per weight owner per step (ops.PackPlan), refreshed by the owner
        plan_s = ops.PackPlan([self.model, self.q_representation, self.q_feature_extractor], True, half=[ops.ACT_HALF, False, False])
        self.optimizer.plans = [plan_s]
        pairs = self.isd._ensure_ema_pairs()
        pairs[0].plans = [ops.PackPlan([self.ema_model], False, half=[ops.ACT_HALF])]
        for pr in pairs[1:]:
            pr.plans = [ops.PackPlan([], False)]
        self.k_fe_ema.plans = [ops.PackPlan([self.k_feature_extractor], False)]
        self.plans = [plan_s] + [pl for pr in pairs for pl in pr.plans] + self.k_fe_ema.plans
        self.iter_num = 0
        self.keep_debug = False          # tests: keep the last step's plan and anchor rows (self.debug)

    def _build_graphs(self):
        """The passes both ranks replay as HIP graphs (one graph per call site: outputs are static buffers); plain instance
        attributes - LossScaleGuard._recapture_train_graphs finds them through vars(self).  Returns (use_graphs, g_train) for the
        members a rank adds."""
        args = self.args
        use_graphs = bool(getattr(args, "graphs", 1))
        g_train = use_graphs and bool(getattr(args, "graph_train", 0))
        self.batched_passes = bool(getattr(args, "batched_passes", 1))
        self.s_train_u = graphs.GraphedTrain(self.model, enabled=g_train)    # student passes: fwd + bwd graphs
        self.s_train_l = graphs.GraphedTrain(self.model, enabled=g_train)
        self.s_train_lu = graphs.GraphedTrain(self.model, enabled=g_train)
        self.t_fwd_lu = graphs.GraphedForward(self.ema_model, enabled=use_graphs)   # no-grad forwards of the teacher
        self.t_fwd_u0 = graphs.GraphedForward(self.ema_model, enabled=use_graphs)
        self.t_fwd_l = graphs.GraphedForward(self.ema_model, enabled=use_graphs)
        self.t_fwd_u = graphs.GraphedForward(self.ema_model, enabled=use_graphs)
        return use_graphs, g_train

    def _stream(self, name):
        """The side stream kept in attribute `name` (declared None by the constructor), created on first use."""
        s = getattr(self, name)
        if s is None:
            s = torch.cuda.Stream()
            setattr(self, name, s)
        return s

    def q_rep(self, x):
        x = ops.conv(x, self.q_representation[0].weight)
        return ops.conv(x, self.q_representation[1].weight)

    def _step_head(self):
        if ops.ACT_HALF:
            self._loss_scale_update()
        for pl in self.plans:                                            # stale only if someone else touched weights
            if not pl.valid:
                pl.refresh()

    def _before_backward(self):
        """What the rank's side stream owes the main stream before loss.backward() is queued."""

    def _after_backward(self):
        """What the rank's side stream owes the main stream before anyone reads the gradients / changes the weights."""

    def _step_tail(self, ws, terms, touch_heads, loss_ce, loss_dice, unsup_loss, reco_loss, loss_eqv, loss_q):
        """Objective, backward, optimizer, EMA, learning rate (2-D :426-435, 3-D :390-400).  One launch for the weighted sum (and
        one for its backward) instead of a chain of 0-d multiplies and adds."""
        a = self.args
        loss = ops.combine_terms(ws, terms)
        self.optimizer.zero_grad()                                       # 2-D :429-431
        self._before_backward()
        loss.backward()
        ops.join_side()                     # weight gradients queued on the side stream (ops._wgrad)
        self._after_backward()
        if touch_heads:   # `0 * rep.sum()` gives EVERY head parameter a zero gradient: SGD still decays / applies momentum to them
            self.optimizer.touch_from(self.heads_start)
        if ops.ACT_HALF:       # the network body's parameter gradients carry the loss scale of the f16 region
            ok_body = self._unscale_and_guard()
        adist.allreduce_grads(self.optimizer)
        if ops.ACT_HALF:
            self._guard_heads_and_publish(ok_body)
        self.optimizer.step()
        self.isd._momentum_update_key_encoder()                          # 2-D :432
        lr_ = a.base_lr * (1.0 - self.iter_num / a.max_iterations) ** 0.9   # 2-D :433-435
        for g in self.optimizer.param_groups:
            g['lr'] = lr_
        self.iter_num += 1
        # values only: nothing returned or kept may hold this step's autograd graph alive into the next step
        # (graphs.GraphedTrain needs the parameters' gradient accumulators recreated on its capture stream)
        self.last_terms = dict(ce=loss_ce.detach(), dice=loss_dice.detach(), unsup=unsup_loss.detach(),
                               reco=reco_loss.detach())
        if loss_eqv is not None:
            self.last_terms["eqv"] = loss_eqv.detach()
        if loss_q is not None:
            self.last_terms["loss_q"] = loss_q
        return loss.detach(), reco_loss.detach()

    def log_mode(self):
        """train(), rank 0, after every step: a status line of the stepper's mode, where the rank logs one."""

    def log_saved(self, path):
        """train(), rank 0, after a snapshot was written."""


def paired_loaders(db_l, db_u, batch_size, generator=None):
    """The labeled and the unlabeled loader (train_arco_2d.py:196-215, train_arco_3d.py:171-190): the labeled set doubled until it
    is no shorter than the unlabeled one; each loader draws with replacement and drops the last incomplete batch."""
    from torch.utils.data import ConcatDataset, DataLoader
    from torch.utils.data.sampler import RandomSampler
    while len(db_l) < len(db_u):
        db_l = ConcatDataset([db_l, db_l])
    mk = lambda ds: DataLoader(ds, batch_size=batch_size, sampler=RandomSampler(data_source=ds, replacement=True, generator=generator),
                               drop_last=True, pin_memory=True)
    return mk(db_l), mk(db_u)


def train(args, snapshot_path, stepper_cls, synthetic, build_loaders):
    """The training loop of either rank: `stepper_cls` is ArcoStep2D / ArcoStep3D, `synthetic(b, patch, n_cls, seed, device)` makes
    a synthetic (images, labels) batch, `build_loaders(args, generator=)` the two loaders of --synthetic 0 (--gpu_ingest 1 replaces
    their datasets by device-resident banks and descriptor twins)."""
    rank, world = adist.init()
    if getattr(args, "dp_local_thresholds", 0):
        glue.state_reduce_hook = None
    dev = torch.device("cuda", adist.local_rank())
    torch.cuda.set_device(dev)
    stepper = stepper_cls(args, dev)
    b = args.batch_size
    loaders = None
    if args.synthetic:
        iters_per_epoch = 100
        if world > 1:         # every rank draws its own cutmix boxes / sampler indices / warps (seed + rank), after the broadcast
            adist.seed_data_pipeline(args.seed)
    else:
        # data parallel: every rank draws its own samples / augmentations (seed + rank), after the weight broadcast above
        generator = adist.seed_data_pipeline(args.seed) if world > 1 else None
        loaders = build_loaders(args, generator=generator)
        if getattr(args, "gpu_ingest", 0):
            # the datasets go to device memory once (one bank per stream, per rank); from here on a batch is a handful of drawn
            # parameters per sample and one kernel launch, equal to the host loaders' batch bit for bit (dataloaders/gpu_ingest.py)
            from .dataloaders import gpu_ingest
            loaders = gpu_ingest.bank_loaders(loaders, paired_loaders, b, dev, generator)
            logging.info("gpu ingest: {} + {} cases, {:.1f} MB of device memory".format(
                loaders[0].bank.n_cases, loaders[1].bank.n_cases, (loaders[0].bank.nbytes + loaders[1].bank.nbytes) / 1e6))
        iters_per_epoch = len(loaders[1])                              # 2-D :217 iterations per epoch = unlabeled batches
        logging.info("{} iterations per epoch".format(iters_per_epoch))
        resume = "../model/{}_{}_labeledfinal/{}/iter_30000.pth".format(args.resume, args.labeled_num, args.model)
        if os.path.exists(resume):                                      # stage-1 weights (2-D :222-225, 3-D :198-201), when present
            sd = torch.load(resume, map_location="cpu")
            stepper.isd.model.load_state_dict(sd); stepper.isd.ema_model.load_state_dict(sd)
            for pl in stepper.plans:                                    # packed weights are stale now
                pl.valid = False
        else:
            logging.info("no stage-1 checkpoint at {}: training from the random initialisation".format(resume))
    max_epoch = args.max_iterations // iters_per_epoch + 1
    l_iter = u_iter = None
    while stepper.iter_num < args.max_iterations:
        it = stepper.iter_num
        if args.synthetic:
            l_img, l_lab = synthetic(b, args.patch_size, args.num_classes, 2 * it * world + rank, dev)
            u_img, _ = synthetic(b, args.patch_size, args.num_classes, (2 * it + 1) * world + rank, dev)
        else:
            if it % iters_per_epoch == 0:                               # 2-D :268-270 fresh iterators every epoch
                l_iter, u_iter = iter(loaders[0]), iter(loaders[1])
            l_next, u_next = next(l_iter), next(u_iter)
            l_img, l_lab = l_next['image'].to(dev, non_blocking=True), l_next['label'].to(dev, non_blocking=True).long()
            u_img = u_next['image'].to(dev, non_blocking=True)
        loss, reco = stepper.step(l_img, l_lab, u_img, it // iters_per_epoch, max_epoch)
        if rank == 0:
            stepper.log_mode()
            if "loss_q" in stepper.last_terms:                          # --revisit 1: the reference's logged total (2-D :426,457)
                logging.info('iteration %d : loss : %f, reco_loss: %f' % (stepper.iter_num, loss.item(), reco.item()))
            else:
                # the reference's logged `loss` also carries k4*loss_q, the revisiting term (2-D :126-136,334,425) - a constant w.r.t. every
                # parameter (no gradient path: weights, banks and every other logged value are unaffected) that needs the dense
                # representations of both nets; by default it is NOT computed, and the log line says so instead of
                # printing a total that silently differs from the reference's (--revisit 1 computes and adds it)
                logging.info('iteration %d : loss : %f (without the gradient-free revisiting term k4*loss_q, k4 = %g: --revisit 1 adds it), '
                             'reco_loss: %f' % (stepper.iter_num, loss.item(), args.k4, reco.item()))
            if stepper.iter_num % 1000 == 0:                           # 2-D :462-470, 3-D :441-449
                path = os.path.join(snapshot_path, 'iter_' + str(stepper.iter_num) + '.pth')
                # parameters are views into the optimiser's flat buffer: save private copies, not the shared storage
                torch.save({k: v.detach().clone() for k, v in stepper.isd.model.state_dict().items()}, path)
                stepper.log_saved(path)
    return "Training Finished!"


def main(argv, build_parser, train):
    args = build_parser().parse_args(argv)
    torch.set_num_threads(min(4, torch.get_num_threads()))   # host logic only; avoids OpenMP oversubscription stalls
    random.seed(args.seed)                                               # 2-D :505-508
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    snapshot_path = "../model/{}_{}_labeled{}/{}".format(args.exp, args.labeled_num, 'final', args.model)
    try:                                                             # the reference writes next to the repo (../model)
        os.makedirs(snapshot_path, exist_ok=True)
    except OSError:                                                  # read-only parent: keep the run inside the cwd
        snapshot_path = snapshot_path[1:]
        os.makedirs(snapshot_path, exist_ok=True)
    logging.basicConfig(filename=snapshot_path + "/log.txt", level=logging.INFO,
                        format='[%(asctime)s.%(msecs)03d] %(message)s', datefmt='%H:%M:%S')
    logging.getLogger().addHandler(logging.StreamHandler(sys.stdout))
    logging.info(str(args))
    return train(args, snapshot_path)
