"""The dynamic loss scale and the overflow guard of the f16-activation-storage mode (--act_dtype f16), shared by the 2-D and the 3-D
stepper: ops.from_half's backward multiplies the gradients that enter the f16 region by ops.LOSS_SCALE, so every parameter gradient of
the network body carries the factor; the stepper divides it out of the body's stretch of the flat gradient, replaces an overflowed
step by a zero-gradient step (on the device, no host synchronisation) and adapts the scale a step later.

A stepper that mixes this in provides: self.optimizer (flat_g), self.heads_start (flat_g[:heads_start] = the network body,
flat_g[heads_start:] = the fp32 heads' bucket), self.args.loss_scale, self.iter_num, and calls
    _loss_scale_update()                    at the start of a step,
    ok = _unscale_and_guard()               after backward (and after merging a second gradient buffer), before dist.allreduce_grads,
    _guard_heads_and_publish(ok)            after dist.allreduce_grads, before optimizer.step()."""
import logging

import torch

from . import dist as adist
from . import graphs, ops


class LossScaleGuard:
    _ovf_host = _ovf_event = None
    overflow_steps = _clean_steps = 0

    def _unscale_and_guard(self):
        """--act_dtype f16: divide the loss scale out of the network's stretch of the flat gradient (flat_g[:heads_start]: the V-Net / U-Net) and guard the step against an
        overflow of the f16 backward (an inf / NaN in flat_g would go straight into SGD, the EMA teacher and,
        a step later, the memory banks - silently and for good).  All on the device, no host synchronisation in the step:
        `ok` = every network gradient finite (on every rank); non-finite values are replaced by zeros and the network's gradient is multiplied
        by ok, so an overflowed step leaves the network with weight decay and momentum only instead of poisoning the run (the heads' fp32
        gradients do not pass through the f16 backward; they are guarded behind their all-reduce: _guard_heads_and_publish).
        The flag is copied to pinned memory and read at the START of the next step (long complete by then): an overflow halves
        the loss scale (floor 1), 500 clean steps double it again up to --loss_scale (dynamic loss scaling)."""
        gv = self.optimizer.flat_g[:self.heads_start]
        gv.mul_(1.0 / ops.LOSS_SCALE)
        ok = torch.isfinite(gv).all()
        torch.nan_to_num_(gv, nan=0.0, posinf=0.0, neginf=0.0)
        okf = ok.to(torch.float32).view(1)
        if adist.is_dist():
            # every rank must take the same decision (a rank that zeroed alone would leave the replicas' loss scales, graphs and -
            # through momentum - weights apart): MIN over ranks, issued by every rank every f16 step, in front of the V-Net bucket
            adist.allreduce_min(okf)
        # Only the V-Net's stretch is written: the heads' gradients are fp32, produced UPSTREAM of the f16 backward (always
        # finite), and under data parallelism their bucket flat_g[heads_start:] is already inside an asynchronous all-reduce
        # started by dist.mark_heads_done's backward hook - nothing may write it before allreduce_grads has waited.
        gv.mul_(okf)
        return okf > 0

    def _guard_heads_and_publish(self, ok):
        """Second half of the guard, AFTER allreduce_grads has waited for the heads' bucket: an f16 forward overflow (an inf
        in a feature-map row or in the loss) makes the heads' fp32 gradients NaN although they never pass through the f16 backward.
        The reduced bucket is identical on every rank, so every rank takes the same decision without another collective: non-finite
        values -> zeros, the bucket multiplied by its own finite flag, and the flag folded into the overflow flag that drives the
        dynamic loss scale (copied to pinned memory, read at the start of the next step)."""
        gh = self.optimizer.flat_g[self.heads_start:]
        okh = torch.isfinite(gh).all()
        torch.nan_to_num_(gh, nan=0.0, posinf=0.0, neginf=0.0)
        gh.mul_(okh.to(torch.float32))
        ok = ok.view(1) & okh.view(1)
        if self._ovf_host is None:
            self._ovf_host = torch.ones(1, dtype=torch.bool).pin_memory()
        self._ovf_host.copy_(ok, non_blocking=True)
        self._ovf_event = torch.cuda.Event()
        self._ovf_event.record()

    def _loss_scale_update(self):
        """Host side of the guard: consume last step's flag (see _unscale_and_guard)."""
        ev = self._ovf_event
        if ev is None:
            return
        ev.synchronize()              # recorded a whole step ago: returns at once
        self._ovf_event = None
        if not bool(self._ovf_host[0]):
            self.overflow_steps += 1
            self._clean_steps = 0
            ops.LOSS_SCALE = max(1.0, ops.LOSS_SCALE / 2.0)
            self._recapture_train_graphs()
            logging.warning("f16 backward overflowed at iteration %d: step reduced to a zero-gradient step, loss scale -> %g",
                            self.iter_num - 1, ops.LOSS_SCALE)
        else:
            self._clean_steps += 1
            if self._clean_steps >= 500 and ops.LOSS_SCALE < float(getattr(self.args, "loss_scale", 16384.0)):
                ops.LOSS_SCALE *= 2.0
                self._clean_steps = 0
                self._recapture_train_graphs()

    def _recapture_train_graphs(self):
        """The loss scale is a kernel argument of the boundary cast inside the captured backward graphs: a new scale needs a
        new capture (the next call of each GraphedTrain re-captures; rare)."""
        for v in vars(self).values():
            if isinstance(v, graphs.GraphedTrain):
                v.captured = False
