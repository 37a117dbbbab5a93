"""The step guard of a training run: a train step whose gradient is not finite does no harm (include/votenet_step_guard.h,
csrc/guard/step_guard.hip, libvotenet_guard.so).

A step here takes a few milliseconds and the host never waits for the device, so nobody looks at a step's numbers while it runs; one NaN
in a gradient would reach every parameter, both Adam moments and the BatchNorm moving averages in that step, and every later step and
predict() after it.  With VoteNetHotPath.enable_step_guard() the optimizer runs behind a verdict formed on the device:

  bad step     any of the 32 partial sums of squares per tensor that the optimizer forms anyway is NaN or +-Inf -- a NaN / Inf gradient
               element, or a finite one whose square overflows fp32 (|g| >~ 1.8e19).  Formed on the bucket the optimizer reads (after the
               all-reduce), so data-parallel replicas decide alike.  The loss value takes no part.
               Parameters and Adam moments are not written at all; the moving averages go back to the guard's snapshot.
  good step    exactly votenet_clip_adam's update, bit for bit.  When the moving averages are all finite they become the new snapshot;
               when they are not (a NaN activation that did not reach the gradient) they are restored as well.
  step count   net._step counts every call, skipped or not (TensorFlow's global_step); Adam's bias correction uses it, so after a skip
               t runs one ahead of the number of applied updates.

The counters live on the device (int32) and are diagnostics: read() is the only read-back, they are no part of a checkpoint, and
enable_step_guard() starts them at zero.  One launch more than an unguarded step; off (the default) a step is what it was."""
import torch

from . import _lib as L
from . import mlp as M

COUNTERS = ("seen", "skipped", "consecutive", "last_skip_step", "ema_restores")  # guard_state[1:6] (votenet_step_guard.h)


def apply_rules(state, grad_bad, ema_bad, step, have_ema=True):
    """The counter rules of the verdict launch on a host list of ints (the restatement tests hold the device to): state as read()
    orders it behind the verdict word -> (new state, restore the moving averages?)."""
    verdict, seen, skipped, consecutive, last, restores = state
    restore = bool(have_ema and (grad_bad or ema_bad))
    seen += 1
    if grad_bad:
        skipped, consecutive, last = skipped + 1, consecutive + 1, step
    else:
        consecutive = 0
    return [int(bool(grad_bad)), seen, skipped, consecutive, last, restores + int(restore)], restore


class StepGuard:
    """The guard's device state for one VoteNetHotPath: the counters and the snapshot of net._ema_flat."""

    def __init__(self, net):
        if not hasattr(net, "_seg"):
            raise L.InvalidArgumentError("enable_step_guard: the optimizer has no state yet -- call init_optimizer() (or load a "
                                         "checkpoint) first")
        self.state_ints = L.side_lib("guard").votenet_step_guard_state_ints()
        self.state = torch.zeros(self.state_ints, dtype=torch.int32, device=net.store.flat.device)
        net._ema_state()  # (creates _ema_flat on first use)
        self._ema = net._ema_flat
        self.snapshot = self._ema.clone() if self._ema is not None else None

    def refresh_snapshot(self):
        """The snapshot becomes a copy of the moving averages as they are now: after anything but a train step rewrote them in place
        (a checkpoint restore), or a bad step would bring back the averages from before."""
        if self.snapshot is not None:
            self.snapshot.copy_(self._ema)

    def apply(self, net, grad_scale):
        """The optimizer of this train step behind the verdict (train_step calls this in place of mlp.clip_adam)."""
        if net._ema_flat is not self._ema:
            raise L.VotenetError("step guard: the model's moving-average buffer was replaced; enable_step_guard() again")
        M.clip_adam_guarded(net._seg, net._sumsq, net.store.flat, net.store.grad, net._m, net._v, net._lr, net._step, self.state,
                            ema=self._ema, ema_snapshot=self.snapshot, grad_scale=grad_scale)
        net._ema_version += 1  # the launch may have rewritten the averages: inference_bn() must not serve a table built before it

    def read(self):
        """The counters as a dict (the guard's only read-back: it waits for the device)."""
        s = self.state.cpu().tolist()
        out = dict(zip(COUNTERS, s[1:1 + len(COUNTERS)]))
        out["last_step_skipped"] = bool(s[0])
        return out
