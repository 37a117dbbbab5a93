"""The pipelined train step with the step guard off and on, alternating in ONE process: ms per step, medians per leg.
    python tools/probe/guard_step.py [--tree DIR] [--off-only] [--rounds N] [--steps K]
Each round runs K pipelined steps with the guard off, then K with it on (enable_step_guard / disable_step_guard between them; the captured
graphs are shared: the guard runs behind them); the host waits for the device only at the end of a K-step leg, as in training.  A leg's
figure is its wall time / K, the median is over the N legs of a kind: N x K steps each (the defaults give 240).  --off-only: both legs run unguarded -- the off/off spread of this box and process, the noise band the guard's
cost is read against.  --tree DIR: import the package from another checkout (it needs no step guard with --off-only): the parent
commit against this tree, guard off, issues the same launches.  Like every step time here, the figures differ box to box."""
import argparse, gc, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
args = ap.parse_args()
R = os.path.abspath(args.tree); sys.path[:0] = [R]
import importlib.util as _iu
_s = _iu.spec_from_file_location("hp", os.path.join(R, "votenet_amd", "hostpin.py")); hostpin = _iu.module_from_spec(_s); _s.loader.exec_module(hostpin); hostpin.pin(0)
import torch
from votenet_amd import loss as VL, model as VM, synth
dev = torch.device("cuda:0")
xs = [torch.from_numpy(synth.room_batch(8, 20480, s)).to(dev) for s in (1000, 500000, 900000)]
gts = [VL.gt_to_device(synth.room_gt(8, 20480, s), dev) for s in (1000, 500000, 900000)]
net = VM.VoteNetHotPath(dev, seed=0)
net.init_optimizer(1e-3)


def run(k, keep=None):
    """k pipelined steps; the wall time of the whole leg / k goes to keep (the host never waits inside a leg, as in training)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        net.train_step(xs[i % 3], gt=gts[i % 3], next_x=[xs[(i + 1) % 3]])
    torch.cuda.synchronize()
    if keep is not None:
        keep.append((time.perf_counter() - t0) / k * 1e3)


run(10); gc.collect(); gc.disable()
legs = {"a": [], "b": []}
guard = None
for rep in range(args.rounds):
    for leg in ("a", "b"):
        if leg == "b" and not args.off_only:
            guard = net.enable_step_guard()  # (its counters start again: the last line shows the last leg's)
        run(args.steps, legs[leg])
        if getattr(net, "step_guard", None) is not None:
            net.disable_step_guard()
names = ("guard off", "guard off (second leg)") if args.off_only else ("guard off", "guard on")
med = [statistics.median(legs[k]) for k in ("a", "b")]
for name, k, m in zip(names, ("a", "b"), med):
    print("%-24s %-14s %d x %d steps, ms per step: %s  median %.4f" % (name, os.path.relpath(R), args.rounds, args.steps,
                                                                       " ".join("%.3f" % v for v in legs[k]), m))
print("second leg - first leg: %+.4f ms per step (%+.2f %% of the step)" % (med[1] - med[0], (med[1] - med[0]) / med[0] * 100))
if guard is not None:
    print("    read() of the last guarded leg:", guard.read())
