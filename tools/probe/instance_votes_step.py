"""The pipelined train step with the vote supervision from instance labels off and on, alternating in ONE process: ms per step, medians
per leg.
    python tools/probe/instance_votes_step.py [--off-only] [--rounds N] [--steps K] [--out PATH]
Each round runs K pipelined steps with the mode off, then K with it on (enable_instance_votes / disable_instance_votes between them; the
captured graphs are shared: the launch runs between two of them, behind the loss); the host waits for the device only at the end of a
K-step leg, as in training.  A leg's figure is its wall time / K, the median is over the N legs of a kind.  --off-only: both legs run
with the mode off -- the off / off spread of this box and process, the noise band the mode's cost is read against.  With the mode off
a step issues the parent commit's launches, so "off" is the parent.  The batches are synthetic rooms; point_box is the generating box
of every point (synth.room_scene_labels), whose rows are room_gt's.  --out PATH: the lines are also written there
(profiles/instance_votes_step.txt is the record DESIGN.md section 8 quotes).  Like every step time here, the figures differ box to box."""
import argparse, gc, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--out", metavar="PATH")
args = ap.parse_args()
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path[:0] = [R]
import importlib.util as _iu
_s = _iu.spec_from_file_location("hp", os.path.join(R, "votenet_amd", "hostpin.py")); hostpin = _iu.module_from_spec(_s); _s.loader.exec_module(hostpin); hostpin.pin(0)
import numpy as np
import torch
from votenet_amd import loss as VL, model as VM, synth
dev = torch.device("cuda:0")
SEEDS, B, N = (1000, 500000, 900000), 8, 20480
xs = [torch.from_numpy(synth.room_batch(B, N, s)).to(dev) for s in SEEDS]
gts = [VL.gt_to_device(synth.room_gt(B, N, s), dev) for s in SEEDS]
for gt, s in zip(gts, SEEDS):
    gt["point_box"] = torch.from_numpy(np.stack([synth.room_scene_labels(N, s + i)[0] for i in range(B)])).to(dev)
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


run(10)
net.enable_instance_votes(); run(3); net.disable_instance_votes()  # the library is loaded and its kernel has run before a leg is timed
gc.collect(); gc.disable()
legs = {"a": [], "b": []}
for rep in range(args.rounds):
    for leg in ("a", "b"):
        if leg == "b" and not args.off_only:
            net.enable_instance_votes()
        run(args.steps, legs[leg])
        net.disable_instance_votes()
names = ("mode off", "mode off (second leg)") if args.off_only else ("mode off", "mode instance")
med = [statistics.median(legs[k]) for k in ("a", "b")]
lines = ["%-22s %d x %d steps, ms per step: %s  median %.4f" % (name, args.rounds, args.steps, " ".join("%.3f" % v for v in legs[k]), m)
         for name, k, m in zip(names, ("a", "b"), med)]
lines.append("second leg - first leg: %+.4f ms per step (%+.2f %% of the step), %s, 8 x 20 480 points"
             % (med[1] - med[0], (med[1] - med[0]) / med[0] * 100, torch.cuda.get_device_name(0)))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
