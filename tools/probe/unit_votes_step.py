"""The pipelined train step with unit-length vote features off, off again and on, alternating in ONE process: ms per step, medians per leg.
    python tools/probe/unit_votes_step.py [--rounds N] [--steps K] [--out PATH]
Each round runs K pipelined steps with the mode off, K more with it off, then K with it on (enable_vote_features / disable_vote_features
between them; each mode replays its own captured stretch graph, captured before a leg is timed); the host waits for the device only at the
end of a K-step leg, as in training.  A leg's figure is its wall time / K, the median is over the N legs of a kind.  The two off legs give
the off / off spread of this box and process, the noise band the mode's cost is read against.  With the mode off a step issues the parent
commit's launches, so "off" is the parent; with it on two of the stretch's launches are other kernels and none is added.  --out PATH: the
lines are also written there (profiles/unit_votes_step.txt is the record DESIGN.md section 8 quotes).  Like every step time here, the
figures differ box to box."""
import argparse, gc, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--out", metavar="PATH")
args = ap.parse_args()
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path[:0] = [R]
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


run(10)
net.enable_vote_features("unit"); run(6); net.disable_vote_features()  # the library is loaded and the mode's graph captured and replayed before a leg is timed
gc.collect(); gc.disable()
LEGS = (("mode off", False), ("mode off (second leg)", False), ("mode unit", True))
legs = {name: [] for name, _ in LEGS}
for rep in range(args.rounds):
    for name, on in LEGS:
        if on:
            net.enable_vote_features("unit")
        run(args.steps, legs[name])
        net.disable_vote_features()
med = {name: statistics.median(v) for name, v in legs.items()}
lines = ["%-22s %d x %d steps, ms per step: %s  median %.4f" % (name, args.rounds, args.steps, " ".join("%.3f" % v for v in legs[name]), med[name])
         for name, _ in LEGS]
base = med["mode off"]
for name in ("mode off (second leg)", "mode unit"):
    lines.append("%s - mode off: %+.4f ms per step (%+.2f %% of the step)" % (name, med[name] - base, (med[name] - base) / base * 100))
graphs = net.__dict__.get("_stretch_graphs", {})
lines.append("%d stretch graphs, replays %s, losses finite %s, %s, 8 x 20 480 points"
             % (len(graphs), [g.replays for g in graphs.values()], bool(torch.isfinite(net.last_losses).all()), torch.cuda.get_device_name(0)))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
