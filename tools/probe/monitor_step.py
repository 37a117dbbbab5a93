"""The pipelined train step with the training summaries off or on: ms per step of one process.
    python tools/probe/monitor_step.py [--tree DIR] [--monitor] [--tensors-every N]
--tree DIR: import the package from another checkout (an older tree unpacked under tools/probe/old_tree, see ab_trees.sh; it needs no
monitors when --monitor is not given).  Run the legs alternately from one shell loop: process-to-process spread is ~1 %, box-to-box more."""
import argparse, gc, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--monitor", action="store_true")
ap.add_argument("--tensors-every", type=int, default=0)
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
if args.monitor:
    net.enable_monitors(window=100, tensors_every=args.tensors_every)


def run(k):
    for i in range(k):
        net.train_step(xs[i % 3], gt=gts[i % 3], next_x=[xs[(i + 1) % 3]])


run(10); torch.cuda.synchronize(); gc.collect(); gc.disable()
res = []
for rep in range(5):
    t0 = time.perf_counter(); run(30); torch.cuda.synchronize(); res.append((time.perf_counter() - t0) / 30 * 1e3)
leg = ("monitors on (window 100, tensors_every %d)" % args.tensors_every) if args.monitor else "monitors off"
print("%-44s %-18s ms per step: %s  median %.3f" % (leg, os.path.relpath(R), " ".join("%.3f" % v for v in res), sorted(res)[2]))
if args.monitor:
    r = net.monitors.read()
    print("    read(): steps %d, moving averages %s" % (r["steps"], {k: round(v, 4) for k, v in r["mean"].items()}))
