"""The pipelined train step with the proposals sampled on the seeds (the default) and on the votes, alternating in ONE process: ms per
step, medians per leg.
    python tools/probe/vote_sampling_step.py [--off-only] [--rounds N] [--steps K] [--out PATH]
    python tools/probe/vote_sampling_step.py --kernels [--reps N]
Each round runs K pipelined steps with the mode off, K with enable_proposal_sampling("vote_fps") -- the fused launch,
vote_sampling.cluster_votes -- and K on a second network from the same seed whose propose() is handed
farthest_point_sample(256, votes_xyz) through its prop_fps argument: the same network function through the five-launch composition of
the existing entries (the control of tests/test_gpu_vote_sampling.py).  Each leg replays its own captured stretch graphs; the host waits
for the device only at the end of a K-step leg, as in training.  A leg's figure is its wall time / K, the median is over the N legs of a
kind.  --off-only: every leg runs with the mode off -- the off / off spread of this box and process, the noise band the mode's cost is
read against.  With the mode off a step issues the parent commit's launches, so "off" is the parent.  --out PATH: the lines are also
written there (profiles/vote_sampling_step.txt is the record DESIGN.md section 8 quotes).
--kernels: no network; N times the fused launch and N times the composition on 8 x 1024 clustered votes -> 256, r = 0.3, K = 64, for a
kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/probe/vote_sampling_step.py --kernels): cluster_votes_kernel
against the summed fps_prefix_t_kernel, fps_prefix_check_kernel, fps_reg_kernel, the gather and ball_query_kernel.  Like every time
here, the figures differ box to box."""
import argparse, gc, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--out", metavar="PATH")
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path[:0] = [R]
import importlib.util as _iu
_s = _iu.spec_from_file_location("hp", os.path.join(R, "votenet_amd", "hostpin.py")); hostpin = _iu.module_from_spec(_s); _s.loader.exec_module(hostpin); hostpin.pin(0)
import numpy as np, torch
from votenet_amd import loss as VL, model as VM, synth, tf_grouping, tf_sampling, vote_sampling as VS
dev = torch.device("cuda:0")

if args.kernels:
    rng = np.random.default_rng(0)
    centres = rng.uniform(-2, 2, (8, 12, 3))
    votes = centres[np.arange(8)[:, None], rng.integers(0, 12, (8, 1024))] + rng.normal(0, 0.1, (8, 1024, 3))
    votes = torch.from_numpy(votes.astype(np.float32)).to(dev)

    def composed():
        fps = tf_sampling.farthest_point_sample(256, votes)
        new_xyz = tf_sampling.gather_point(votes, fps)
        return (fps, new_xyz) + tuple(tf_grouping.query_ball_point(0.3, 64, votes, new_xyz))
    for fn, name in ((lambda: VS.cluster_votes(votes, 256, 0.3, 64), "fused"), (composed, "composed")):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            got = fn()
        torch.cuda.synchronize()
        print("%-9s %d calls back to back, 8 x 1024 -> 256, r 0.3, K 64: %.1f us per call (wall, launches included)"
              % (name, args.reps, (time.perf_counter() - t0) / args.reps * 1e6))
    assert all(torch.equal(a, b) for a, b in zip(VS.cluster_votes(votes, 256, 0.3, 64), composed()))
    sys.exit(0)

xs = [torch.from_numpy(synth.room_batch(8, 20480, s)).to(dev) for s in (1000, 500000, 900000)]
gts = [VL.gt_to_device(synth.room_gt(8, 20480, s), dev) for s in (1000, 500000, 900000)]
net = VM.VoteNetHotPath(dev, seed=0)
net.init_optimizer(1e-3)
comp = VM.VoteNetHotPath(dev, seed=0)  # the composition: the votes' sample through propose's prop_fps argument
comp.init_optimizer(1e-3)
_propose = comp.propose
comp.propose = lambda vx, vp, sx, tape=None, prop_fps=None: _propose(vx, vp, sx, tape, tf_sampling.farthest_point_sample(comp.proposal.npoint, vx))


def run(n, k, keep=None):
    """k pipelined steps of network n; the wall time of the whole leg / k goes to keep (the host never waits inside a leg)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        n.train_step(xs[i % 3], gt=gts[i % 3], next_x=[xs[(i + 1) % 3]])
    torch.cuda.synchronize()
    if keep is not None:
        keep.append((time.perf_counter() - t0) / k * 1e3)


run(net, 10)
net.enable_proposal_sampling("vote_fps"); run(net, 4); net.disable_proposal_sampling()  # the library is loaded, both captures exist
run(comp, 10)
gc.collect(); gc.disable()
legs = {"a": [], "b": [], "c": []}
for rep in range(args.rounds):
    for leg in ("a", "b", "c"):
        if leg == "b" and not args.off_only:
            net.enable_proposal_sampling("vote_fps")
        run(comp if leg == "c" and not args.off_only else net, args.steps, legs[leg])
        net.disable_proposal_sampling()
names = ("mode off", "mode off (second leg)", "mode off (third leg)") if args.off_only else \
    ("mode off", "vote_fps, fused launch", "vote_fps, five launches")
med = [statistics.median(legs[k]) for k in ("a", "b", "c")]
lines = ["%-24s %d x %d steps, ms per step: %s  median %.4f" % (name, args.rounds, args.steps, " ".join("%.3f" % v for v in legs[k]), m)
         for name, k, m in zip(names, ("a", "b", "c"), med)]
for i in (1, 2):
    lines.append("%s - first leg: %+.4f ms per step (%+.2f %% of the step)" % (names[i], med[i] - med[0], (med[i] - med[0]) / med[0] * 100))
lines.append("%s, 8 x 20 480 points" % torch.cuda.get_device_name(0))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
