"""What point features cost: the pipelined train step of the default network against the point_features=4 network, alternating legs in
ONE process, and the input step (subsample_augment against subsample_augment_features) from 8 x ~300 000 raw rows to 8 x 20 480 points.
    python tools/probe/point_features_step.py [--rounds N] [--steps K] [--no-step] [--no-input]
A step leg is K pipelined steps (the host waits for the device only at its end, as in training), its figure the wall time / K; the
median is over the N legs of a kind.  The default leg is THIS tree's default network (point_features=0), not the parent commit's: what
the change does to the default path itself is the existing suite's and bench.py's to show.  The first / second half of the default legs is the default step's own spread, the band the
difference is read against.  The input entries are timed with HIP events around 20 calls, median of 15 such groups, alternating.  Like
every time here, the figures differ box to box: only this same-process alternation counts."""
import argparse, gc, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--no-input", action="store_true")
args = ap.parse_args()
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path[:0] = [R]
import importlib.util as _iu
_s = _iu.spec_from_file_location("hp", os.path.join(R, "votenet_amd", "hostpin.py")); hostpin = _iu.module_from_spec(_s); _s.loader.exec_module(hostpin); hostpin.pin(0)
import numpy as np, torch
from votenet_amd import input_pipeline as IP, loss as VL, model as VM, synth
dev = torch.device("cuda:0")
B, n = 8, 20480
print("device:", torch.cuda.get_device_name(0))

if not args.no_input:
    rng = np.random.default_rng(0)
    sizes = rng.integers(280000, 320000, B)
    arrays = [np.concatenate([rng.normal(size=(m, 3)) * 2, rng.random((m, 3))], 1).astype(np.float32) for m in sizes]
    raw, off = IP.pack_ragged(arrays, dev)
    aug = IP.draw_augmentation(B, np.random.RandomState(1))
    calls = {"subsample_augment": lambda: IP.subsample_augment(raw, off, n, aug, None, seed=3),
             "subsample_augment_features height": lambda: IP.subsample_augment_features(raw, off, n, aug, None, seed=3, height=True, extra_cols=0),
             "subsample_augment_features height + 3 columns": lambda: IP.subsample_augment_features(raw, off, n, aug, None, seed=3, height=True, extra_cols=3),
             "subsample_augment_features 3 columns": lambda: IP.subsample_augment_features(raw, off, n, aug, None, seed=3, height=False, extra_cols=3)}
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for rep in range(15):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 20)
    print("input step, %d scenes of %d..%d raw rows (stride 6, float32) -> %d points, ms per call (20 calls back to back, 15 groups):" % (B, sizes.min(), sizes.max(), n))
    for k, v in ms.items():
        print("    %-48s median %.4f  min %.4f  max %.4f" % (k, statistics.median(v), min(v), max(v)))

if not args.no_step:
    seeds = (1000, 500000, 900000)
    xs = [torch.from_numpy(synth.room_batch(B, n, s)).to(dev) for s in seeds]
    gts = [VL.gt_to_device(synth.room_gt(B, n, s), dev) for s in seeds]
    fs = []
    for x in xs:  # [height | three colours]
        rawx = torch.cat([x.reshape(B * n, 3), torch.rand(B * n, 3, device=dev)], 1).contiguous()
        fs.append(IP.subsample_augment_features(rawx, np.arange(B + 1, dtype=np.int64) * n, n, choice=torch.arange(n, dtype=torch.int32, device=dev).repeat(B, 1),
                                                depth_to_camera=False, height=True, extra_cols=3)[1])
    nets = {"default": VM.VoteNetHotPath(dev, seed=0), "point_features=4": VM.VoteNetHotPath(dev, seed=0, point_features=4)}
    for net in nets.values():
        net.init_optimizer(1e-3)

    def run(name, k, keep=None):
        net = nets[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            if name == "default":
                net.train_step(xs[i % 3], gt=gts[i % 3], next_x=[xs[(i + 1) % 3]])
            else:
                net.train_step(xs[i % 3], gt=gts[i % 3], next_x=[xs[(i + 1) % 3]], feats=fs[i % 3], next_feats=[fs[(i + 1) % 3]])
        torch.cuda.synchronize()
        if keep is not None:
            keep.append((time.perf_counter() - t0) / k * 1e3)
    for name in nets:
        run(name, 10)
    gc.collect(); gc.disable()
    legs = {name: [] for name in nets}
    for rep in range(args.rounds):
        for name in nets:
            run(name, args.steps, legs[name])
    med = {k: statistics.median(v) for k, v in legs.items()}
    for k, v in legs.items():
        print("%-18s %d x %d steps, ms per step: %s  median %.4f" % (k, args.rounds, args.steps, " ".join("%.3f" % t for t in v), med[k]))
    d = legs["default"]
    h = len(d) // 2
    print("default step, first half of its legs against the second: %+.4f ms (its own spread: min %.4f max %.4f)"
          % (statistics.median(d[h:]) - statistics.median(d[:h]), min(d), max(d)))
    print("point_features=4 - default: %+.4f ms per step (%+.2f %% of the step)"
          % (med["point_features=4"] - med["default"], (med["point_features=4"] - med["default"]) / med["default"] * 100))
