"""One evaluation pass over 64 held-out synthetic scenes (8 batches of 8 x 20 480 points, mAP@0.25 and @0.5) on a model trained as in
tools/train_eval.py, timed two ways on the same box, alternating:
  (a) per batch and per threshold: predict, then eval_det (host IoU table, Python loop per detection) -- mean of per-batch mAPs;
  (b) evaluator.evaluate: predict(sync=False) -> DetectionAccumulator.add per batch, one read-back -- mAP over the set;
  (b') the same with the ground truth uploaded once beforehand (evaluator.gt_to_device).
    python tools/bench_eval.py [train_steps] [repeats]
Wall time around a device synchronise; medians and the spread of `repeats` alternations after two warm-up rounds."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib.util
_spec = importlib.util.spec_from_file_location("votenet_hostpin", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "votenet_amd", "hostpin.py"))
hostpin = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(hostpin)  # by path: the package's __init__ would import torch first
hostpin.pin(0)
import numpy as np, torch
from votenet_amd import evaluator as E, loss as VL, synth
from votenet_amd.model import VoteNetHotPath

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 600
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
B, n, nb, nval = 8, 20480, 16, 8
net = VoteNetHotPath(dev, seed=0)
net.init_optimizer(1e-3)
xs = [torch.from_numpy(synth.room_batch(B, n, 5000 + B * i)).to(dev) for i in range(nb)]
gts = [VL.gt_to_device(synth.room_gt(B, n, 5000 + B * i), dev) for i in range(nb)]
val_x = [torch.from_numpy(synth.room_batch(B, n, 90000 + B * i)).to(dev) for i in range(nval)]
val_gt = [E.gt_for_eval(synth.room_gt(B, n, 90000 + B * i)) for i in range(nval)]
val_gt_dev = [E.gt_to_device(g, dev) for g in val_gt]
for i in range(steps):
    net.train_step(xs[i % nb], gt=gts[i % nb], next_x=xs[(i + 1) % nb])
torch.cuda.synchronize()
THR = (0.25, 0.5)


def per_batch():
    res = {}
    for thr in THR:
        res[thr] = float(np.nanmean([E.eval_det(net.predict(x, 0.25), g, thr)[1] for x, g in zip(val_x, val_gt)]))
    return res


def streaming(gt):
    res = E.evaluate(net, val_x, gt, THR)
    return {thr: res[thr]["mAP"] for thr in THR}


ways = [("(a) predict + eval_det per batch and threshold", per_batch), ("(b) evaluate, numpy ground truth", lambda: streaming(val_gt)),
        ("(b') evaluate, ground truth on the device", lambda: streaming(val_gt_dev))]
times = {name: [] for name, _ in ways}
last = {}
for r in range(repeats + 2):
    for name, fn in ways:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[name] = fn()
        torch.cuda.synchronize()
        if r >= 2:
            times[name].append((time.perf_counter() - t0) * 1e3)
print("evaluation pass over %d scenes after %d training steps, %d alternations (ms): median [min .. max]" % (B * nval, steps, repeats))
for name, _ in ways:
    t = np.array(times[name])
    print("  %-50s %8.2f [%8.2f .. %8.2f]   mAP@0.25 %.4f  mAP@0.5 %.4f" % (name, np.median(t), t.min(), t.max(), last[name][0.25], last[name][0.5]))
