"""Input pipeline (votenet_subsample_augment + votenet_augment_boxes) at the BASELINE shape: 8 scenes x 50 000 raw depth
points -> 20 480, against the numpy restatement of the reference's per-scene code on one host core."""
import sys, time, torch
import os; R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [R, os.path.join(R, "tests"), os.path.join(R, "tools")]
import numpy as np
from votenet_amd import input_pipeline as IP
from oracle import oracle_input as OI
from bench_mlp_util import timeit
dev = torch.device("cuda:0")
b, n_raw, n_out = 8, 50000, 20480
rng = np.random.default_rng(0)
aug = IP.draw_augmentation(b, np.random.RandomState(0))
off = np.arange(b + 1) * n_raw
for dt, cols in ((np.float32, 3), (np.float64, 6)):
    rawn = rng.normal(size=(b * n_raw, cols)).astype(dt)
    raw = torch.from_numpy(rawn).to(dev)
    ch = torch.from_numpy(IP.draw_choice(np.random.RandomState(1), [n_raw] * b, n_out)).to(dev)
    row = 3 * rawn.itemsize
    alg = b * n_out * (row + 12)
    for name, c in (("device draw", None), ("host choice", ch)):
        extra = b * n_out * 4 if c is not None else 0
        ms = timeit(lambda: IP.subsample_augment(raw, off, n_out, aug, c, seed=3), it=50)
        print("points %s cols=%d %-11s: %.4f ms  %.0f GB/s algorithmic (%.1f MB)" % (dt.__name__, cols, name, ms, (alg + extra) / ms / 1e6, (alg + extra) / 1e6))
    t = time.perf_counter()
    for s in range(b):
        OI.augment_points(rawn[s * n_raw:(s + 1) * n_raw], np.random.RandomState(s).choice(n_raw, n_out, replace=False), aug.flip_x[s], aug.flip_z[s], aug.angle[s], aug.scale[s], literal=True)
    print("  numpy, one core (choice + augmentation as the reference writes them): %.2f ms / batch" % ((time.perf_counter() - t) * 1e3))
cnt = rng.integers(3, 12, b)
pk = lambda a: IP.pack_ragged(a, dev)
dc, boff = pk([rng.normal(size=(c, 3)) for c in cnt]); ds, _ = pk([np.abs(rng.normal(size=(c, 3))) + .3 for c in cnt])
dh, _ = pk([rng.uniform(-3, 3, c) for c in cnt]); dk, _ = pk([rng.integers(0, 10, c).astype(np.int32) for c in cnt])
print("boxes: %.4f ms / batch" % timeit(lambda: IP.augment_boxes(dc, ds, dh, dk, boff, aug), it=50))

# ---- ground-truth selection (votenet_select_boxes) and the whole path parsed scene -> model inputs (build_batch):
# 8 scenes x 50 000 - 200 000 raw rows -> 20 480, 4 / 16 / 32 objects per scene.  Median and spread of repeated timed launches.
from votenet_amd import sunrgbd
def med(fn, rep=9, it=20):
    t = sorted(timeit(fn, it=it) for _ in range(rep))
    return t[len(t) // 2], t[0], t[-1]
n_raws = rng.integers(50000, 200001, b)
clouds = [np.column_stack([rng.uniform(-3, 3, n), rng.uniform(0.5, 7, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32) for n in n_raws]
raw, off = IP.pack_ragged(clouds, dev)
calib = (np.tile(np.eye(3), (b, 1, 1)), np.tile(np.array([[529.5, 0, 365.0], [0, 529.5, 265.0], [0, 0, 1.0]]), (b, 1, 1)))
print("selection: %d scenes, raw rows %s -> %d" % (b, [int(n) for n in n_raws], n_out))
print("  subsample_augment + augment_boxes (what the pipeline cost before the selection): %.4f ms (min %.4f, max %.4f)"
      % med(lambda: (IP.subsample_augment(raw, off, n_out, aug, None, seed=3), IP.augment_boxes(dc, ds, dh, dk, boff, aug))))
for nobj in (4, 16, 32):
    scenes = []
    for s in range(b):
        cen = np.column_stack([rng.uniform(-2, 2, nobj), rng.uniform(2, 6, nobj), rng.uniform(-1, 1, nobj)])
        scenes.append({"cls": rng.integers(0, 10, nobj).astype(np.int32), "box2d": np.tile([-1e4, -1e4, 1e4, 1e4], (nobj, 1)),
                       "centroid": cen, "half_extent": rng.uniform(0.3, 0.9, (nobj, 3)), "heading": rng.uniform(-3, 3, nobj)})
    objects = sunrgbd.pack_objects(scenes)
    dobj = {k: (torch.from_numpy(v).to(dev) if k != "obj_offset" else v) for k, v in objects.items()}  # labels staged once
    pairs = b * n_out * nobj
    ms, lo, hi = med(lambda: IP.select_boxes(raw, off, calib, dobj, n_out, None, seed=3))
    print("  %2d objects: select_boxes %.4f ms (min %.4f, max %.4f; incl. the read-back of %d counts)  %.1f G pair/s"
          % (nobj, ms, lo, hi, b, pairs / ms / 1e6))
    ms, lo, hi = med(lambda: IP.build_batch(raw, off, calib, dobj, aug, None, seed=3))
    kept = len(IP.build_batch(raw, off, calib, dobj, aug, None, seed=3)[2])
    print("  %2d objects: build_batch  %.4f ms (min %.4f, max %.4f; %d of %d scenes kept)" % (nobj, ms, lo, hi, kept, b))
