"""The cost of dropping empty predicted boxes (libvotenet_boxpts.so):
  votenet_box_point_counts (memset + one kernel) at 8 scenes x 256 boxes x 20 480 points -- BASELINE config 3's predict -- and at
  4 x 256 x 80 000, beside a plain torch expression of the same counts on the same GPU (checked equal before it is timed),
  votenet_gate_objectness at 8 x 256, and predict (forward + decode + NMS, prefetched geometry, nothing sized on the host) with and
  without min_points=5 under both protocols.
    python tools/bench_box_points.py
Device time per call by events over 30 calls after 6 warm-up calls (tools/bench_mlp_util.timeit).  One JSON line at the end."""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [R, R + "/tools"]
import numpy as np, torch
from votenet_amd import box_points as BP, evaluator as E, synth
from votenet_amd.model import VoteNetHotPath
from bench_mlp_util import timeit
dev = torch.device("cuda:0")


def torch_counts(boxes, pts):
    """The header's rule as broadcast torch expressions: (B,N,P) intermediates."""
    c0 = boxes[:, :, 0]
    q = pts[:, None, :, :] - c0[:, :, None, :]
    inside = None
    for k in (1, 3, 4):
        e = boxes[:, :, k] - c0
        ee = (e * e).sum(-1)[:, :, None]
        t = (q * e[:, :, None, :]).sum(-1)
        m = (t >= 0) & (t <= ee)
        inside = m if inside is None else inside & m
    return inside.sum(-1, dtype=torch.int32)


def scene(b, n, npts, seed):
    rng = np.random.default_rng(seed)
    boxes = E.box_corners(rng.random((b, n, 3)) * [6, 1.5, 6], rng.random((b, n, 3)) * 1.5 + 0.2, rng.random((b, n)) * 6.28)
    pts = (rng.random((b, npts, 3)) * [6, 1.5, 6]).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(dev), torch.from_numpy(pts).to(dev)


out = {"device": torch.cuda.get_device_name(0)}
for b, n, npts in ((8, 256, 20480), (4, 256, 80000)):
    boxes, pts = scene(b, n, npts, npts)
    got, ref = BP.box_point_counts(boxes, pts), torch_counts(boxes, pts)
    differ = int((got != ref).sum())  # (torch's sums need not associate as the rule does: a point within rounding of a face may differ)
    key = "%dx%dx%d" % (b, n, npts)
    out[key] = dict(kernel_ms=timeit(lambda: BP.box_point_counts(boxes, pts), it=30, warm=6),
                    torch_ms=timeit(lambda: torch_counts(boxes, pts), it=30, warm=6), counts_differing_from_torch=differ,
                    mean_count=float(got.float().mean()))
    print("box_point_counts %-14s: %.4f ms   torch expression: %.3f ms   (%d of %d counts differ, mean count %.1f)"
          % (key, out[key]["kernel_ms"], out[key]["torch_ms"], differ, b * n, out[key]["mean_count"]))
boxes, pts = scene(8, 256, 20480, 1)
counts, obj = BP.box_point_counts(boxes, pts), torch.randn(8, 256, 2, device=dev)
out["gate_8x256_ms"] = timeit(lambda: BP.gate_objectness(obj, counts, 5), it=30, warm=6)
print("gate_objectness 8 x 256: %.4f ms" % out["gate_8x256_ms"])

B, npts = 8, 20480
net = VoteNetHotPath(dev, seed=0)
xs = [torch.from_numpy(synth.room_batch(B, npts, 1000 + B * i)).to(dev) for i in range(3)]
i = [0]
def predict(protocol, min_points):
    k = i[0]; i[0] += 1
    return net.predict(xs[k % 3], 0.25, next_x=[xs[(k + 1) % 3], xs[(k + 2) % 3]], sync=False, batch_statistics=True, protocol=protocol,
                       min_points=min_points)
for protocol in ("reference", "per_class"):
    for mp in (0, BP.PAPER_MIN_POINTS):
        key = "predict_%s_min_points_%d_ms" % (protocol, mp)
        out[key] = timeit(lambda: predict(protocol, mp), it=30, warm=6)
        print("predict, 8 scenes, protocol %-9s min_points %d: %.3f ms per call" % (protocol, mp, out[key]))
print(json.dumps(out))
