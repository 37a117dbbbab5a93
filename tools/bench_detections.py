"""The cost of the per-class detection protocol at BASELINE config 3's shape, 8 scenes x 256 proposals x 10 classes:
  predict (forward + decode + NMS, prefetched geometry, nothing sized on the host) under the reference's protocol and the paper's,
  and the two entries of libvotenet_detect.so alone on the proposals of one predict call: votenet_class_nms3d in its four modes,
  votenet_eval_match_rows on the 20 480 rows of the per-class mode beside votenet_eval_match on the reference protocol's kept rows.
    python tools/bench_detections.py [--nms-overlap {rotated,aabb3d,bev}] [--nms-old-type]
--nms-overlap aabb3d / bev: the per-class predict call and the NMS lines are timed a second time with aabb_nms.class_nms_aabb
(libvotenet_aabb.so) in class_nms3d's place, on the same proposals; --nms-old-type: with its intersection-over-the-later-box measure.
Device time per call by events over 30 calls after 6 warm-up calls (tools/bench_mlp_util.timeit)."""
import argparse, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [R, R + "/tools"]
import torch
from votenet_amd import detections as D, evaluator as E, synth
from votenet_amd.model import VoteNetHotPath
from bench_mlp_util import timeit
ap = argparse.ArgumentParser()
ap.add_argument("--nms-overlap", choices=("rotated", "aabb3d", "bev"), default="rotated")
ap.add_argument("--nms-old-type", action="store_true")
args = ap.parse_args()
if args.nms_old_type and args.nms_overlap == "rotated":
    ap.error("--nms-old-type needs --nms-overlap aabb3d or bev")
measure = "over_later" if args.nms_old_type else "iou"
dev = torch.device("cuda:0")
B, n = 8, 20480
net = VoteNetHotPath(dev, seed=0)
xs = [torch.from_numpy(synth.room_batch(B, n, 1000 + B * i)).to(dev) for i in range(3)]
gt = E.gt_to_device(E.gt_for_eval(synth.room_gt(B, n, 1000)), dev)
i = [0]
def predict(protocol, **kw):
    k = i[0]; i[0] += 1
    return net.predict(xs[k % 3], 0.25, next_x=[xs[(k + 1) % 3], xs[(k + 2) % 3]], sync=False, batch_statistics=True, protocol=protocol, **kw)
for protocol in ("reference", "per_class"):
    print("predict, 8 scenes, protocol %-9s: %.3f ms per call" % (protocol, timeit(lambda: predict(protocol), it=30, warm=6)))
if args.nms_overlap != "rotated":
    t = timeit(lambda: predict("per_class", nms_overlap=args.nms_overlap, nms_measure=measure), it=30, warm=6)
    print("predict, 8 scenes, protocol per_class, NMS overlap %s / %s: %.3f ms per call" % (args.nms_overlap, measure, t))
ref, per = predict("reference"), net.predict(xs[0], 0.25, sync=False, batch_statistics=True, protocol="per_class")
obj = per["proposals_output"][..., :2].contiguous()
for class_nms in (True, False):
    for per_class in (True, False):
        t = timeit(lambda: D.class_nms3d(per["bboxes"], obj, per["class_scores"], 0.25, 0.05, class_nms, per_class), it=30, warm=6)
        print("  class_nms3d 8 x 256 x 10, class_nms %-5s per_class %-5s: %.3f ms" % (class_nms, per_class, t))
        if args.nms_overlap != "rotated":
            from votenet_amd import aabb_nms
            t = timeit(lambda: aabb_nms.class_nms_aabb(per["bboxes"], obj, per["class_scores"], 0.25, 0.05, class_nms, per_class, args.nms_overlap,
                                                       measure), it=30, warm=6)
            print("  class_nms_aabb (%s / %s), class_nms %-5s per_class %-5s: %.3f ms" % (args.nms_overlap, measure, class_nms, per_class, t))
acc = E.DetectionAccumulator(dev, capacity=1 << 22)
def add(pred):
    acc.reset()
    acc.add(pred, gt)
print("  eval_match_rows, %d rows offered: %.3f ms" % (per["det_rows"].shape[0], timeit(lambda: add(per), it=30, warm=6)))
print("  eval_match, %d kept rows offered:  %.3f ms" % (ref["nms_idx"].shape[0], timeit(lambda: add(ref), it=30, warm=6)))
