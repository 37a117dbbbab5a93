"""End-to-end check on synthetic rooms (GPU box only): train the hot path with the reference's loss, then run the predict
tower (decode -> 3D NMS) on held-out scenes and report mAP@0.25 / @0.5 with the reference's evaluator logic: "mAP" is the mean
of the per-batch mAPs (the figure of every earlier log), "set mAP" the reference's own metric, detections ranked over the whole
validation set (evaluator.evaluate).
    python tools/train_eval.py [steps] [train_batches] [--save PATH] [--resume PATH] [--monitor K] [--guard] [--height] [--per-class] [--min-points K]
                                                      [--nms-overlap {rotated,aabb3d,bev}] [--nms-old-type] [--paper-votes] [--paper-proposals] [--vote-fps]
                                                      [--unit-votes] [--heading-bins N] [--classes K]
--save PATH: a checkpoint (VoteNetHotPath.save) at every evaluation and at the end.  --resume PATH: continue the run a checkpoint
holds -- parameters, moving averages, Adam state and step count -- up to `steps` steps in all, on the batches it would have seen.  --monitor K: the reference's training summaries from the device
(VoteNetHotPath.enable_monitors): every K steps the moving averages of obj_accuracy / sem_accuracy / total_cost over the last 100 steps
(run.py:127) beside the window's mean n_pos / n_neg, every 10 K steps the five tensors with the smallest and the largest gradient rms.
--guard: the step guard (VoteNetHotPath.enable_step_guard): a step whose gradient is not finite is skipped on the device; the skipped steps
and the restores of the moving averages are printed at the end (with --monitor K: every K steps too).
--height: the network takes one input feature per point, the height above the scene's floor (VoteNetHotPath(point_features=1)), made on
the device by input_pipeline.subsample_augment_features from the same clouds (already in the camera frame; the rooms have no colour).
--per-class: at the end, the set-level mAP under both protocols: the reference's (class-agnostic NMS by the largest class logit, one
detection per kept box) and the VoteNet paper's (detections.class_nms3d: class-wise NMS by objectness, confidence threshold 0.05, one
detection per class and kept box scored P(object) P(class)).
--min-points K: a predicted box that holds fewer than K points of its scene's cloud is dropped before the NMS (box_points; the count runs on
the device) in the set-level evaluations.
--nms-overlap: the overlap the per-class protocol's NMS suppresses by (aabb_nms; --per-class only): rotated, the rotated-box IoU of the
rest of the project (the default); aabb3d, the overlap of the boxes' axis-aligned hulls, the paper's; bev, the same on the ground plane.
--nms-old-type: with aabb3d or bev, the paper's use_old_type_nms: intersection over the later box instead of IoU.
--per-class --min-points 5 --nms-overlap aabb3d is the paper's protocol.
--paper-votes: train with the paper's vote supervision (VoteNetHotPath.enable_vote_supervision("paper"), vote_supervision.py): a seed votes
for the centres of the boxes that contain it, the closest of up to three is charged, the mean is over the supervised seeds; the printed
vote_reg_loss and total cost are then the paper's.  A setting of the run, not of the checkpoint: give it again with --resume.
--paper-proposals: train with the paper's objectness and centre supervision (VoteNetHotPath.enable_proposal_supervision("paper"),
proposal_supervision.py): one cross-entropy weighted 0.2 / 0.8 over all proposals outside the grey zone, and a Chamfer distance between
the predicted centres and the real ground-truth centres; the printed obj_cls_loss, center_loss, box loss and total cost are then the
paper's.  Independent of --paper-votes; likewise a setting of the run.  With both, the two terms whose RULE differed from the paper's
follow it; its size-residual mean over the axes (1/3), its overall x 10 and the BatchNorm momentum schedule are not taken over.
--vote-fps: the proposal module's cluster centres are sampled by farthest-point sampling on the VOTES, the paper's rule
(VoteNetHotPath.enable_proposal_sampling("vote_fps"), vote_sampling.py), in training and in every evaluation of the run; the default
samples the seeds, as the reference does.  Independent of --paper-votes / --paper-proposals; likewise a setting of the run, not of the
checkpoint: evaluate a network under the mode it was trained in.
--unit-votes: each vote's features are divided by their L2 norm before the proposal module reads them, as the authors' VoteNet does
(VoteNetHotPath.enable_vote_features("unit"), unit_votes.py), in training and in every evaluation of the run; the default hands the sum
on as it is, as the reference does.  Independent of the other flags; likewise a setting of the run, not of the checkpoint.
--paper-votes --paper-proposals --vote-fps --unit-votes is the paper's training rule as far as this project follows it.  The run's
modes are printed in its first line.
--heading-bins N --classes K: train and evaluate a network of another detection head (VoteNetHotPath(head=synth.room_head(N, K)),
head.py): N heading bins, K classes with one size template each; the rooms' boxes then take their classes from range(K) and, with
N = 1, stand axis-aligned, and every loss, decode and evaluation of the run reads the net's head.  --heading-bins 1 --classes 18 is the
shape of the VoteNet paper's second benchmark.  The defaults, 12 and 10, are the reference's head.  The head is part of the
checkpoint: --resume refuses a file of another one.  Composes with every flag above."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib.util
_spec = importlib.util.spec_from_file_location("votenet_hostpin", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "votenet_amd", "hostpin.py"))
hostpin = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(hostpin)  # by path: the package's __init__ would import torch first
hostpin.pin(0)  # as bench.py: the host threads on eight cores of the GPU's NUMA node
import numpy as np, torch
from votenet_amd import evaluator as E, input_pipeline as IP, loss as VL, synth
from votenet_amd.model import VoteNetHotPath

synth_default = (synth.NH, synth.NC)
ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=600)
ap.add_argument("train_batches", nargs="?", type=int, default=16)
ap.add_argument("--save", metavar="PATH", help="write a checkpoint at every evaluation and at the end")
ap.add_argument("--resume", metavar="PATH", help="continue from this checkpoint")
ap.add_argument("--monitor", metavar="K", type=int, default=0, help="print the moving averages of the accuracies and the cost every K steps")
ap.add_argument("--guard", action="store_true", help="skip steps whose gradient is not finite (on the device); print how many were")
ap.add_argument("--height", action="store_true", help="feed the height above the floor as a point feature (point_features=1)")
ap.add_argument("--per-class", action="store_true", help="print the set-level mAP under the reference's and the paper's protocol at the end")
ap.add_argument("--min-points", metavar="K", type=int, default=0, help="drop predicted boxes that hold fewer than K points of the cloud (the paper: 5)")
ap.add_argument("--nms-overlap", choices=("rotated", "aabb3d", "bev"), default="rotated", help="the overlap of the per-class protocol's NMS (the paper: aabb3d)")
ap.add_argument("--nms-old-type", action="store_true", help="with aabb3d / bev: intersection over the later box instead of IoU (the paper's use_old_type_nms)")
ap.add_argument("--paper-votes", action="store_true", help="supervise the votes as the VoteNet paper does (one launch more behind the loss)")
ap.add_argument("--paper-proposals", action="store_true", help="supervise objectness and centre as the VoteNet paper does (one launch more behind the loss)")
ap.add_argument("--vote-fps", action="store_true", help="sample the proposal module's centres by FPS on the votes, as the VoteNet paper does (one launch in the stretch)")
ap.add_argument("--unit-votes", action="store_true", help="divide each vote's features by their L2 norm, as the authors' VoteNet does (in place of two glue launches)")
ap.add_argument("--heading-bins", metavar="N", type=int, default=synth_default[0], help="heading bins of the detection head (the reference: 12; axis-aligned boxes: 1)")
ap.add_argument("--classes", metavar="K", type=int, default=synth_default[1], help="classes (= size templates) of the detection head (the reference: 10)")
args = ap.parse_args()
if (args.nms_overlap != "rotated" or args.nms_old_type) and not args.per_class:
    ap.error("--nms-overlap / --nms-old-type need --per-class: the reference's protocol suppresses by the rotated-box IoU")
if args.nms_old_type and args.nms_overlap == "rotated":
    ap.error("--nms-old-type needs --nms-overlap aabb3d or bev")
steps, nb = args.steps, args.train_batches
dev = torch.device("cuda:0")
B, n = 8, 20480
head = synth.room_head(args.heading_bins, args.classes)  # (12, 10: the default head itself)
net = VoteNetHotPath(dev, seed=0, point_features=1 if args.height else 0, head=head)
net.init_optimizer(1e-3)
if args.resume:
    net.load(args.resume)
start = net._step
if args.monitor > 0:
    net.enable_monitors(window=100, tensors_every=10 * args.monitor)
if args.guard:
    net.enable_step_guard()  # (after the resume: its snapshot is of the restored moving averages)
if args.paper_votes:
    net.enable_vote_supervision("paper")
if args.paper_proposals:
    net.enable_proposal_supervision("paper")
if args.vote_fps:
    net.enable_proposal_sampling("vote_fps")
if args.unit_votes:
    net.enable_vote_features("unit")
print("run: vote supervision %s, proposal supervision %s, proposal sampling %s, vote features %s, head %d heading bins / %d classes (%d columns)"
      % (net.vote_supervision or "reference", net.proposal_supervision or "reference", net.proposal_sampling or "seed_fps", net.vote_features or "sum",
         head.nh, head.nc, head.width))
xs = [torch.from_numpy(synth.room_batch(B, n, 5000 + B * i, head=head)).to(dev) for i in range(nb)]
gts = [VL.gt_to_device(synth.room_gt(B, n, 5000 + B * i, head=head), dev) for i in range(nb)]
val_x = [torch.from_numpy(synth.room_batch(B, n, 90000 + B * i, head=head)).to(dev) for i in range(4)]
val_gt = [E.gt_for_eval(synth.room_gt(B, n, 90000 + B * i, head=head), head=head) for i in range(4)]


def heights(x):
    """(B, n, 1): the cloud's own rows in their order (choice = arange), camera frame already -> the points again and their height"""
    b, m = x.shape[:2]
    points, feats, _ = IP.subsample_augment_features(x.reshape(b * m, 3), np.arange(b + 1, dtype=np.int64) * m, m,
                                                     choice=torch.arange(m, dtype=torch.int32, device=dev).repeat(b, 1), depth_to_camera=False)
    assert torch.equal(points, x)
    return feats


fs = [heights(x) for x in xs] if args.height else [None] * nb
val_f = [heights(x) for x in val_x] if args.height else [None] * 4


def evaluate():
    res = {}
    for thr in (0.25, 0.5):
        aps = []
        for x, f, g in zip(val_x, val_f, val_gt):
            pred = net.predict(x, 0.25, feats=f)
            aps.append(E.eval_det(pred, g, thr, head=head)[1])
        res[thr] = float(np.nanmean(aps))
    return res


def save():
    if args.save:
        net.save(args.save)
        print("step %d: saved %s" % (net._step, args.save))


def report(step):
    """The line of every earlier log (mean of the per-batch mAPs), and beside it the reference's metric: mAP over the whole set."""
    res = E.evaluate(net, list(zip(val_x, val_f)) if args.height else val_x, val_gt, (0.25, 0.5), min_points=args.min_points)
    print("step %d: mAP" % step, evaluate(), " set mAP", {thr: res[thr]["mAP"] for thr in (0.25, 0.5)})


def guard_line(step):
    r = net.step_guard.read()  # (the one read-back of the guard)
    print("step %d  step guard: %d of %d steps skipped (%d in a row now, the last at step %d), %d restores of the moving averages"
          % (step, r["skipped"], r["seen"], r["consecutive"], r["last_skip_step"], r["ema_restores"]))


t0 = time.time()
report(start)
for i in range(start, steps):
    net.train_step(xs[i % nb], gt=gts[i % nb], next_x=xs[(i + 1) % nb], feats=fs[i % nb], next_feats=fs[(i + 1) % nb])  # geometry of the next batch under this step
    if (i + 1) % 100 == 0:
        l = net.last_losses.cpu().numpy()
        print("step %d  cost %.3f  vote %.3f obj %.3f box %.3f sem %.3f  pos %d  (%.1f s)" % (i + 1, l[0], l[1], l[2], l[9], l[8], int(l[10]),
                                                                                              time.time() - t0))
    if args.monitor > 0 and (i + 1) % args.monitor == 0:
        r = net.monitors.read()  # (the one read-back of the monitors: every K steps)
        m = r["mean"]
        print("step %d  moving averages over %d steps: obj_accuracy %.4f  sem_accuracy %.4f  total_cost %.4f  n_pos %.1f  n_neg %.1f"
              % (i + 1, r["filled"], m["obj_accuracy"], m["sem_accuracy"], m["total_cost"], m["n_pos"], m["n_neg"]))
        if (i + 1) % (10 * args.monitor) == 0 and r["tensors"]:
            by_rms = sorted(r["tensors"].items(), key=lambda kv: kv[1]["grad"]["rms"])
            for title, rows in (("smallest", by_rms[:5]), ("largest", by_rms[-5:])):
                print("step %d  %s gradient rms (of step %d; rms of the clipped gradient = rms x clip factor):" % (i + 1, title, r["tensors_step"]))
                for name, t in rows:
                    print("    %-28s grad rms %.3e  clip factor %.3e  param rms %.3e  non-finite %d" % (name, t["grad"]["rms"], t["grad"]["clip_factor"],
                                                                                                    t["param"]["rms"], t["grad"]["nonfinite"] + t["param"]["nonfinite"]))
    if args.guard and args.monitor > 0 and (i + 1) % args.monitor == 0:
        guard_line(i + 1)
    if (i + 1) % 300 == 0:
        report(i + 1)
        save()
if steps % 300 or steps <= start:  # (a run that ends on an evaluation has just saved)
    save()
if args.guard:
    guard_line(net._step)
if args.per_class:
    val = list(zip(val_x, val_f)) if args.height else val_x
    for name, proto in (("reference protocol", "reference"), ("per-class protocol", "per_class")):
        kw = dict(nms_overlap=args.nms_overlap, nms_measure="over_later" if args.nms_old_type else "iou") if proto == "per_class" else {}
        res = E.evaluate(net, val, val_gt, (0.25, 0.5), protocol=proto, min_points=args.min_points, **kw)
        if kw and args.nms_overlap != "rotated":
            name += ", NMS overlap %s / %s" % (kw["nms_overlap"], kw["nms_measure"])
        print("step %d: set mAP, %s" % (net._step, name), {thr: res[thr]["mAP"] for thr in (0.25, 0.5)})
