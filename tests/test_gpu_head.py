"""GPU: a network under another detection head (votenet_amd/head.py; the heads of tests/head_cases.py) through every layer that used
to read the default head's constants -- the last GEMM of the proposal module on its padded copy or, for a width that is a multiple of
64, on the matrix itself; the loss kernel on the tensor that GEMM leaves; decode and predict under both protocols; the replayed
stretch; the set-level evaluation; the monitors; the paper's supervision modes on ground truth from labelled points; the label
encoding -- each against the float64 / restated reference the default head's test of that layer uses, at that test's bar."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402
from head_cases import HEADS, WIDTH_PAD, head  # noqa: E402

pytestmark = pytest.mark.gpu

B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_monitors.py)
NAMES = ["total_cost", "vote_reg_loss", "obj_cls_loss", "center_loss", "heading_cls_loss", "heading_residual_loss", "size_cls_loss",
         "size_residual_loss", "sem_cls_loss", "box_loss"]
OTHERS = [n for n in sorted(HEADS) if n != "default"]


def bits(t):
    t = t.detach().contiguous().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def close(got, want, floor=1.0):
    """the bar of tests/test_gpu_loss.py: 1e-5 relative, floor 1.0 for loss values, 1e-3 for cotangents"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.abs(got - want).max() <= 1e-5 * max(floor, np.abs(want).max()))


def _net(dev, name, seed=5, **kw):
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL, head=head(name), **kw)
    net.init_optimizer(1e-3)
    return net


_batches = {}


def batch(dev, name, seed=300):
    """(x, ground truth on the device, ground truth on the host) of B rooms drawn under the head; made once per head and seed."""
    from votenet_amd import loss as VL
    from votenet_amd import synth
    if (name, seed) not in _batches:
        h = head(name)
        gt_np = synth.room_gt(B, NPTS, seed, head=h)
        _batches[name, seed] = (torch.from_numpy(synth.room_batch(B, NPTS, seed, head=h)).to(dev), VL.gt_to_device(gt_np, dev), gt_np)
    return _batches[name, seed]


# ---------------------------------------------------------------- the default head, given or not
def test_default_head_given_explicitly_is_the_implicit_one_bit_for_bit(hiplib, dev):
    """The bit-reproducible mode (mlp.set_deterministic, as test_training_gradients_are_bit_reproducible sets it up).  Two networks from
    one seed, one with head=HeadConfig.sunrgbd(): forward outputs, the loss vector, every parameter after one train_step, and predict's
    boxes / scores / nms_idx carry the same bits."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    from votenet_amd.head import HeadConfig
    x, gt, _ = batch(dev, "default", 77)
    prev = M.set_deterministic(True)
    try:
        res = []
        for kw in ({}, dict(head=HeadConfig.sunrgbd())):
            net = VM.VoteNetHotPath(dev, seed=11, npoints=SMALL, **kw)
            out = {k: v.clone() for k, v in net.forward(x).items()}
            net.train_step(x, gt=gt)
            pred = net.predict(x)
            torch.cuda.synchronize()
            res.append((out, net.last_losses.clone(), net.store.flat.clone(), {k: pred[k].clone() for k in ("bboxes", "scores", "nms_idx", "class_scores")}))
    finally:
        M.set_deterministic(prev)
    (o0, l0, p0, d0), (o1, l1, p1, d1) = res
    assert set(o0) == set(o1) and all(torch.equal(bits(o0[k]), bits(o1[k])) for k in o0)
    assert torch.isfinite(l0[1]) and torch.equal(bits(l0), bits(l1))
    assert torch.equal(bits(p0), bits(p1))
    assert d0["nms_idx"].shape[0] > 0 and all(torch.equal(bits(d0[k]), bits(d1[k])) for k in d0)


# ---------------------------------------------------------------- forward and backward, every head, every GEMM form
@pytest.mark.parametrize("name", OTHERS)
def test_full_backward_vs_autograd_under_each_head(hiplib, dev, gemm_form, name, monkeypatch):
    """test_gpu_backward._full_backward_vs_autograd itself -- forward against float64 (proposals_output < 5e-5), every gradient tensor
    against float64 autograd (worst < 1e-4, median < 2e-5) -- with the network it builds given the head: the last layer of mlp2 runs
    padded to 64 / 128 / 192 columns, or unpadded at 64 / 128, and its cotangent is head.width wide."""
    import test_gpu_backward as TB
    from votenet_amd import model as VM
    made = []

    class WithHead(VM.VoteNetHotPath):
        def __init__(self, *a, **kw):
            super().__init__(*a, head=head(name), **kw)
            made.append(self)
    monkeypatch.setattr(VM, "VoteNetHotPath", WithHead)
    worst, tape = TB._full_backward_vs_autograd(dev, 2048, SMALL, 5)
    net, = made
    width, pad = WIDTH_PAD[name]
    last = tape[7]["recs2"][-1]
    assert net.head.width == width and net.proposal.mlp2[-1].cout_pad == pad and bool(last.get("padded")) == bool(pad)
    assert "proposal/conv_post_2/W" in worst and "proposal/conv_post_2/b" in worst and len(worst) > 60


# ---------------------------------------------------------------- the loss kernel on what the net leaves
def _loss_case(dev, name):
    """A forward pass of a fresh net under the head and ground truth whose first three boxes of every scene sit 5 cm beside a proposal
    (so positives exist whatever the random network votes for); for `tiny`, box 0 of scene 1 carries class 5 >= nc = 3."""
    x, _, gt_np = batch(dev, name)
    net = _net(dev, name)
    out = net.forward(x)
    gt_np = {k: v.copy() for k, v in gt_np.items()}
    pxyz = out["proposals_xyz"].cpu().numpy()
    for s in range(B):
        for j in range(3):
            gt_np["bboxes_xyz"][s, j] = pxyz[s, 40 * j + 1] + np.float32(0.05)
    if name == "tiny":
        gt_np["semantic_labels"][1, 0] = gt_np["size_labels"][1, 0] = 5
    return net, out, gt_np


@pytest.mark.parametrize("name", sorted(HEADS))
def test_loss_kernel_under_each_head(hiplib, dev, name):
    """votenet_loss on proposals_output as the proposal module leaves it -- a pitched view of the padded GEMM's result, or the contiguous
    tensor for exact64 / exact128 -- against tests/loss_ref.votenet_loss(nh, ns, nc) in float64 and its autograd, at test_gpu_loss.py's
    bars (1e-5 relative, floors 1.0 and 1e-3).  tiny: a box of class 5 >= nc gives NaN exactly where the reference has NaN (the class
    blocks loss_ref.label_blocks names), everything else finite at the same bars."""
    from votenet_amd import loss as VL
    net, out, gt_np = _loss_case(dev, name)
    h = net.head
    pout = out["proposals_output"]
    width, pad = WIDTH_PAD[name]
    assert tuple(pout.shape) == (B, 256, width) and pout.is_contiguous() == (pad == 0) and pout.stride(1) == (pad or width)
    losses, cot = VL.votenet_loss(out, VL.gt_to_device(gt_np, dev), head=h)
    l2, _ = VL.votenet_loss(out, VL.gt_to_device(gt_np, dev), nh=h.nh, ns=h.ns, nc=h.nc)  # the keywords still work
    assert torch.equal(bits(losses), bits(l2))
    got = dict(zip(NAMES + ["n_pos", "n_neg"], losses.cpu().tolist()))
    T = lambda a: torch.from_numpy(a).double() if a.dtype == np.float32 else torch.from_numpy(a)
    D = lambda t: t.detach().cpu().double()
    v, p, w = (D(out[k]).clone().requires_grad_(True) for k in ("votes_xyz", "proposals_xyz", "proposals_output"))
    r = loss_ref.votenet_loss(D(out["seeds_xyz"]), v, p, w, {k: T(a) for k, a in gt_np.items()}, nh=h.nh, ns=h.ns, nc=h.nc)
    r["total_cost"].backward()
    print("head %s losses %s" % (name, got))
    assert int(got["n_pos"]) == r["n_pos"] >= 3 * B and int(got["n_neg"]) == r["n_neg"] > 0
    nan_terms = [k for k in NAMES if np.isnan(float(r[k].detach()))]
    assert nan_terms == (["total_cost", "size_cls_loss", "sem_cls_loss", "box_loss"] if name == "tiny" else [])
    for k in NAMES:
        want = float(r[k].detach())
        if np.isnan(want):
            assert np.isnan(got[k]), (k, got[k])
        else:
            assert abs(got[k] - want) <= 1e-5 * max(1.0, abs(want)), (k, got[k], want)
    for key, ref in (("votes_xyz", v.grad), ("proposals_xyz", p.grad), ("proposals_output", w.grad)):
        g = cot[key].double().cpu()
        assert cot[key].is_contiguous() and g.shape == ref.shape
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(g), nan), key
        err = float((g[~nan] - ref[~nan]).abs().max()) / max(1e-3, float(ref[~nan].abs().max()))
        print("head %s %s error %.2e NaN entries %d" % (name, key, err, int(nan.sum())))
        assert err <= 1e-5, (key, err)
    if name == "tiny":
        # the rows of the mislabelled box's positives: NaN over the size-class and semantic-class blocks, the valid residual slot untouched
        mine = (r["positive"][1] & (r["bboxes_assignment"][1] == 0)).numpy()
        size_cols, _ = loss_ref.label_blocks("size_labels", 0, h.nh, h.ns, h.nc)
        sem_cols, _ = loss_ref.label_blocks("semantic_labels", 0, h.nh, h.ns, h.nc)
        d = cot["proposals_output"].cpu().numpy()
        assert mine.sum() >= 1 and np.isnan(d[1][np.ix_(mine, list(size_cols) + list(sem_cols))]).all()
        rest = np.ones(d.shape, bool)
        rest[1][np.ix_(mine, list(size_cols) + list(sem_cols))] = False
        assert not np.isnan(d[rest]).any() and not (d[1][mine][:, h.size_res] != 0).any()


# ---------------------------------------------------------------- decode and predict
@pytest.mark.parametrize("name", ["scannet", "wide"])
def test_decode_under_the_head_vs_oracle(hiplib, dev, name):
    """votenet_decode_boxes with the head's bins and templates against oracle.oracle_loss.decode_boxes, at test_gpu_loss.py's bar for it
    (1e-5 of the largest coordinate; the scores equal): on a draw whose heading residuals fall below 0 and above 2 nh (both sides of
    floormod; with one bin the angle is floormod(res * pi, 2 pi)) and whose size residuals reach the 1e-6 floor, and on the network's own
    output, through VoteNetHotPath.decode_boxes (the templates uploaded once per net)."""
    from oracle import oracle_loss
    from votenet_amd import loss as VL
    h = head(name)
    rng = np.random.default_rng(11)
    prop = (rng.random((3, 50, 3)) * 4).astype(np.float32)
    out = rng.normal(0, 1.5, (3, 50, h.width)).astype(np.float32)
    out[0, 0, h.size_res] = -5.0
    if h.nh == 1:
        out[0, 1:6, h.heading_res] = np.array([-0.5, 2.0, 2.5, -30.0, 0.0], np.float32)[:, None]
    boxes, scores = VL.decode_boxes(torch.from_numpy(prop).to(dev), torch.from_numpy(out).to(dev), head=h)
    eb, es = oracle_loss.decode_boxes(prop, out, h.mean_sizes_f32, nh=h.nh, ns=h.ns, nc=h.nc)
    assert np.abs(boxes.cpu().numpy() - eb).max() <= 1e-5 * max(1.0, np.abs(eb).max())
    assert (scores.cpu().numpy() == es).all()
    x, _, _ = batch(dev, name)
    net = _net(dev, name)
    o = net.forward(x)
    nb, ns_ = net.decode_boxes(o["proposals_xyz"], o["proposals_output"])
    table = net._mean_sizes_dev
    nb2, _ = net.decode_boxes(o["proposals_xyz"], o["proposals_output"])
    assert net._mean_sizes_dev is table and np.array_equal(table.cpu().numpy(), h.mean_sizes_f32) and torch.equal(bits(nb), bits(nb2))
    eb, es = oracle_loss.decode_boxes(o["proposals_xyz"].cpu().numpy(), o["proposals_output"].cpu().numpy(), h.mean_sizes_f32, nh=h.nh, ns=h.ns,
                                      nc=h.nc)
    assert np.abs(nb.cpu().numpy() - eb).max() <= 1e-5 * max(1.0, np.abs(eb).max()) and (ns_.cpu().numpy() == es).all()


@pytest.mark.parametrize("name", ["scannet", "wide"])
def test_predict_under_the_head_both_protocols(hiplib, dev, name):
    """predict in the reference protocol: class_scores are the head's last nc columns, the boxes the oracle's decode with the head's
    templates, nms_idx NMS3D's on those boxes.  predict(protocol="per_class", min_points=5, nms_overlap="aabb3d"): the rows are
    detections_ref.class_nms3d's over aabb_nms_ref's table, with nc from the head, on the gated objectness."""
    import aabb_nms_ref as A
    import detections_ref as R
    from oracle import oracle_loss
    from votenet_amd import aabb_nms, box_points, tf_nms3d
    from votenet_amd import detections as D
    h = head(name)
    x, gt, _ = batch(dev, name)
    net = _net(dev, name)
    for _ in range(3):
        net.train_step(x, gt=gt)
    pred = net.predict(x)
    pout = pred["proposals_output"]
    assert tuple(pred["class_scores"].shape) == (B, 256, h.nc) and torch.equal(bits(pred["class_scores"]), bits(pout[..., -h.nc:]))
    eb, es = oracle_loss.decode_boxes(pred["proposals_xyz"].cpu().numpy(), pout.cpu().numpy(), h.mean_sizes_f32, nh=h.nh, ns=h.ns, nc=h.nc)
    assert np.abs(pred["bboxes"].cpu().numpy() - eb).max() <= 1e-5 * max(1.0, np.abs(eb).max()) and (pred["scores"].cpu().numpy() == es).all()
    keep = tf_nms3d.NMS3D(pred["bboxes"], pred["scores"], pout[..., :2].contiguous(), 0.25)
    assert pred["nms_idx"].shape[0] > 0 and torch.equal(pred["nms_idx"], keep)
    if h.nh == 1:  # axis-aligned boxes: every decoded heading is floormod(res * pi, 2 pi) of one bin
        assert torch.isfinite(pred["bboxes"]).all()
    # the paper's protocol
    per = net.predict(x, protocol="per_class", min_points=5, nms_overlap="aabb3d")
    assert tuple(per["det_rows"].shape) == (B * 256 * h.nc, 4) and tuple(per["class_scores"].shape) == (B, 256, h.nc)
    gated = box_points.gate_objectness(per["proposals_output"][..., :2].contiguous(), per["point_counts"], 5)
    boxes = per["bboxes"].cpu().numpy()
    table = aabb_nms.overlap_matrix(per["bboxes"], "aabb3d", "iou").cpu().numpy()
    exp_table = A.overlap_table(boxes, "aabb3d", "iou")
    assert np.array_equal(table, exp_table, equal_nan=True)
    p = D.protocol_params("per_class", 0.25)
    exp = R.class_nms3d(exp_table, gated.cpu().numpy(), per["class_scores"].cpu().numpy(), p["iou_threshold"], p["conf_thresh"],
                        class_nms=p["class_nms"], per_class=p["per_class"])
    scene, box, klass, score, offset = D.rows_to_host(per)
    print("head %s: %d kept boxes (reference protocol), %d per-class rows, classes seen %d" % (name, keep.shape[0], len(scene), len(set(klass.tolist()))))
    assert np.array_equal(offset, exp["det_offset"]) and np.array_equal(np.stack([scene, box, klass], 1), exp["rows"])
    assert np.allclose(score, exp["score"], rtol=1e-5, atol=2.0 ** -126, equal_nan=True)
    assert len(scene) > 0 and klass.max() < h.nc and (h.nc <= 10 or klass.max() >= 10)  # classes beyond the default head's ten occur


# ---------------------------------------------------------------- the replayed stretch
@pytest.mark.parametrize("name", ["scannet", "exact128"])
def test_stretch_graph_replays_are_the_launch_by_launch_step_under_the_head(hiplib, dev, monkeypatch, name):
    """test_gpu_model.test_stretch_graph_replays_are_the_launch_by_launch_step under the head, its assertions kept: two replicas on the
    same batches, the graph replica taking the launch replica's state before every step; forward results, losses and moving averages
    bit-equal, gradient buckets equal to the run-to-run spread of the atomics (1e-4 of the largest entry), and the graph replica really
    replayed.  (The bit-reproducible mode never replays a graph -- model._stretch_eligible -- so, as there, the default mode.)"""
    from votenet_amd import model as VM
    xs, gts = zip(*[batch(dev, name, 90 + i)[:2] for i in range(2)])
    ref, got = _net(dev, name), _net(dev, name)
    for net in (ref, got):
        net._ema_state()
    steps = 5
    for i in range(steps):
        got.store.flat.copy_(ref.store.flat)
        got.store.params_changed()
        got._m.copy_(ref._m), got._v.copy_(ref._v), got._ema_flat.copy_(ref._ema_flat)
        res = []
        for net, flag in ((ref, False), (got, True)):
            monkeypatch.setattr(VM, "STRETCH_GRAPH", flag)
            out = net.train_step(xs[i % 2], gt=gts[i % 2], next_x=xs[(i + 1) % 2])
            torch.cuda.synchronize()
            res.append(({k: v.clone() for k, v in out.items()}, net.last_losses.clone(), net.store.grad.clone(), net._ema_flat.clone()))
        (o0, l0, g0, e0), (o1, l1, g1, e1) = res
        assert tuple(o1["proposals_output"].shape) == (B, 256, head(name).width)
        for k in o0:
            assert torch.equal(o0[k], o1[k]), (i, k)
        nn = lambda t: torch.nan_to_num(t, nan=-12345.0)
        assert torch.equal(nn(l0), nn(l1)), (i, l0.tolist(), l1.tolist())
        assert torch.equal(e0, e1), i
        assert float((g0 - g1).abs().max()) <= 1e-4 * float(g0.abs().max()), i
    assert not ref.__dict__.get("_stretch_graphs") and len(got._stretch_graphs) == 1
    assert sum(g.replays for g in got._stretch_graphs.values()) == steps - 1


# ---------------------------------------------------------------- evaluation
def test_evaluate_under_the_scannet_head_equals_eval_det(hiplib, dev):
    """evaluator.evaluate over two batches against eval_det(head=) on the host over the same predictions: AP per class and mAP equal to
    1e-12 (test_gpu_eval_accumulator.py compares them for equality).  The ground truth is made from the network's own kept boxes, so
    true and false positives both occur, over classes beyond the default head's ten; one box carries class 20 >= 18 and is counted
    nowhere.  DetectionAccumulator(num_class=18) over the same predictions gives evaluate's result."""
    from test_gpu_eval_accumulator import concatenate
    from votenet_amd import InvalidArgumentError
    from votenet_amd import evaluator as E
    h = head("scannet")
    net = _net(dev, "scannet")
    xs = [batch(dev, "scannet", 90 + i)[0] for i in range(2)]
    for i in range(3):
        net.train_step(xs[i % 2], gt=batch(dev, "scannet", 90 + i % 2)[1])
    gts = []
    for x in xs:  # inference-mode BatchNorm: a scene's outputs are reproducible from call to call
        pred = net.predict(x)
        keep, cls = pred["nms_idx"].cpu().numpy(), pred["class_scores"].argmax(-1).cpu().numpy()
        boxes = pred["bboxes"].cpu().numpy()
        g_boxes, g_labels = np.zeros((B, 8, 8, 3), np.float32), np.zeros((B, 8), np.int32)
        for s in range(B):
            kept = keep[keep[:, 0] == s][:3, 1].tolist()  # (a network of three steps keeps few boxes: its objectness gate)
            assert len(kept) >= 2
            mine = (kept + [i for i in range(256) if i not in kept])[:8]
            g_boxes[s], g_labels[s] = boxes[s, mine], cls[s, mine]
            g_labels[s, 1] = (g_labels[s, 1] + 1) % 18   # a wrong class: its detection is a false positive
            g_labels[s, 4] = 11 + s                      # classes the default head does not have
            g_labels[s, 6] = 20                          # beyond the head: counted nowhere
            g_labels[s, 7] = 17
        gts.append(dict(boxes=g_boxes, labels=g_labels, count=np.array([7, 8][:B], np.int32)))
    seen, predict = [], net.predict

    def recording_predict(*a, **kw):
        seen.append(predict(*a, **kw))
        return seen[-1]
    net.predict = recording_predict
    try:
        res = E.evaluate(net, xs, gts, (0.25, 0.5))
    finally:
        del net.predict
    pred, gt = concatenate(list(zip(seen, gts)))
    acc = E.DetectionAccumulator(dev, (0.25, 0.5), num_class=18)
    for p, g in zip(seen, gts):
        acc.add(p, g)
    direct = acc.result()
    for thr in (0.25, 0.5):
        ap, m = E.eval_det(pred, gt, thr, head=h)
        got = res[thr]
        print("thr %.2f: mAP evaluate %.17g eval_det %.17g classes %s npos %s" % (thr, got["mAP"], m, sorted(ap), got["npos"]))
        assert sorted(got["ap"]) == sorted(ap) and len(ap) >= 3 and max(ap) < 18
        assert all(abs(got["ap"][c] - ap[c]) <= 1e-12 for c in ap) and abs(got["mAP"] - m) <= 1e-12
        assert direct[thr]["ap"] == got["ap"] and direct[thr]["mAP"] == got["mAP"]
        labels = np.concatenate([g["labels"][s, :g["count"][s]] for g in gts for s in range(B)])
        assert sum(got["npos"].values()) == int((labels < 18).sum()) < len(labels)  # class 20 is in no count
        assert 0.0 < m < 1.0 or thr == 0.5
    with pytest.raises(InvalidArgumentError):  # the default head's accumulator refuses 18-column class scores
        E.DetectionAccumulator(dev, (0.25,)).add(seen[0], gts[0])


# ---------------------------------------------------------------- monitors
def test_monitors_under_the_scannet_head(hiplib, dev):
    """enable_monitors: the step's accuracies and counts against monitors_ref.accuracies(nh=1, ns=18, nc=18) on the step's own forward
    results, compared as test_gpu_monitors.py compares them (counts equal, accuracies the rounded float64 quotients)."""
    import monitors_ref as MR
    from test_gpu_monitors import _check_against_reference
    x, gt, gt_np = batch(dev, "scannet")
    net = _net(dev, "scannet")
    mon = net.enable_monitors(window=4)
    for _ in range(2):  # the first step of a shape runs launch by launch, the second is captured
        out = net.train_step(x, gt=gt)
        torch.cuda.synchronize()
        want = MR.accuracies(out["proposals_xyz"].cpu().numpy(), out["proposals_output"].cpu().numpy(), gt_np, nh=1, ns=18, nc=18)
        _check_against_reference(net.last_accuracies, mon.counts, want)
        l = net.last_losses.cpu().numpy()
        assert [want["n_pos"], want["n_neg"]] == [int(l[10]), int(l[11])] and want["n_neg"] > 0


# ---------------------------------------------------------------- the supervision modes on ground truth from labelled points
def test_supervision_modes_under_the_scannet_head(hiplib, dev):
    """Ground truth from build_batch_from_labels(head=, point_box=True): 18 classes, one heading bin.  One train_step with
    enable_instance_votes() and enable_proposal_supervision("paper"), in the bit-reproducible mode: the step's loss vector is
    votenet_loss(head=) with the two launches behind it on the step's own forward results, bit for bit; columns 0..4 of the
    proposals_output cotangent and losses[2], losses[3] match tests/proposal_supervision_ref.py at the bars of its GPU test (centre
    columns bit for bit, objectness columns rtol 1e-5, the values 1e-5 relative), losses[1] matches tests/instance_votes_ref.py, and
    columns 5.. are the plain loss's, bit for bit."""
    import instance_votes_ref as IR
    import proposal_supervision_ref as PR
    from votenet_amd import input_pipeline as IP
    from votenet_amd import instance_votes as IV
    from votenet_amd import loss as VL
    from votenet_amd import mlp as M
    from votenet_amd import proposal_supervision as PS
    from votenet_amd import synth
    h = head("scannet")
    scenes, inst, sem = [], [], []
    for i in range(B):
        pts = synth.room_scene(NPTS, 600 + i, head=h)[0]
        scenes.append(np.stack([pts[:, 0], pts[:, 2], -pts[:, 1]], 1))  # upright-depth rows of the camera-frame room
        a, c = synth.room_scene_labels(NPTS, 600 + i, head=h)
        inst.append(a), sem.append(c)
    raw, off = IP.pack_ragged(scenes, dev)
    choice = np.tile(np.arange(NPTS, dtype=np.int32), (B, 1))
    x, gt, index = IP.build_batch_from_labels(raw, off, np.concatenate(inst), np.concatenate(sem), np.arange(18, dtype=np.int32), choice,
                                              n_out=NPTS, head=h, point_box=True)
    assert index.tolist() == list(range(B))
    labels = gt["semantic_labels"].cpu().numpy()
    assert labels.max() >= 10 and labels.max() < 18 and (gt["heading_labels"] == 0).all() and (gt["heading_residuals"] == 0).all()
    assert torch.equal(gt["size_labels"], gt["semantic_labels"])
    # a class map into the default head's ten classes drops the others: the head is what lets them through
    _, gt10, _ = IP.build_batch_from_labels(raw, off, np.concatenate(inst), np.concatenate(sem), np.arange(18, dtype=np.int32), choice, n_out=NPTS)
    assert gt10["semantic_labels"].max() < 10
    prev = M.set_deterministic(True)
    try:
        net = _net(dev, "scannet", seed=9)
        net.enable_instance_votes()
        net.enable_proposal_supervision("paper")
        out = {k: v.clone() for k, v in net.train_step(x, gt=gt).items()}
        torch.cuda.synchronize()
        l_on = net.last_losses.cpu().numpy()
        idx1, idx2 = net._seed_levels[:2]
        ref, cot = VL.votenet_loss(out, gt, head=h)
        ref_cot = {k: v.clone() for k, v in cot.items()}
        paper = ref.clone()
        IV.instance_vote_loss(out, gt, paper, (idx1, idx2), d_votes=cot["votes_xyz"])
        PS.paper_proposal_loss(out, gt, paper, d_xyz=cot["proposals_xyz"], d_out=cot["proposals_output"], head=h)
        torch.cuda.synchronize()
    finally:
        M.set_deterministic(prev)
    l_ref, l_paper = ref.cpu().numpy(), paper.cpu().numpy()
    assert np.array_equal(l_paper.view(np.int32), l_on.view(np.int32))
    a = PR.loss(out["proposals_xyz"].cpu().numpy(), out["proposals_output"].cpu().numpy(), gt["bboxes_xyz"].cpu().numpy(), losses=l_ref)
    v = IR.loss(idx1.cpu().numpy(), idx2.cpu().numpy(), gt["point_box"].cpu().numpy(), out["votes_xyz"].cpu().numpy(), gt["bboxes_xyz"].cpu().numpy())
    print("Np Nn G", a["Np"], a["Nn"], a["G"], "obj", l_ref[2], l_on[2], a["obj"], "center", l_ref[3], l_on[3], a["center"], "vote", l_ref[1],
          l_on[1], v["L"], "P", v["P"])
    assert a["Np"] == l_ref[10] and a["Nn"] == l_ref[11] > 0 and v["P"] > 0
    assert close(l_on[2], a["obj"]) and close(l_on[3], a["center"]) and close(l_on[1], v["L"])
    with_votes = l_ref.copy()
    with_votes[1] = l_on[1]
    assert np.array_equal(l_on, PR.reform(with_votes, l_on[2], l_on[3]), equal_nan=True)
    d_out = cot["proposals_output"]
    assert tuple(d_out.shape) == (B, 256, 97)
    assert torch.equal(bits(d_out[..., 2:5]), bits(a["d_ctr"])) and torch.equal(bits(cot["proposals_xyz"]), bits(a["d_ctr"]))
    assert np.allclose(d_out[..., :2].cpu().numpy(), a["d_obj"], rtol=1e-5, atol=1e-8)
    assert torch.equal(bits(d_out[..., 5:]), bits(ref_cot["proposals_output"][..., 5:]))
    assert not torch.equal(bits(d_out[..., :5]), bits(ref_cot["proposals_output"][..., :5]))
    assert torch.equal(bits(cot["votes_xyz"]), bits(v["d_votes"]))


# ---------------------------------------------------------------- the label encoding
@pytest.mark.parametrize("name", ["scannet", "tiny"])
def test_label_encoding_under_the_head(hiplib, dev, name):
    """augment_boxes with the head's templates and bins (what build_batch(head=) passes) against synth.angle2class(angle, nh) and
    (size - T[c]) / T[c] in float64 rounded once to float32: equal, test_gpu_input.py's bar for the encoder (test_boxes_bit_exact)."""
    from votenet_amd import input_pipeline as IP
    from votenet_amd import synth
    h = head(name)
    T = h.mean_sizes_f64
    rng = np.random.default_rng(h.nc)
    cnt = [5, 1, 8]
    cen = [rng.normal(size=(c, 3)) * 2 for c in cnt]
    siz = [np.abs(rng.normal(size=(c, 3))) + 0.3 for c in cnt]
    hed = [rng.uniform(-2 * np.pi, 2 * np.pi, c) for c in cnt]
    hed[0][0] = 0.0
    cls = [rng.integers(0, h.nc, c).astype(np.int32) for c in cnt]
    cls[2][:h.nc] = np.arange(min(h.nc, 8))
    dc, off = IP.pack_ragged(cen, dev)
    ds, dh, dk = (IP.pack_ragged(a, dev)[0] for a in (siz, hed, cls))
    got = {k: v.cpu().numpy() for k, v in IP.augment_boxes(dc, ds, dh, dk, off, None, **IP._head_kw(h)).items()}
    assert got["bboxes_xyz"].shape == (3, 8, 3)
    for s, c in enumerate(cnt):
        for j in range(8):
            i = min(j, c - 1)  # padding repeats the last box
            hc, hr = synth.angle2class(hed[s][i], h.nh)
            k = cls[s][i]
            assert got["heading_labels"][s, j] == hc and got["heading_residuals"][s, j] == np.float32(hr / (np.pi / h.nh))
            assert got["size_labels"][s, j] == got["semantic_labels"][s, j] == k
            assert np.array_equal(got["size_residuals"][s, j], ((siz[s][i] - T[k]) / T[k]).astype(np.float32))
            assert np.array_equal(got["bboxes_lwh"][s, j], siz[s][i].astype(np.float32))
    if h.nh == 1:
        assert (got["heading_labels"] == 0).all() and np.abs(got["heading_residuals"]).max() <= 1.0 + 1e-6


def test_build_batch_under_the_scannet_head(hiplib, dev, golden):
    """build_batch(head=) on the recorded scenes: the boxes select_boxes keeps, encoded with the head's one bin and 18 templates."""
    from test_gpu_select_boxes import fixture_objects, ragged_rows
    from votenet_amd import input_pipeline as IP
    from votenet_amd import synth
    h = head("scannet")
    T = h.mean_sizes_f64
    g = golden("select_boxes")
    b, n_out = int(g["b"]), int(g["n_out"])
    raw, off = ragged_rows([g["raw64_%d" % s] for s in range(b)], dev)
    choice = np.stack([g["choice_%d" % s] for s in range(b)])
    calib, objects = (g["Rtilt"], g["K"]), fixture_objects(g)
    points, gt, index = IP.build_batch(raw, off, calib, objects, None, choice, n_out=n_out, head=h)
    p0, gt0, index0 = IP.build_batch(raw, off, calib, objects, None, choice, n_out=n_out)
    assert torch.equal(points, p0) and index.tolist() == index0.tolist()
    for k in ("bboxes_xyz", "bboxes_lwh", "bboxes_roty", "semantic_labels", "size_labels"):
        assert torch.equal(gt[k], gt0[k]), k
    assert not torch.equal(gt["heading_residuals"], gt0["heading_residuals"]) and (gt["heading_labels"] == 0).all()
    sel = IP.select_boxes(raw, off, calib, objects, n_out, choice)
    size, heading, cls = (sel[k].cpu().numpy() for k in ("size", "heading", "cls"))
    cnt = np.diff(sel["box_offset"])
    row = 0
    for s_out, s in enumerate(index):
        start = int(sel["box_offset"][s])
        for j in range(cnt[s]):
            i = start + j
            hc, hr = synth.angle2class(heading[i], 1)
            assert hc == 0 and gt["heading_residuals"][s_out, j].item() == np.float32(hr / np.pi)
            assert np.array_equal(gt["size_residuals"][s_out, j].cpu().numpy(), ((size[i] - T[cls[i]]) / T[cls[i]]).astype(np.float32))
            row += 1
    assert row == int(cnt[index].sum()) > 0
