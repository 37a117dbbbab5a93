"""GPU: the streaming detection evaluator (evaluator.DetectionAccumulator / evaluate over votenet_eval_match, csrc/eval_match.hip).
The yardstick is always eval_det -- the one-batch evaluator, overlaps from votenet_iou3d_cross, the reference's greedy loop on the
host (evaluator.py:76-200) -- on the CONCATENATION of everything that was added: scenes stacked along the batch axis, the kept rows
concatenated with the scene offset added.  Equality is exact (==): the overlaps come from the same device function and the
precision / recall arithmetic from the same numpy code."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.25, 0.5)
NC = 10


def concatenate(parts):
    """[(pred, gt)] as added -> one (pred, gt) for eval_det.  pred: device tensors, nms_idx the valid rows only; gt numpy."""
    off, rows = 0, []
    for pred, _ in parts:
        r = pred["nms_idx"]
        if "nms_count" in pred:
            r = r[:int(pred["nms_count"].item())]
        rows.append(r + torch.tensor([off, 0], dtype=torch.int32, device=r.device))
        off += pred["bboxes"].shape[0]
    pred = dict(bboxes=torch.cat([p["bboxes"] for p, _ in parts]), class_scores=torch.cat([p["class_scores"] for p, _ in parts]),
                nms_idx=torch.cat(rows))
    host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    gt = {k: np.concatenate([host(g[k]) for _, g in parts]) for k in ("boxes", "labels", "count")}
    return pred, gt


def eval_det_curves(pred, gt, thr):
    """eval_det (votenet_amd/evaluator.py:71-95) kept line for line, returning the rec / prec arrays eval_det drops.  The caller
    holds its ap to eval_det's own."""
    from votenet_amd import evaluator as E
    from votenet_amd import tf_nms3d
    dev = pred["bboxes"].device
    iou = tf_nms3d.iou3d_cross(pred["bboxes"], torch.from_numpy(np.ascontiguousarray(gt["boxes"], dtype=np.float32)).to(dev)).cpu().numpy()
    keep = pred["nms_idx"].cpu().numpy()
    cls_scores = pred["class_scores"].detach().cpu().numpy()
    labels, count = np.asarray(gt["labels"]), np.asarray(gt["count"])
    out = {}
    for c in range(NC):
        gt_count, gt_cols = {}, {}
        for b in range(labels.shape[0]):
            cols = np.nonzero(labels[b, :count[b]] == c)[0]
            if len(cols):
                gt_count[b], gt_cols[b] = len(cols), cols
        if not gt_count:
            continue
        d_img, d_score, d_iou = [], [], []
        for b, i in keep:
            if int(cls_scores[b, i].argmax()) != c:
                continue
            d_img.append(int(b))
            d_score.append(float(cls_scores[b, i].max()))
            d_iou.append(iou[b, i, gt_cols[b]] if b in gt_cols else np.zeros(0, np.float32))
        for b in set(d_img):
            gt_count.setdefault(b, 0)
        out[c] = E.eval_det_cls(d_img, d_score, d_iou, gt_count, thr)
    return out


def check_against_eval_det(res, parts, note=""):
    """res: DetectionAccumulator.result() after adding `parts` -> asserts equality with eval_det on the concatenation; returns
    {thr: mAP}."""
    from votenet_amd import evaluator as E
    pred, gt = concatenate(parts)
    maps = {}
    for thr in THRESHOLDS:
        ap, m = E.eval_det(pred, gt, thr)
        curves = eval_det_curves(pred, gt, thr)
        assert {c: v[2] for c, v in curves.items()} == ap  # the restated loop is eval_det
        got = res[thr]
        print("%s thr %.2f: mAP accumulator %.17g  eval_det %.17g  classes %s  detections %d" %
              (note, thr, got["mAP"], m, sorted(ap), pred["nms_idx"].shape[0]))
        assert sorted(got["ap"]) == sorted(ap), (sorted(got["ap"]), sorted(ap))
        for c in ap:
            assert np.array_equal(got["rec"][c], curves[c][0]), (thr, c)
            assert np.array_equal(got["prec"][c], curves[c][1]), (thr, c)
            assert got["ap"][c] == ap[c], (thr, c, got["ap"][c], ap[c])
        assert got["mAP"] == m or (np.isnan(m) and np.isnan(got["mAP"])), (thr, got["mAP"], m)
        maps[thr] = m
    return maps


def random_scenes(rng, dev, B=8, N=256, G=64, round_scores=False, count=None, no_rows=(), repeat_padding=False):
    """Ground truth: count[s] random boxes in a room, the rest of the G rows garbage (or the last box repeated).  Predictions: two
    thirds jittered copies of ground-truth boxes (several claim the same box, most with the box's class on top), the rest random.
    Kept rows: a random subset of every scene's boxes, shuffled across the batch."""
    from votenet_amd import evaluator as E
    mk = lambda c, s, h: E.box_corners(c, s, h)
    count = np.asarray(count if count is not None else rng.integers(1, G + 1, B))
    g_c, g_s, g_h = rng.random((B, G, 3)) * [5, 1, 5], rng.random((B, G, 3)) * 0.8 + 0.3, rng.random((B, G)) * 6.28
    labels = rng.integers(0, NC, (B, G)).astype(np.int32)
    if repeat_padding:
        for s in range(B):
            if count[s]:
                last = count[s] - 1
                g_c[s, count[s]:], g_s[s, count[s]:], g_h[s, count[s]:], labels[s, count[s]:] = g_c[s, last], g_s[s, last], g_h[s, last], labels[s, last]
    p_c, p_s, p_h = rng.random((B, N, 3)) * [5, 1, 5], rng.random((B, N, 3)) * 0.8 + 0.3, rng.random((B, N)) * 6.28
    cls = rng.normal(size=(B, N, NC)).astype(np.float32)
    for s in range(B):
        if not count[s]:
            continue
        src = rng.integers(0, count[s], N)
        near = rng.random(N) < 0.67
        p_c[s, near] = g_c[s, src[near]] + rng.normal(size=(int(near.sum()), 3)) * 0.05
        p_s[s, near] = g_s[s, src[near]] * (1 + rng.normal(size=(int(near.sum()), 3)) * 0.08)
        p_h[s, near] = g_h[s, src[near]] + rng.normal(size=int(near.sum())) * 0.05
        right = near & (rng.random(N) < 0.8)
        cls[s, right, labels[s, src[right]]] += 2.5
    if round_scores:
        cls = np.round(cls, 1).astype(np.float32)
    rows = np.array([[s, i] for s in range(B) if s not in no_rows for i in np.nonzero(rng.random(N) < 0.6)[0]], np.int32).reshape(-1, 2)
    rows = rows[rng.permutation(len(rows))]
    pred = dict(bboxes=torch.from_numpy(mk(p_c, p_s, p_h)).to(dev), class_scores=torch.from_numpy(cls).to(dev), nms_idx=torch.from_numpy(rows).to(dev))
    return pred, dict(boxes=mk(g_c, g_s, g_h), labels=labels, count=count)


def split(pred, gt, chunks):
    """The scenes of (pred, gt) as len(chunks) batches; chunk = consecutive scene numbers.  Kept rows keep their relative order."""
    parts = []
    rows = pred["nms_idx"].cpu().numpy()
    for ch in chunks:
        lo, hi = ch[0], ch[-1] + 1
        r = rows[(rows[:, 0] >= lo) & (rows[:, 0] < hi)] - np.array([lo, 0], np.int32)
        p = dict(bboxes=pred["bboxes"][lo:hi].contiguous(), class_scores=pred["class_scores"][lo:hi].contiguous(),
                 nms_idx=torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32)).to(pred["bboxes"].device))
        parts.append((p, {k: v[lo:hi] for k, v in gt.items()}))
    return parts


def accumulate(dev, parts, **kw):
    from votenet_amd import evaluator as E
    acc = E.DetectionAccumulator(dev, THRESHOLDS, **kw)
    for p, g in parts:
        acc.add(p, g)
    return acc


@pytest.mark.parametrize("nsplit", [1, 2, 5])
def test_random_scenes_equal_eval_det_on_the_concatenation(hiplib, dev, nsplit):
    rng = np.random.default_rng(7)
    pred, gt = random_scenes(rng, dev)
    assert gt["count"].min() < gt["count"].max()  # ragged
    parts = split(pred, gt, np.array_split(np.arange(8), nsplit))
    acc = accumulate(dev, parts, capacity=8 * 256)
    maps = check_against_eval_det(acc.result(), parts, "random scenes, %d add calls:" % nsplit)
    assert 0.0 < maps[0.5] and maps[0.25] < 1.0  # the case has matches and misses at both thresholds
    # reset() starts a new set on the same buffers
    acc.reset()
    acc.add(*parts[0])
    check_against_eval_det(acc.result(), parts[:1], "after reset:")


def test_ties_empty_scenes_empty_add_and_repeated_padding(hiplib, dev):
    """Scores rounded to one decimal (ties inside and across scenes), scene 5 without ground truth, scene 3 without a kept row and
    alone in its add call (row count 0), padding rows that repeat the last box (gt_for_eval's layout)."""
    rng = np.random.default_rng(11)
    count = rng.integers(1, 65, 8)
    count[5] = 0
    pred, gt = random_scenes(rng, dev, round_scores=True, count=count, no_rows=(3,), repeat_padding=True)
    sc = pred["class_scores"].cpu().numpy().max(-1)
    assert len(np.unique(sc)) < 100  # 2048 boxes on fewer than 100 scores: many ties
    parts = split(pred, gt, [[0, 1, 2], [3], [4, 5, 6, 7]])
    assert parts[1][0]["nms_idx"].shape[0] == 0
    res = accumulate(dev, parts, capacity=8 * 256).result()
    check_against_eval_det(res, parts, "ties / empty scenes:")
    # the padding is not counted: npos is the number of valid rows per class
    for c, n in res[0.25]["npos"].items():
        assert n == sum(int((gt["labels"][s, :count[s]] == c).sum()) for s in range(8))


def test_a_scene_fills_a_round_of_kept_rows_and_another_has_one_row_in_the_next(hiplib, dev):
    """257 kept rows: scene 1's 256 fill the first round of 256 rows the workgroups read, scene 0's single row is listed last, alone
    in the second round; three ground-truth rows per scene."""
    rng = np.random.default_rng(13)
    pred, gt = random_scenes(rng, dev, B=2, N=256, G=3, count=[3, 3])
    rows = np.array([[1, i] for i in range(256)] + [[0, 200]], np.int32)
    pred["nms_idx"] = torch.from_numpy(rows).to(dev)
    parts = [(pred, gt)]
    acc = accumulate(dev, parts, capacity=257)
    maps = check_against_eval_det(acc.result(), parts, "257 rows, 256 + 1:")
    assert int(acc._state[0]) == 257 and maps[0.25] > 0.0


def test_overlaps_are_bit_equal_to_iou3d_cross(hiplib, dev):
    """Thresholds one ulp either side of a detection's largest overlap (taken from votenet_iou3d_cross) flip its true-positive bit
    exactly there: the kernel's ovmax is that table's value, bit for bit.  One detection per scene, so nothing is ever taken."""
    from votenet_amd import evaluator as E
    from votenet_amd import tf_nms3d
    rng = np.random.default_rng(5)
    pred, gt = random_scenes(rng, dev, B=8, N=64, G=16, count=np.full(8, 16))
    iou = tf_nms3d.iou3d_cross(pred["bboxes"], torch.from_numpy(gt["boxes"]).to(dev)).cpu().numpy()
    cls = pred["class_scores"].cpu().numpy().argmax(-1)
    checked = 0
    for s in range(8):
        for i in range(64):
            cols = np.nonzero(gt["labels"][s] == cls[s, i])[0]
            if not len(cols) or not iou[s, i, cols].max() > 0.05:
                continue
            ovmax = np.float32(iou[s, i, cols].max())
            thr = (float(np.nextafter(ovmax, np.float32(0))), float(ovmax))
            p = dict(pred, nms_idx=torch.tensor([[s, i]], dtype=torch.int32, device=dev))
            acc = E.DetectionAccumulator(dev, thr, capacity=4)
            acc.add(p, gt)
            res = acc.result()
            assert res[thr[0]]["rec"][cls[s, i]][-1] > 0 and res[thr[1]]["rec"][cls[s, i]][-1] == 0, (s, i, ovmax)
            checked += 1
            break
    assert checked >= 6


def test_perfect_and_shifted_detections_over_two_add_calls(hiplib, dev):
    """tests/test_evaluator.py:test_eval_det_perfect_and_shifted_detections, the four scenes split over two add calls."""
    from votenet_amd import evaluator as E
    from votenet_amd import synth
    gt = E.gt_for_eval(synth.room_gt(4, 2048, 40))
    B, G = gt["labels"].shape
    cls = np.zeros((B, G, 10), np.float32)
    cls[np.arange(B)[:, None], np.arange(G)[None], gt["labels"]] = 5.0
    keep = np.array([[b, i] for b in range(B) for i in range(gt["count"][b])], np.int32)
    near = (gt["boxes"] + np.array([0.02, 0.01, -0.02], np.float32)).astype(np.float32)
    pred = dict(bboxes=torch.from_numpy(near).to(dev), nms_idx=torch.from_numpy(keep).to(dev), class_scores=torch.from_numpy(cls).to(dev))
    parts = split(pred, gt, [[0, 1], [2, 3]])
    res = accumulate(dev, parts, capacity=B * G).result()
    for thr in THRESHOLDS:
        assert res[thr]["mAP"] == 1.0 and all(v == 1.0 for v in res[thr]["ap"].values()) and res[thr]["ap"]
    c0 = int(gt["labels"][0, 0])
    moved = near.copy()
    moved[gt["labels"] == c0] += 10.0
    pred["bboxes"] = torch.from_numpy(moved).to(dev)
    parts = split(pred, gt, [[0, 1], [2, 3]])
    res2 = accumulate(dev, parts, capacity=B * G).result()
    for thr in THRESHOLDS:
        assert res2[thr]["ap"][c0] == 0.0 and all(v == 1.0 for k, v in res2[thr]["ap"].items() if k != c0) and res2[thr]["mAP"] < 1.0
    check_against_eval_det(res2, parts, "shifted class:")


def test_set_level_map_is_not_the_mean_of_batch_maps(hiplib, dev):
    """Batch 0: one class-0 box found exactly, score 5.  Batch 1: the same, and a false positive of class 0 at
    score 9.  Per batch: AP 1.0 and 0.5 -> mean 0.75.  Over the set the false positive outranks BOTH
    true positives: precision 1/2 then 2/3, AP = 0.5 * 2/3 + 0.5 * 2/3 = 2/3.  The accumulator returns the set-level value."""
    from votenet_amd import evaluator as E
    centre = np.array([[[1.0, 0.5, 1.0], [4.0, 0.5, 4.0]]])
    size, head = np.full((1, 2, 3), 0.8), np.zeros((1, 2))
    gtb = E.box_corners(centre, size, head)                                   # (1,2,8,3): box 1 is padding
    gt = dict(boxes=gtb, labels=np.zeros((1, 2), np.int32), count=np.array([1]))
    det = E.box_corners(centre + np.array([0.02, 0.01, -0.02]), size, head)  # box 0 on the ground truth, box 1 far from it
    hi, lo = np.zeros((1, 2, NC), np.float32), np.zeros((1, 2, NC), np.float32)
    hi[0, :, 0], lo[0, :, 0] = (5.0, 9.0), (5.0, 1.0)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    p0 = dict(bboxes=T(det), class_scores=T(lo), nms_idx=T(np.array([[0, 0]], np.int32)))           # batch 0: the true positive only
    p1 = dict(bboxes=T(det), class_scores=T(hi), nms_idx=T(np.array([[0, 0], [0, 1]], np.int32)))   # batch 1: true + confident false
    parts = [(p0, gt), (p1, gt)]
    per_batch = float(np.mean([E.eval_det(p, g, 0.25)[1] for p, g in parts]))
    res = accumulate(dev, parts, capacity=8).result()
    maps = check_against_eval_det(res, parts, "set-level vs per-batch:")
    print("set-level mAP@0.25 %.6f, mean of per-batch mAPs %.6f" % (res[0.25]["mAP"], per_batch))
    assert per_batch == 0.75
    assert res[0.25]["mAP"] == maps[0.25] == 0.5 * (2.0 / 3.0) + 0.5 * (2.0 / 3.0)
    assert res[0.25]["mAP"] != per_batch


def test_overflow_raises_and_nothing_is_written_beyond_capacity(hiplib, dev):
    from votenet_amd import VotenetError, evaluator as E
    rng = np.random.default_rng(3)
    pred, gt = random_scenes(rng, dev)
    offered = pred["nms_idx"].shape[0]
    cap = 300
    assert offered > cap
    buf = torch.full((cap + 4096, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=cap, records=buf)
    acc.add(pred, gt)
    with pytest.raises(VotenetError, match="capacity %d, %d detections offered" % (cap, offered)):
        acc.result()
    assert bool((buf[cap:] == 0x5A5A5A5A).all()), "the guard region behind the record buffer was written"
    assert bool((buf[:cap, 2] != 0x5A5A5A5A).any())  # ... and the buffer itself was used
    # a buffer that is exactly large enough is not an overflow
    acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=offered)
    acc.add(pred, gt)
    check_against_eval_det(acc.result(), [(pred, gt)], "capacity == offered:")


def test_add_does_not_synchronise_and_refuses_bad_rows(hiplib, dev):
    from votenet_amd import InvalidArgumentError, evaluator as E
    rng = np.random.default_rng(4)
    pred, gt = random_scenes(rng, dev, B=2, N=32, G=8)
    acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=256)
    gd = E.gt_to_device(gt, dev)
    pad = dict(pred, nms_count=torch.tensor([pred["nms_idx"].shape[0]], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any host synchronisation inside add raises
    try:
        acc.add(pad, gd)
        acc.add(pred, gd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_against_eval_det(acc.result(), [(pred, gt), (pred, gt)], "device ground truth, device count:")
    bad = dict(pred, nms_idx=torch.tensor([[0, 1], [2, 0], [0, 32]], dtype=torch.int32, device=dev))  # scene 2, box 32: outside
    acc.reset()
    acc.add(bad, gt)
    with pytest.raises(InvalidArgumentError, match="outside its batch"):
        acc.result()


STEPS, TRAIN_BATCHES, VAL_BATCHES, B, NPTS = 300, 12, 3, 8, 20480


def test_evaluate_a_trained_model_equals_eval_det_on_its_predictions(hiplib, dev):
    """The recipe of tests/test_gpu_convergence.py, 300 steps.  evaluate()'s own predictions are recorded as it makes them (the
    default mode's forward is not bit-reproducible from call to call) and concatenated for eval_det.  The same recorded
    predictions in the synchronous form (nms_idx cut to its length on the host, what predict(sync=True) returns), with numpy and
    with device ground truth, give the same records; predict(sync=True) itself is held to eval_det on its own output."""
    from votenet_amd import evaluator as E
    from votenet_amd import loss as VL
    from votenet_amd import synth
    from votenet_amd.model import VoteNetHotPath
    net = VoteNetHotPath(dev, seed=0)
    net.init_optimizer(1e-3)
    xs = [torch.from_numpy(synth.room_batch(B, NPTS, 5000 + B * i)).to(dev) for i in range(TRAIN_BATCHES)]
    gts = [VL.gt_to_device(synth.room_gt(B, NPTS, 5000 + B * i), dev) for i in range(TRAIN_BATCHES)]
    val_x = [torch.from_numpy(synth.room_batch(B, NPTS, 90000 + B * i)).to(dev) for i in range(VAL_BATCHES)]
    val_gt = [E.gt_for_eval(synth.room_gt(B, NPTS, 90000 + B * i)) for i in range(VAL_BATCHES)]
    for i in range(STEPS):
        net.train_step(xs[i % TRAIN_BATCHES], gt=gts[i % TRAIN_BATCHES], next_x=xs[(i + 1) % TRAIN_BATCHES])
    torch.cuda.synchronize()
    seen, predict = [], net.predict

    def recording_predict(*a, **kw):
        assert kw.get("sync") is False
        seen.append(predict(*a, **kw))
        return seen[-1]
    net.predict = recording_predict
    try:
        res = E.evaluate(net, val_x, val_gt, THRESHOLDS)
    finally:
        del net.predict
    assert len(seen) == VAL_BATCHES and all("nms_count" in p and p["nms_idx"].shape[0] == B * 256 for p in seen)
    parts = list(zip(seen, val_gt))
    maps = check_against_eval_det(res, parts, "evaluate(), %d steps:" % STEPS)
    per_batch = {thr: float(np.nanmean([E.eval_det(*concatenate([pg]), thr)[1] for pg in parts])) for thr in THRESHOLDS}
    print("\n".join(["streaming evaluation: %d steps, %d held-out scenes" % (STEPS, B * VAL_BATCHES)] +
                    ["  mAP@%.2f over the set %.4f   mean of per-batch mAPs %.4f" % (t, maps[t], per_batch[t]) for t in THRESHOLDS]))
    assert res[0.25]["ap"] and sum(len(v) for v in res[0.25]["rec"].values()) > 0
    # the same predictions: synchronous form, numpy / device ground truth
    as_sync = [{k: (v[:int(p["nms_count"].item())] if k == "nms_idx" else v) for k, v in p.items() if k != "nms_count"} for p in seen]
    dev_gt = [E.gt_to_device(g, dev) for g in val_gt]
    for other in (accumulate(dev, list(zip(as_sync, val_gt))), accumulate(dev, list(zip(seen, dev_gt))), accumulate(dev, list(zip(as_sync, dev_gt)))):
        r2 = other.result()
        for thr in THRESHOLDS:
            assert r2[thr]["ap"] == res[thr]["ap"] and r2[thr]["mAP"] == res[thr]["mAP"]
            assert all(np.array_equal(r2[thr]["prec"][c], res[thr]["prec"][c]) and np.array_equal(r2[thr]["rec"][c], res[thr]["rec"][c])
                       for c in res[thr]["ap"])
    # predict(sync=True) as it comes
    sync_parts = [(net.predict(x, 0.25), g) for x, g in zip(val_x, val_gt)]
    assert all("nms_count" not in p for p, _ in sync_parts)
    check_against_eval_det(accumulate(dev, sync_parts).result(), sync_parts, "predict(sync=True):")
