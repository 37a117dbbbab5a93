"""GPU: per-class detections (libvotenet_detect.so: votenet_class_nms3d, votenet_eval_match_rows; votenet_amd/detections.py, the
`protocol` of VoteNetHotPath.predict / evaluator.evaluate) against the numpy restatement of include/votenet_detections.h
(tests/detections_ref.py) fed the DEVICE's own overlap tables (votenet_iou3d_matrix / votenet_iou3d_cross): decisions are compared
exactly, scores to 1e-5 relative of their float64 evaluation (the project's bar for sums; only expf differs between the two)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_ref as R  # noqa: E402

import cases  # noqa: E402  (tests/golden, on the path by conftest.py)

pytestmark = pytest.mark.gpu

NC = 10
THRESHOLDS = (0.25, 0.5)
COMBOS = [(cn, pc, c) for cn in (True, False) for pc in (True, False) for c in (0.0, 0.05, 0.5)]
TINY = 2.0 ** -126  # below fp32's smallest normal number a product has no 1e-5 relative precision to hold it to


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def clear_of(table, thr):
    with np.errstate(invalid="ignore"):
        return not (np.abs(table - np.float32(thr)) < 1e-5).any()


def draw_boxes(O, b, n, seed, thr, room=None):
    """Boxes as the NMS tests draw them (cases.nms_random); the seed is redrawn, here on the CPU, until no entry of the oracle's
    table lies within 1e-5 of the threshold (an overlap within rounding of it could fall either side)."""
    room = room or (2.0 if n < 32 else 6.0 if n == 256 else 4.0)
    for k in range(50):
        c = cases.nms_random(b=b, n=n, seed=seed + 1000 * k, room=room)
        if all(clear_of(O.iou3d_matrix(c["bboxes"][s]), thr) for s in range(b)):
            return c["bboxes"]
    raise AssertionError("no seed found")


def device_table(boxes, dev, thr):
    from votenet_amd import tf_nms3d
    iou = tf_nms3d.iou3d_matrix(T(boxes, dev)).cpu().numpy()
    assert clear_of(iou, thr)  # a condition on the inputs, not a tolerance on the result
    return iou


def check(boxes, obj, cls, dev, thr, combos, iou=None):
    """class_nms3d on the device == the restatement over the device's table, for every (class_nms, per_class, conf_thresh) given."""
    from votenet_amd import detections as D
    iou = device_table(boxes, dev, thr) if iou is None else iou
    bb, ob, cs = T(boxes, dev), T(obj, dev), T(cls, dev)
    b, n, nc = cls.shape
    kept_any = 0
    for cn, pc, c in combos:
        det = D.class_nms3d(bb, ob, cs, thr, c, class_nms=cn, per_class=pc)
        assert tuple(det["det_rows"].shape) == (b * n * (nc if pc else 1), 4) and det["det_rows"].dtype == torch.int32
        assert tuple(det["det_offset"].shape) == (b + 1,) and det["det_offset"].dtype == torch.int32
        scene, box, klass, score, offset = D.rows_to_host(det)
        exp = R.class_nms3d(iou, obj, cls, thr, c, class_nms=cn, per_class=pc)
        assert np.array_equal(offset, exp["det_offset"]), (cn, pc, c, offset, exp["det_offset"])
        assert np.array_equal(np.stack([scene, box, klass], 1), exp["rows"]), (cn, pc, c)
        assert score.dtype == np.float32
        err = np.abs(score.astype(np.float64) - exp["score"]) / np.maximum(np.abs(exp["score"]), TINY)
        print("class_nms %d per_class %d conf %.2f: %d rows, largest relative score error %.3g"
              % (cn, pc, c, len(score), np.nanmax(err) if len(err) and not np.isnan(err).all() else 0.0))
        assert np.allclose(score, exp["score"], rtol=1e-5, atol=TINY, equal_nan=True), (cn, pc, c)
        kept_any += len(score)
    return kept_any


@pytest.mark.parametrize("b,n,nc", [(1, 1, 1), (2, 63, 10), (3, 64, 10), (2, 65, 3), (2, 130, 10), (8, 256, 10), (1, 512, 2)])
def test_class_nms3d_equals_the_restatement_over_the_device_table(hiplib, dev, O, b, n, nc):
    """63 / 64 / 65: either side of one mask word; 130: two word boundaries; 512: the limit; 8 x 256 x 10: the model's shape."""
    thr = 0.25
    boxes = draw_boxes(O, b, n, 7 * n + b, thr)
    rng = np.random.default_rng(n)
    obj = rng.normal(size=(b, n, 2)).astype(np.float32) * 2
    cls = rng.normal(size=(b, n, nc)).astype(np.float32) * 2
    iou = device_table(boxes, dev, thr)
    assert check(boxes, obj, cls, dev, thr, COMBOS, iou) > 0
    if n > 1:  # the class rule and the suppression both did something
        a = R.class_nms3d(iou, obj, cls, thr, 0.0, class_nms=True, per_class=False)["det_offset"][-1]
        c = R.class_nms3d(iou, obj, cls, thr, 0.0, class_nms=False, per_class=False)["det_offset"][-1]
        cand = int((R.margins(obj) > -np.inf).sum())
        assert c < cand and (nc == 1 or c < a <= cand), (c, a, cand)


def test_adversarial_scenes(hiplib, dev, O):
    """Scene 0: no candidate.  1: the first box removes every other.  2: every box in one class.  3: tied margins.  4: NaN
    objectness, NaN class logits (some of a row, a whole row).  5: plain."""
    b, n, nc, thr = 6, 70, 4, 0.25
    rng = np.random.default_rng(5)
    for k in range(50):
        boxes = cases.nms_random(b=b, n=n, seed=77 + 1000 * k, room=3.0)["bboxes"]
        prng = np.random.default_rng(k)
        for i in range(n):  # scene 1: one box, nudged
            boxes[1, i] = cases.corner_box(1.0, 1.2, 0.9, 0.3, (prng.normal() * 0.015, prng.normal() * 0.015, prng.normal() * 0.015)).astype(np.float32)
        if all(clear_of(O.iou3d_matrix(boxes[s]), thr) for s in range(b)):
            break
    else:
        raise AssertionError("no seed found")
    obj = rng.normal(size=(b, n, 2)).astype(np.float32) * 2
    cls = rng.normal(size=(b, n, nc)).astype(np.float32)
    obj[0] = np.array([9.0, 0.0], np.float32)  # d = -9: below every threshold but 0
    cls[1, :, 1] += 20.0
    cls[2, :, 3] += 20.0
    obj[3] = np.round(obj[3], 0)
    obj[4, ::7, 0] = np.nan
    obj[4, 3] = np.array([np.inf, np.inf], np.float32)
    cls[4, 1::5, 2] = np.nan
    cls[4, 2::9] = np.nan
    iou = device_table(boxes, dev, thr)
    assert iou[1][~np.eye(n, dtype=bool)].min() > 0.5
    d = R.margins(obj)
    assert len(np.unique(d[3])) < n // 3 and np.isnan(d[4]).sum() >= 10
    combos = [(cn, pc, c) for cn in (True, False) for pc in (True, False) for c in (0.05, 0.0)]
    check(boxes, obj, cls, dev, thr, combos, iou)
    exp = R.class_nms3d(iou, obj, cls, thr, 0.05, class_nms=True, per_class=False)
    assert exp["kept"][0] == [] and exp["kept"][1] == [int(np.argmax(d[1]))]
    assert len(exp["kept"][2]) == len(R.class_nms3d(iou, obj, cls, thr, 0.05, class_nms=False, per_class=False)["kept"][2])
    assert not any(np.isnan(d[4, i]) for i in exp["kept"][4]) and any(np.isnan(cls[4, i]).all() for i in exp["kept"][4])
    assert len(R.class_nms3d(iou, obj, cls, thr, 0.0, class_nms=True, per_class=False)["kept"][0]) > 0  # conf 0 keeps d = -9


@pytest.mark.parametrize("b,n", [(3, 64), (2, 130)])
def test_class_agnostic_mode_keeps_what_the_shipped_nms_keeps(hiplib, dev, O, b, n):
    """class_nms off, per_class off, conf_thresh 0.5, scores := o1 - o0: per scene, the kept sequence of tf_nms3d.NMS3D, exactly."""
    from votenet_amd import detections as D
    from votenet_amd import tf_nms3d
    thr = 0.25
    boxes = draw_boxes(O, b, n, 3 * n + b, thr)
    device_table(boxes, dev, thr)
    rng = np.random.default_rng(n + 1)
    obj = rng.normal(size=(b, n, 2)).astype(np.float32)
    obj[0, :8] = np.round(obj[0, :8], 0)  # some ties
    cls = rng.normal(size=(b, n, NC)).astype(np.float32)
    d = R.margins(obj)
    keep = tf_nms3d.NMS3D(T(boxes, dev), T(d, dev), T(obj, dev), thr).cpu().numpy()
    scene, box, klass, score, offset = D.rows_to_host(D.class_nms3d(T(boxes, dev), T(obj, dev), T(cls, dev), thr, 0.5, class_nms=False, per_class=False))
    assert 0 < len(keep) < int((d > 0).sum()) and offset[-1] == len(keep)
    for s in range(b):
        assert box[offset[s]:offset[s + 1]].tolist() == keep[keep[:, 0] == s][:, 1].tolist(), s
        assert (scene[offset[s]:offset[s + 1]] == s).all()
    assert np.array_equal(klass, cls[scene, box].argmax(-1))


def test_two_runs_write_the_same_bytes(hiplib, dev):
    from votenet_amd import detections as D
    c = cases.nms_random(b=8, n=256, seed=33, room=6.0)
    rng = np.random.default_rng(0)
    bb, ob = T(c["bboxes"], dev), T(c["objectiveness"] * 2, dev)
    cs = T(rng.normal(size=(8, 256, NC)).astype(np.float32), dev)
    a, b2 = D.class_nms3d(bb, ob, cs), D.class_nms3d(bb, ob, cs)
    total = int(a["det_offset"][-1])
    assert total > 0 and torch.equal(a["det_offset"], b2["det_offset"]) and torch.equal(a["det_rows"][:total], b2["det_rows"][:total])


def test_invalid_arguments_raise_with_the_limit_and_launch_nothing(hiplib, dev):
    from votenet_amd import InvalidArgumentError, VotenetError, _lib as L, detections as D
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(InvalidArgumentError, match="at most 512 boxes per scene, got n = 513"):
        D.class_nms3d(z(1, 513, 8, 3), z(1, 513, 2), z(1, 513, NC))
    with pytest.raises(InvalidArgumentError, match=r"classes must be in \[1, 64\], got 65"):
        D.class_nms3d(z(1, 16, 8, 3), z(1, 16, 2), z(1, 16, 65))
    for thr in (1.5, -0.25):
        with pytest.raises(InvalidArgumentError, match=r"iou_threshold must be in \[0, 1\]"):
            D.class_nms3d(z(1, 16, 8, 3), z(1, 16, 2), z(1, 16, NC), thr)
    with pytest.raises(InvalidArgumentError, match=r"conf_thresh must be in \[0, 1\)"):
        D.class_nms3d(z(1, 16, 8, 3), z(1, 16, 2), z(1, 16, NC), 0.25, 1.0)
    lib = L.side_lib("detect")
    need = lib.votenet_class_nms3d_workspace_bytes(2, 16, NC)
    rows = torch.full((2 * 16 * NC, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    off = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    bb, ob, cs = z(2, 16, 8, 3), z(2, 16, 2) + torch.tensor([0.0, 1.0], device=dev), z(2, 16, NC)
    call = lambda n, nc, thr, wsb: lib.votenet_class_nms3d(2, n, nc, L.ptr(bb), L.ptr(ob), L.ptr(cs), thr, 0.0, 1, 1, L.ptr(rows), 2 * 16 * NC,
                                                           L.ptr(off), L.ptr(ws), wsb, L.stream_ptr())
    with pytest.raises(VotenetError, match="workspace of %d bytes required" % need):
        L.check(call(16, NC, 0.25, need - 1), side="detect")
    assert call(513, NC, 0.25, need) == 1 and call(16, 65, 0.25, need) == 1 and call(16, NC, 1.5, need) == 1
    torch.cuda.synchronize()
    assert bool((off == 0x5A5A5A5A).all()) and bool((rows == 0x5A5A5A5A).all())  # nothing ran
    L.check(call(16, NC, 0.25, need), side="detect")  # ... and the same call with its workspace does
    assert off.cpu().tolist() == [0, 16 * NC, 32 * NC]  # boxes without volume: nothing removes anything


# ------------------------------------------------------------------ the matcher
def match_case(O, rng_seed, B=3, N=256, G=16):
    """Ground truth in classes 0..5 only; scene 1 without ground truth; padding rows that are garbage.  Detections: two thirds nudged
    copies of ground-truth boxes (several claim one box).  The seed is redrawn until the oracle's detection x ground-truth table
    stays clear of both thresholds."""
    from votenet_amd import evaluator as E
    for k in range(50):
        rng = np.random.default_rng(rng_seed + 1000 * k)
        mk = lambda n: E.box_corners(rng.random((B, n, 3)) * [5, 1, 5], rng.random((B, n, 3)) * 0.8 + 0.3, rng.random((B, n)) * 6.28)
        gtb, det = mk(G), mk(N)
        count = np.array([G - 3, 0, G // 2][:B], np.int32)
        labels = rng.integers(0, 6, (B, G)).astype(np.int32)
        src = np.zeros((B, N), np.int64)
        for s in range(B):
            if count[s]:
                src[s] = rng.integers(0, count[s], N)
                near = rng.random(N) < 0.67
                det[s, near] = gtb[s, src[s, near]] + (rng.normal(size=(int(near.sum()), 1, 3)) * 0.04).astype(np.float32)
        table = [O.iou3d_matrix(np.concatenate([det[s], gtb[s]]))[:N, N:] for s in range(B)]
        if all(clear_of(t, thr) for t in table for thr in THRESHOLDS):
            return det, gtb, labels, count, rng
    raise AssertionError("no seed found")


def cross_table(det, gtb, dev):
    from votenet_amd import tf_nms3d
    table = tf_nms3d.iou3d_cross(T(det, dev), T(gtb, dev)).cpu().numpy()
    assert all(clear_of(table, thr) for thr in THRESHOLDS)
    return table


def rows_tensor(scene, box, klass, score, dev, pad=0):
    rows = np.stack([scene, box, klass, np.asarray(score, np.float32).view(np.int32)], 1).astype(np.int32)
    rows = np.concatenate([rows, np.full((pad, 4), 0x5A5A5A5A, np.int32)])
    return T(rows, dev)


def records_of(acc):
    """the accumulator's records in arrival order: (score, class, tp_mask, scene, arrival), npos"""
    state = acc._state.cpu().numpy()
    rec = acc._records[:int(state[0])].cpu().numpy()
    rec = rec[np.argsort(rec[:, 3].view(np.uint32), kind="stable")]
    return rec[:, 0].copy().view(np.float32), rec[:, 1] & 0xff, (rec[:, 1] >> 8) & 0xff, rec[:, 2], rec[:, 3].view(np.uint32), state[2:]


def test_match_rows_equals_the_restated_evaluation(hiplib, dev, O):
    """Scene 0 offers all 256 x 10 = 2560 rows (beyond the 1024 rows of votenet_eval_match), integer scores (ties), ground truth in
    six of ten classes; scene 1 has no ground truth; scene 2 a random subset of rows, not grouped by class."""
    from votenet_amd import evaluator as E
    det, gtb, labels, count, rng = match_case(O, 21)
    B, N, G = 3, 256, 16
    table = cross_table(det, gtb, dev)
    scene = np.concatenate([np.zeros(N * NC, np.int32), np.ones(40, np.int32), np.full(700, 2, np.int32)])
    pick1, pick2 = rng.permutation(N * NC)[:40], rng.permutation(N * NC)[:700]
    box = np.concatenate([np.repeat(np.arange(N), NC), pick1 // NC, pick2 // NC]).astype(np.int32)
    klass = np.concatenate([np.tile(np.arange(NC), N), pick1 % NC, pick2 % NC]).astype(np.int32)
    score = rng.integers(-5, 40, len(scene)).astype(np.float32)
    offset = np.array([0, N * NC, N * NC + 40, N * NC + 740], np.int32)
    pred = dict(bboxes=T(det, dev), det_rows=rows_tensor(scene, box, klass, score, dev, pad=100), det_offset=T(offset, dev))
    gt = dict(boxes=gtb, labels=labels, count=count)
    acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=2 * len(scene))
    gt_dev = E.gt_to_device(gt, dev)  # (the upload from pageable memory synchronises: before the mode is switched on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # add() must not synchronise
    try:
        acc.add(pred, gt_dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = acc.result()
    exp = {thr: R.eval_rows(scene, box, klass, score, table, labels, count, NC, thr) for thr in THRESHOLDS}
    rscore, rcls, rmask, rscene, rarr, npos = records_of(acc)
    assert len(rscore) == len(scene) and np.array_equal(rarr, np.arange(len(scene)))
    assert np.array_equal(rscore, score) and np.array_equal(rcls, klass) and np.array_equal(rscene, scene)
    for t, thr in enumerate(THRESHOLDS):
        assert np.array_equal((rmask >> t) & 1, exp[thr]["tp"].astype(np.int64)), thr
        assert np.array_equal(npos, exp[thr]["npos"])
        assert sorted(res[thr]["ap"]) == sorted(exp[thr]["ap"]) == sorted(set(labels[0, :count[0]]) | set(labels[2, :count[2]]))
        for c in exp[thr]["ap"]:
            assert abs(res[thr]["ap"][c] - exp[thr]["ap"][c]) <= 1e-12 and not np.isnan(res[thr]["ap"][c])
        print("thr %.2f: %d true positives of %d rows, mAP %.4f" % (thr, int(exp[thr]["tp"].sum()), len(scene), res[thr]["mAP"]))
    assert 10 < exp[0.5]["tp"].sum() <= npos.sum() and npos[6:].sum() == 0
    passing = 0  # rows that pass 0.5 on a box of their class: more than there are true positives -- several rows claimed one box
    for r in range(len(scene)):
        cols = np.nonzero(labels[scene[r], :count[scene[r]]] == klass[r])[0]
        passing += bool(len(cols) and table[scene[r], box[r], cols].max() > 0.5)
    assert passing > exp[0.5]["tp"].sum()
    # a second add continues the scene and arrival numbers
    acc.add(pred, gt)
    r2 = records_of(acc)
    k = len(scene)
    assert len(r2[0]) == 2 * k and np.array_equal(r2[3][k:], scene + B) and np.array_equal(r2[4][k:], np.arange(k) + k + 100)
    assert np.array_equal(r2[2][k:], rmask) and np.array_equal(r2[5], 2 * npos)
    both = R.eval_rows(np.concatenate([scene, scene + B]), np.tile(box, 2), np.tile(klass, 2), np.tile(score, 2),
                       np.concatenate([table, table]), np.concatenate([labels, labels]), np.tile(count, 2), NC, 0.25)
    res2 = acc.result()
    assert all(abs(res2[0.25]["ap"][c] - both["ap"][c]) <= 1e-12 for c in both["ap"])


def test_match_rows_of_one_class_cross_the_rounds_of_a_scene(hiplib, dev, O):
    """b = 2, n = 257, two classes, every box a row of either class: each (scene, class) workgroup reads its scene's 514 rows in
    rounds of 256 and keeps 128, 128 and 1 of them -- 257, past one round's worth of slots.  Through the entry itself (the
    accumulator's launches have ten classes), against the restated evaluation."""
    from votenet_amd import _lib as L, evaluator as E
    B, N, G, nc = 2, 257, 16, 2
    det, gtb, labels, count, rng = match_case(O, 23, B=B, N=N, G=G)
    labels = (labels % nc).astype(np.int32)
    count = np.array([G - 3, G // 2], np.int32)
    table = cross_table(det, gtb, dev)
    scene = np.repeat(np.arange(B), N * nc).astype(np.int32)
    box = np.tile(np.repeat(np.arange(N), nc), B).astype(np.int32)
    klass = np.tile(np.arange(nc), B * N).astype(np.int32)
    score = rng.integers(-5, 40, len(scene)).astype(np.float32)
    K = len(scene)
    bb, rows, offset = T(det, dev), rows_tensor(scene, box, klass, score, dev), T(np.array([0, N * nc, 2 * N * nc], np.int32), dev)
    g = E.gt_to_device(dict(boxes=gtb, labels=labels, count=count), dev)
    records = torch.zeros((K, 4), dtype=torch.int32, device=dev)
    state = torch.zeros(2 + nc, dtype=torch.int32, device=dev)  # [records offered, flags, npos[nc]], the accumulator's layout
    thr = (ctypes.c_float * len(THRESHOLDS))(*THRESHOLDS)
    L.check(L.side_lib("detect").votenet_eval_match_rows(
        B, N, G, nc, L.ptr(bb), L.ptr(rows), K, L.ptr(offset), L.ptr(g["boxes"]), L.ptr(g["labels"]), L.ptr(g["count"]), len(THRESHOLDS),
        thr, 0, 0, L.ptr(records), K, state.data_ptr(), state.data_ptr() + 8, state.data_ptr() + 4, L.stream_ptr()), side="detect")
    state = state.cpu().numpy()
    assert state[0] == K and state[1] == 0
    rec = records.cpu().numpy()
    rec = rec[np.argsort(rec[:, 3].view(np.uint32), kind="stable")]  # arrival order: the order of the rows
    assert np.array_equal(rec[:, 3].view(np.uint32), np.arange(K)) and np.array_equal(rec[:, 0].copy().view(np.float32), score)
    assert np.array_equal(rec[:, 1] & 0xff, klass) and np.array_equal(rec[:, 2], scene)
    for t, thr_t in enumerate(THRESHOLDS):
        exp = R.eval_rows(scene, box, klass, score, table, labels, count, nc, thr_t)
        assert np.array_equal((rec[:, 1] >> (8 + t)) & 1, exp["tp"].astype(np.int64)), thr_t
        assert np.array_equal(state[2:], exp["npos"])
        print("thr %.2f: %d true positives of %d rows" % (thr_t, int(exp["tp"].sum()), K))
        assert 0 < exp["tp"].sum() < K


def test_match_rows_flags_bad_rows_and_overflow(hiplib, dev, O):
    from votenet_amd import InvalidArgumentError, VotenetError, evaluator as E
    det, gtb, labels, count, rng = match_case(O, 22, B=2, N=32, G=8)
    gt = dict(boxes=gtb, labels=labels, count=count)
    scene = np.repeat(np.arange(2), 32).astype(np.int32)
    box = np.tile(np.arange(32), 2).astype(np.int32)
    klass = rng.integers(0, NC, 64).astype(np.int32)
    score = rng.integers(0, 9, 64).astype(np.float32)
    offset = T(np.array([0, 32, 64], np.int32), dev)
    good = dict(bboxes=T(det, dev), det_rows=rows_tensor(scene, box, klass, score, dev), det_offset=offset)
    acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=63)
    acc.add(good, gt)
    with pytest.raises(VotenetError, match="capacity 63, 64 detections offered"):
        acc.result()
    acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=64)
    acc.add(good, gt)
    assert len(records_of(acc)[0]) == 64 and acc.result()
    for col, value in ((0, 1), (0, -1), (1, 32), (1, -1), (2, NC), (2, -3)):  # the wrong scene, a box / a class outside
        bad = np.stack([scene, box, klass], 1)
        bad[5, col] = value
        acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=64)
        acc.add(dict(good, det_rows=rows_tensor(bad[:, 0], bad[:, 1], bad[:, 2], score, dev)), gt)
        with pytest.raises(InvalidArgumentError, match="outside its batch"):
            acc.result()
        assert int(acc._state[0]) == 63  # the bad row is skipped, the others are matched
    for off in ([0, 40, 32], [0, 32, 65], [-1, 32, 64]):  # offsets that do not ascend inside the buffer
        acc = E.DetectionAccumulator(dev, THRESHOLDS, capacity=64)
        acc.add(dict(good, det_offset=T(np.array(off, np.int32), dev)), gt)
        with pytest.raises(InvalidArgumentError, match="outside its batch"):
            acc.result()


# ------------------------------------------------------------------ the whole path
NPTS = 20480


@pytest.fixture(scope="module")
def net(hiplib, dev):
    """A VoteNet after a few training steps on synthetic rooms: its proposals are spread over the classes."""
    from votenet_amd import loss as VL
    from votenet_amd import synth
    from votenet_amd.model import VoteNetHotPath
    net = VoteNetHotPath(dev, seed=0)
    net.init_optimizer(1e-3)
    x = torch.from_numpy(synth.room_batch(2, NPTS, 5000)).to(dev)
    gt = VL.gt_to_device(synth.room_gt(2, NPTS, 5000), dev)
    for _ in range(20):
        net.train_step(x, gt=gt)
    torch.cuda.synchronize()
    return net


def test_predict_per_class_is_class_nms3d_on_its_own_boxes(net, dev):
    from votenet_amd import detections as D
    from votenet_amd import synth
    x = torch.from_numpy(synth.room_batch(2, NPTS, 90000)).to(dev)
    pred = net.predict(x, batch_statistics=True, protocol="per_class")
    assert "nms_idx" not in pred and "nms_count" not in pred and pred["det_rows"].is_cuda and pred["det_offset"].is_cuda
    obj, cls = pred["proposals_output"][..., :2].contiguous(), pred["proposals_output"][..., -NC:].contiguous()
    assert torch.equal(cls, pred["class_scores"])
    for proto, kw in (("per_class", {}), (dict(conf_thresh=0.0, per_class=False), dict(conf_thresh=0.0, per_class=False))):
        if kw:
            pred = net.predict(x, batch_statistics=True, protocol=proto)
        own = D.class_nms3d(pred["bboxes"], pred["proposals_output"][..., :2].contiguous(), pred["class_scores"], **kw)
        total = int(own["det_offset"][-1])
        assert total > 0 and torch.equal(own["det_offset"], pred["det_offset"]) and torch.equal(own["det_rows"][:total], pred["det_rows"][:total])
        assert pred["det_rows"].shape[0] == 2 * 256 * (1 if kw else NC)
    with pytest.raises(ValueError, match="protocol"):
        net.predict(x, batch_statistics=True, protocol="paper")


def test_predict_without_protocol_is_what_it_was(net, dev):
    from votenet_amd import synth
    from votenet_amd import tf_nms3d
    x = torch.from_numpy(synth.room_batch(2, NPTS, 90002)).to(dev)
    pred = net.predict(x, batch_statistics=True)
    assert {"proposals_xyz", "proposals_output"} <= set(pred) and set(pred) - set(net.forward(x)) == {"bboxes", "scores", "nms_idx", "class_scores"}
    direct = tf_nms3d.NMS3D(pred["bboxes"], pred["scores"], pred["proposals_output"][..., :2].contiguous(), 0.25)
    assert len(direct) > 0 and torch.equal(direct, pred["nms_idx"])
    padded = net.predict(x, batch_statistics=True, sync=False)
    assert set(padded) == set(pred) | {"nms_count"}


def test_evaluate_per_class_equals_the_restated_evaluation_of_its_rows(net, dev):
    """Three batches.  evaluate()'s predictions are recorded as it makes them; the restated evaluation runs on the rows and the
    scores the device wrote (so the order is exact) and the device's own overlap table."""
    from votenet_amd import detections as D
    from votenet_amd import evaluator as E
    from votenet_amd import synth
    from votenet_amd import tf_nms3d
    val_x = [torch.from_numpy(synth.room_batch(2, NPTS, 90000 + 2 * i)).to(dev) for i in range(3)]
    val_gt = [E.gt_for_eval(synth.room_gt(2, NPTS, 90000 + 2 * i)) for i in range(3)]
    seen, predict = [], net.predict

    def recording_predict(*a, **kw):
        assert kw.get("sync") is False and kw.get("protocol") == "per_class"
        seen.append(predict(*a, batch_statistics=True, **kw))
        return seen[-1]
    net.predict = recording_predict
    try:
        res = E.evaluate(net, val_x, val_gt, THRESHOLDS, protocol="per_class")
    finally:
        del net.predict
    assert len(seen) == 3
    scene, box, klass, score, tables, labels, count = [], [], [], [], [], [], []
    for i, (p, g) in enumerate(zip(seen, val_gt)):
        s, b, k, sc, off = D.rows_to_host(p)
        assert off[-1] > 0 and p["det_rows"].shape[0] == 2 * 256 * NC
        scene.append(s + 2 * i), box.append(b), klass.append(k), score.append(sc)
        tables.append(tf_nms3d.iou3d_cross(p["bboxes"], T(g["boxes"], dev)).cpu().numpy())
        labels.append(g["labels"]), count.append(g["count"])
    G = max(t.shape[2] for t in tables)
    tables = [np.pad(t, ((0, 0), (0, 0), (0, G - t.shape[2]))) for t in tables]
    labels = [np.pad(l, ((0, 0), (0, G - l.shape[1])), constant_values=-1) for l in labels]
    args = (np.concatenate(scene), np.concatenate(box), np.concatenate(klass), np.concatenate(score), np.concatenate(tables),
            np.concatenate(labels), np.concatenate(count), NC)
    for thr in THRESHOLDS:
        exp = R.eval_rows(*args, thr)
        assert sorted(res[thr]["ap"]) == sorted(exp["ap"]) and len(exp["ap"]) > 0
        for c in exp["ap"]:
            assert not np.isnan(res[thr]["ap"][c]) and abs(res[thr]["ap"][c] - exp["ap"][c]) <= 1e-12, (thr, c)
        assert abs(res[thr]["mAP"] - exp["mAP"]) <= 1e-12
        print("per-class protocol, thr %.2f: mAP %.4f over %d rows, %d true positives" % (thr, exp["mAP"], len(args[0]), int(exp["tp"].sum())))
