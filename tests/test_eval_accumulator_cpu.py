"""CPU: the host half of the streaming detection evaluation (votenet_amd/evaluator.py: finalize_records,
DetectionAccumulator.result) and the closed form the device kernel decides true positives by (csrc/eval_match.hip), against
eval_det_cls and the literal loops of tests/test_evaluator.py:ref_eval_det_cls (evaluator.py:76-161 of the reference)."""
import numpy as np
import pytest

from test_evaluator import ref_eval_det_cls

THRESHOLDS = (0.25, 0.5)


def random_class_set(rng, ndet=60, nimg=7, tie_scores=True, tie_overlaps=True):
    """One class: detections (image, score, overlap row against the image's ground truth), in arrival order."""
    gt_count = {img: int(rng.integers(0, 4)) for img in range(nimg)}
    dets = []
    for _ in range(ndet):
        img = int(rng.integers(0, nimg))
        row = (rng.random(gt_count[img]) * (rng.random() < 0.7)).astype(np.float32)
        if tie_overlaps:
            row = np.round(row * 4) / np.float32(4) + np.float32(0.01) * (row > 0)  # equal maxima: the first one must win
        score = float(np.round(rng.random(), 1)) if tie_scores else float(rng.random())
        dets.append((img, score, row.astype(np.float32)))
    return dets, gt_count


def closed_form_tp(dets, thr):
    """The kernel's rule: d is a true positive iff ovmax_d > thr and no e of the same image with jmax_e == jmax_d and
    ovmax_e > thr comes before d by (score descending, arrival ascending)."""
    n = len(dets)
    img = np.array([d[0] for d in dets])
    score = np.array([d[1] for d in dets], np.float64)
    has = np.array([len(d[2]) > 0 for d in dets])
    ovmax = np.array([d[2].max() if len(d[2]) else -np.inf for d in dets], np.float32)
    jmax = np.array([int(d[2].argmax()) if len(d[2]) else -1 for d in dets])
    q = has & (ovmax > thr)
    idx = np.arange(n)
    before = (score[None, :] > score[:, None]) | ((score[None, :] == score[:, None]) & (idx[None, :] < idx[:, None]))  # [d, e]
    same = (img[None, :] == img[:, None]) & (jmax[None, :] == jmax[:, None])
    taken = (before & same & q[None, :]).any(1)
    return q & ~taken


def pack_records(score, cls, mask, scene, arrival):
    rec = np.zeros((len(score), 4), np.int32)
    rec[:, 0] = np.asarray(score, np.float32).view(np.int32)
    rec[:, 1] = np.asarray(cls, np.int32) | (np.asarray(mask, np.int32) << 8)
    rec[:, 2] = scene
    rec[:, 3] = np.asarray(arrival, np.uint32).view(np.int32)
    return rec


@pytest.mark.parametrize("seed", range(8))
def test_closed_form_equals_the_reference_loop(seed):
    from votenet_amd import evaluator as E
    rng = np.random.default_rng(seed)
    dets, gt_count = random_class_set(rng, tie_scores=seed % 2 == 0)
    npos = sum(gt_count.values())
    order = np.argsort(-np.array([d[1] for d in dets]), kind="stable")
    for thr in THRESHOLDS:
        tp = closed_form_tp(dets, thr)[order].astype(np.float64)
        fp = 1.0 - tp
        fp, tp = np.cumsum(fp), np.cumsum(tp)
        rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        assert E.voc_ap(rec, prec) == ref_eval_det_cls(dets, None, npos, thr)
        rec2, prec2, ap2 = E.eval_det_cls([d[0] for d in dets], [d[1] for d in dets], [d[2] for d in dets], gt_count, thr)
        assert np.array_equal(rec, rec2) and np.array_equal(prec, prec2) and E.voc_ap(rec, prec) == ap2


@pytest.mark.parametrize("seed", range(5))
def test_finalize_records_equals_eval_det_cls(seed):
    """Three classes' detections interleaved in one arrival order, records shuffled in the buffer (the kernel appends scenes in
    no fixed order): rec, prec and ap per class equal eval_det_cls on that class's detections, at both thresholds from one set
    of records."""
    from votenet_amd import evaluator as E
    rng = np.random.default_rng(100 + seed)
    nc = 3
    per_class = [random_class_set(rng, ndet=int(rng.integers(20, 70))) for _ in range(nc)]
    slots = rng.permutation(np.concatenate([np.full(len(per_class[c][0]), c) for c in range(nc)]))  # class of every arrival
    pos = [np.nonzero(slots == c)[0] for c in range(nc)]
    score, cls, mask, scene, arrival = [], [], [], [], []
    for c in range(nc):
        dets = per_class[c][0]
        m = sum(closed_form_tp(dets, thr).astype(np.int32) << t for t, thr in enumerate(THRESHOLDS))
        score += [d[1] for d in dets]
        scene += [d[0] for d in dets]
        cls += [c] * len(dets)
        mask += list(m)
        arrival += list(pos[c])
    rec = pack_records(score, cls, mask, scene, arrival)
    rec = rec[rng.permutation(len(rec))]
    npos = np.array([sum(per_class[c][1].values()) for c in range(nc)] + [0])
    res = E.finalize_records(rec, npos, THRESHOLDS)
    for thr in THRESHOLDS:
        aps = []
        for c in range(nc):
            dets, gt_count = per_class[c]
            if npos[c] == 0:
                assert c not in res[thr]["ap"]
                continue
            r, p, ap = E.eval_det_cls([d[0] for d in dets], [d[1] for d in dets], [d[2] for d in dets], gt_count, thr)
            assert np.array_equal(res[thr]["rec"][c], r) and np.array_equal(res[thr]["prec"][c], p)
            assert res[thr]["ap"][c] == ap and res[thr]["npos"][c] == npos[c]
            aps.append(ap)
        assert res[thr]["mAP"] == float(np.mean(aps))
        assert nc not in res[thr]["ap"]  # a class without ground truth is absent


def host_accumulator(records, offered, flags, npos, capacity):
    """A DetectionAccumulator whose buffers are host tensors: result() only copies and finalises (the constructor insists on a
    device, the package has no CPU path for add)."""
    import torch
    from votenet_amd import evaluator as E
    acc = object.__new__(E.DetectionAccumulator)
    acc.thresholds, acc.capacity = THRESHOLDS, capacity
    acc._records = torch.from_numpy(np.ascontiguousarray(records))
    acc._state = torch.from_numpy(np.concatenate([[offered, flags], npos]).astype(np.int32))
    return acc


def test_result_raises_on_overflow_and_skips_classes_without_ground_truth():
    from votenet_amd import VotenetError, evaluator as E
    from votenet_amd.synth import NC
    npos = np.zeros(NC, np.int64)
    npos[2], npos[5] = 2, 1
    rec = pack_records([0.9, 0.8, 0.7, 0.6], [2, 2, 7, 5], [3, 1, 0, 0], [0, 0, 1, 1], [0, 1, 2, 3])
    res = host_accumulator(rec, 4, 0, npos, 4).result()
    assert sorted(res[0.25]["ap"]) == [2, 5] and sorted(res[0.5]["ap"]) == [2, 5]   # class 7: detections but no ground truth
    assert res[0.25]["ap"][2] == 1.0 and res[0.5]["ap"][2] == 0.5 and res[0.25]["ap"][5] == 0.0
    assert res[0.25]["mAP"] == 0.5 and res[0.5]["mAP"] == 0.25
    assert np.array_equal(res[0.5]["rec"][2], [0.5, 0.5]) and np.array_equal(res[0.5]["prec"][2], [1.0, 0.5])
    with pytest.raises(VotenetError, match=r"capacity 4, 9 detections offered"):
        host_accumulator(rec, 9, E.DetectionAccumulator.FLAG_OVERFLOW, npos, 4).result()
    with pytest.raises(VotenetError, match=r"capacity 4, 9 detections offered"):
        host_accumulator(rec, 9, 0, npos, 4).result()
    empty = host_accumulator(rec[:0], 0, 0, np.zeros(NC, np.int64), 4).result()
    assert empty[0.25]["ap"] == {} and np.isnan(empty[0.25]["mAP"])


def test_kernel_argument_validation(hiplib):
    """votenet_eval_match refuses what its LDS tables cannot hold before anything is launched (no GPU here)."""
    import ctypes
    thr = (ctypes.c_float * 2)(0.25, 0.5)
    p = ctypes.c_void_p(8)
    call = lambda b=1, n=4, g=4, nc=10, nthr=2, t=thr, rec=p, cap=16: hiplib.votenet_eval_match(
        b, n, g, nc, p, p, 0, None, p, p, p, p, nthr, t, 0, 0, rec, cap, p, p, p, None)
    for kw, text in ((dict(n=0), b"n >= 1"), (dict(g=4097), b"at most 4096 ground-truth rows"), (dict(nthr=9), b"1 to 8 IoU thresholds"),
                     (dict(nthr=0), b"1 to 8 IoU thresholds"), (dict(nc=257), b"number of classes"), (dict(rec=None), b"null accumulator buffer"),
                     (dict(t=None), b"null thresholds"), (dict(cap=-1), b"negative row count or capacity")):
        assert call(**kw) == 1 and text in hiplib.votenet_last_error(), (kw, hiplib.votenet_last_error())
    assert call(b=0) == 0  # an empty batch touches nothing
