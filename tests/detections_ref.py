"""Host restatement (numpy) of include/votenet_detections.h: class-wise 3D NMS over a GIVEN IoU table, the scores in float64, and
evaluator.py:76-161 over explicit (scene, box, class, score) rows and a GIVEN detection x ground-truth overlap table.  Nothing here
computes an overlap: the tables come from the oracle (CPU tests) or from the device's own votenet_iou3d_matrix / votenet_iou3d_cross
(GPU tests), so a comparison with the device is exact."""
import math

import numpy as np


def conf_logit(c):
    """T = float32(log(c) - log1p(-c)) in double; 0 -> -inf."""
    if c == 0:
        return np.float32(-np.inf)
    return np.float32(math.log(c) - math.log1p(-c))


def argmax_first(logits):
    """-> (first arg-max where a NaN never wins over a number; all NaN: 0, that maximum (NaN if all NaN))."""
    best, arg = logits[0], 0
    for c in range(1, len(logits)):
        v = logits[c]
        if v > best or (best != best and v == v):
            best, arg = v, c
    return arg, best


def margins(objectness):
    """d = o1 - o0 in fp32."""
    o = np.asarray(objectness, np.float32)
    with np.errstate(invalid="ignore"):
        return (o[..., 1] - o[..., 0]).astype(np.float32)


def visit_order(d, T):
    """candidates (d > T; never a NaN) of one scene by d descending, equal d by ascending index."""
    cand = [i for i in range(len(d)) if d[i] > T]
    return sorted(cand, key=lambda i: (-float(d[i]), i))


def greedy(iou, order, cls, thr, class_nms):
    """iou[later][earlier] of one scene; a candidate falls iff an earlier KEPT one (of its class) overlaps it by more than thr."""
    kept, cls = [], np.asarray(cls)
    for j in order:
        k = np.asarray(kept, np.int64)
        with np.errstate(invalid="ignore"):
            hit = iou[j, k] > thr  # strict; a NaN overlap is no hit
        if class_nms:
            hit &= cls[k] == cls[j]
        if not hit.any():
            kept.append(j)
    return kept


def scores64(d, logits):
    """-> (p_obj, p_c (NC,)) by the header's formulas, evaluated in float64 on the fp32 inputs."""
    with np.errstate(all="ignore"):
        p_obj = 1.0 / (1.0 + np.exp(-np.float64(d)))
        m = np.float64(argmax_first(logits)[1])
        e = np.exp(np.asarray(logits, np.float64) - m)
        s = 0.0
        for v in e:  # class order
            s += v
        return p_obj, e / s


def class_nms3d(iou, objectness, class_scores, iou_threshold=0.25, conf_thresh=0.05, class_nms=True, per_class=True, d=None):
    """iou (B,N,N) with iou[s][later][earlier], objectness (B,N,2), class_scores (B,N,NC) ->
    dict(rows (K,3) int32 {scene, box, class}, score (K,) float64, det_offset (B+1,) int32, kept [per scene: boxes in visit order]).
    d: the margins, if the caller formed them already."""
    class_scores = np.asarray(class_scores, np.float32)
    B, N, NC = class_scores.shape
    d = margins(objectness) if d is None else np.asarray(d, np.float32)
    T, thr = conf_logit(conf_thresh), np.float32(iou_threshold)
    rows, score, offset, kept_all = [], [], [0], []
    for s in range(B):
        cls = [argmax_first(class_scores[s, i])[0] for i in range(N)]
        kept = greedy(iou[s], visit_order(d[s], T), cls, thr, class_nms)
        kept_all.append(kept)
        for i in kept:
            p_obj, p_c = scores64(d[s, i], class_scores[s, i])
            if per_class:
                for c in range(NC):
                    rows.append((s, i, c))
                    score.append(p_obj * p_c[c])
            else:
                rows.append((s, i, cls[i]))
                score.append(p_obj)
        offset.append(len(rows))
    return dict(rows=np.array(rows, np.int32).reshape(-1, 3), score=np.array(score, np.float64), det_offset=np.array(offset, np.int32),
                kept=kept_all)


def voc_ap(rec, prec):
    """evaluator.py:42-73, the area form."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def eval_rows(scene, box, cls, score, table, gt_labels, gt_count, nc, ovthresh):
    """evaluator.py:76-161 over explicit detection rows, listed in arrival order.  table (S,N,G): overlap of box (scene, box) with
    ground-truth row g of its scene; gt_labels (S,G), gt_count (S,) valid rows.  Per class: the class's rows by score descending
    (stable: equal scores in arrival order; a NaN score as -inf), each claims the ground-truth box of its class and scene it
    overlaps most (the first such), and is a true positive iff that overlap exceeds ovthresh and nobody claimed the box before.
    -> dict(tp (K,) bool per row, npos (nc,), ap / rec / prec {class: ...} for the classes with ground truth)."""
    scene, box, cls = np.asarray(scene), np.asarray(box), np.asarray(cls)
    score = np.asarray(score, np.float64)
    score = np.where(np.isnan(score), -np.inf, score)
    gt_labels, gt_count = np.asarray(gt_labels), np.asarray(gt_count)
    tp_row = np.zeros(len(scene), bool)
    npos = np.zeros(nc, np.int64)
    out = dict(ap={}, rec={}, prec={})
    for c in range(nc):
        cols = {s: np.nonzero(gt_labels[s, :gt_count[s]] == c)[0] for s in range(gt_labels.shape[0])}
        npos[c] = sum(len(v) for v in cols.values())
        mine = np.nonzero(cls == c)[0]
        order = mine[np.argsort(-score[mine], kind="stable")]
        taken = set()
        tp, fp = np.zeros(len(order)), np.zeros(len(order))
        for r, k in enumerate(order):
            s = int(scene[k])
            ovmax, jmax = -np.inf, -1
            for j in cols[s]:
                ov = table[s, box[k], j]
                if ov != ov:  # `ov.max() > ovthresh` of a row with a NaN is false
                    ovmax, jmax = -np.inf, -1
                    break
                if ov > ovmax:
                    ovmax, jmax = ov, int(j)
            if ovmax > np.float32(ovthresh) and (s, jmax) not in taken:
                tp[r] = 1.0
                taken.add((s, jmax))
                tp_row[k] = True
            else:
                fp[r] = 1.0
        if npos[c] > 0:
            fpc, tpc = np.cumsum(fp), np.cumsum(tp)
            rec = tpc / float(npos[c])
            prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
            out["rec"][c], out["prec"][c], out["ap"][c] = rec, prec, voc_ap(rec, prec)
    out["tp"], out["npos"] = tp_row, npos
    out["mAP"] = float(np.mean(list(out["ap"].values()))) if out["ap"] else float("nan")
    return out
