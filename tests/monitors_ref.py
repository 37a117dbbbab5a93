"""A float64 numpy restatement of the training summaries (votenet_accuracies, votenet_tensor_stats), written from the reference's
model.py:148-166, 210-216 (assignment, obj_accuracy, sem_accuracy), tf.nn.in_top_k's contract and tensorpack's rms summary.  Test
infrastructure: nothing here imports the package under test."""
import numpy as np

HIST_BINS = 130


def in_top_1(logits, target):
    """tf.nn.in_top_k(predictions, targets, 1) of one row: the target's score is finite and no other class scores strictly higher."""
    logits = np.asarray(logits, dtype=np.float64)
    if not 0 <= int(target) < len(logits):
        return False
    t = logits[int(target)]
    return bool(np.isfinite(t) and not (logits > t).any())


def assignment(prop, bboxes_xyz, pos_thr=0.3, neg_thr=0.6):
    """model.py:148-155 -> (positive mask, negative mask, assigned box, min_dist), all (B, P); first arg-min."""
    d = np.linalg.norm(np.asarray(prop, np.float64)[:, :, None] - np.asarray(bboxes_xyz, np.float64)[:, None], axis=-1)
    mind = d.min(-1)
    return mind < pos_thr, mind > neg_thr, d.argmin(-1), mind


def decision_margin(prop, bboxes_xyz, pos_thr=0.3, neg_thr=0.6):
    """How far the case is from a decision an fp32 kernel could take the other way: (smallest |min_dist - threshold|, smallest gap
    between a proposal's nearest and second nearest DISTINCT distance).  Repeated (padding) boxes tie exactly and take the first
    arg-min in both arithmetics."""
    d = np.linalg.norm(np.asarray(prop, np.float64)[:, :, None] - np.asarray(bboxes_xyz, np.float64)[:, None], axis=-1)
    mind = d.min(-1)
    thr = min(np.abs(mind - pos_thr).min(), np.abs(mind - neg_thr).min())
    gap = np.where(d > mind[..., None], d - mind[..., None], np.inf).min()
    return float(thr), float(gap)


def accuracies(prop, out, gt, nh=12, ns=10, nc=10, pos_thr=0.3, neg_thr=0.6):
    """-> dict(n_obj_correct, n_sem_correct, n_pos, n_neg (ints), obj_accuracy, sem_accuracy (float64; NaN on an empty set))."""
    pos, neg, box, _ = assignment(prop, gt["bboxes_xyz"], pos_thr, neg_thr)
    out = np.asarray(out)
    assert out.shape[-1] == 5 + 2 * nh + 4 * ns + nc
    n_obj = n_sem = 0
    for b, p in zip(*np.nonzero(pos)):
        n_obj += in_top_1(out[b, p, :2], 1)                                                       # model.py:164
        n_sem += in_top_1(out[b, p, out.shape[-1] - nc:], gt["semantic_labels"][b, box[b, p]])    # model.py:210-215
    for b, p in zip(*np.nonzero(neg)):
        n_obj += in_top_1(out[b, p, :2], 0)                                                       # model.py:165
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        obj_acc = np.float64(n_obj) / np.float64(n_pos + n_neg)
        sem_acc = np.float64(n_sem) / np.float64(n_pos)
    return dict(n_obj_correct=int(n_obj), n_sem_correct=int(n_sem), n_pos=n_pos, n_neg=n_neg, obj_accuracy=float(obj_acc),
                sem_accuracy=float(sem_acc))


def hist_bin(v):
    """Bin of one fp32 value: 0 zero / subnormal; 1 + (e + 40) positive with |v| in [2^e, 2^(e+1)), e clamped to [-40, 23];
    65 + (e + 40) negative; 129 inf / NaN."""
    v = np.float32(v)
    if not np.isfinite(v):
        return HIST_BINS - 1
    a = abs(float(v))
    if a < 2.0 ** -126:
        return 0
    _, e = np.frexp(a)  # a = m * 2^e, 0.5 <= m < 1
    e = min(max(int(e) - 1, -40), 23)
    return 1 + (e + 40) + (64 if np.signbit(v) else 0)


def tensor_stats(x, segments, scale=1.0, clip=0.0):
    """x: the flat fp32 bucket; segments: [(start, end)].  -> per segment dict(numel, nonfinite, sum, sumsq, abs_sum (float64 sums
    over the finite elements), min, max (fp32; +inf / -inf without a finite element), hist (130 int64), clip_factor)."""
    rows = []
    for a, b in segments:
        v = np.asarray(x[a:b], dtype=np.float32)
        if scale != 1.0:
            v = (v * np.float32(scale)).astype(np.float32)
        fin = np.isfinite(v)
        f = v[fin].astype(np.float64)
        hist = np.zeros(HIST_BINS, np.int64)
        for e in v:
            hist[hist_bin(e)] += 1
        bad = int((~fin).sum())
        ss = float((f * f).sum())
        factor = 1.0
        if clip > 0:
            factor = clip / max(np.sqrt(ss) / (b - a), clip)
        if bad:
            factor = float("nan")
        rows.append(dict(numel=b - a, nonfinite=bad, sum=float(f.sum()), sumsq=ss, abs_sum=float(np.abs(f).sum()),
                         min=np.float32(f.min()) if f.size else np.float32(np.inf),
                         max=np.float32(f.max()) if f.size else np.float32(-np.inf), hist=hist, clip_factor=factor))
    return rows


# ---- the hand-made cases of the accuracy tests: two scenes, a few proposals placed ON box centres (distance 0: positive) or far away
# (negative), logits written by hand.  -> (prop, out, gt, expected dict)
def _blank(b, p, bb, nh=12, ns=10, nc=10):
    F = np.float32
    gt = dict(bboxes_xyz=np.zeros((b, bb, 3), F), bboxes_lwh=np.ones((b, bb, 3), F), bboxes_roty=np.zeros((b, bb), F),
              semantic_labels=np.zeros((b, bb), np.int32), heading_labels=np.zeros((b, bb), np.int32),
              heading_residuals=np.zeros((b, bb), F), size_labels=np.zeros((b, bb), np.int32), size_residuals=np.zeros((b, bb, 3), F))
    for s in range(b):
        for j in range(bb):
            gt["bboxes_xyz"][s, j] = (3.0 * j, 0.0, 2.0 + 5.0 * s)
    prop = np.full((b, p, 3), 100.0, F)   # far from every box: negative
    out = np.zeros((b, p, 5 + 2 * nh + 4 * ns + nc), F)
    out[:, :, 0] = 1.0                    # class 0 ahead: a negative is obj-correct unless a case says otherwise
    return prop, out, gt


def case_tie():
    """A tie in the objectness logits is correct (for a positive and for a negative); a tie in the class logits too."""
    prop, out, gt = _blank(2, 4, 2)
    gt["semantic_labels"][0, 1] = 3
    prop[0, 0] = gt["bboxes_xyz"][0, 1]   # positive, box 1, label 3
    out[0, 0, :2] = (0.5, 0.5)            # tie: class 1 in the top 1
    out[0, 0, 69 + 3] = 2.0
    out[0, 0, 69 + 7] = 2.0               # tie between the label and another class: correct
    out[0, 1, :2] = (-1.0, -1.0)          # negative with a tie: class 0 in the top 1
    out[1, 2, :2] = (0.0, 1.0)            # negative that says "object": wrong
    return prop, out, gt, dict(n_obj_correct=7, n_sem_correct=1, n_pos=1, n_neg=7, obj_accuracy=7 / 8, sem_accuracy=1.0)


def case_nan_target():
    """A NaN (or infinite) target logit is wrong whatever the others are; a NaN in ANOTHER class does not beat the target."""
    prop, out, gt = _blank(2, 4, 2)
    gt["semantic_labels"][:] = 2
    prop[0, 0] = gt["bboxes_xyz"][0, 0]
    out[0, 0, :2] = (0.0, np.nan)         # positive, target logit (class 1) NaN: obj wrong
    out[0, 0, 69 + 2] = np.nan            # sem target NaN: wrong
    prop[1, 1] = gt["bboxes_xyz"][1, 1]
    out[1, 1, :2] = (np.nan, 0.0)         # positive, the OTHER logit NaN: correct
    out[1, 1, 69 + 2] = 1.0
    out[1, 1, 69 + 5] = np.nan            # another class NaN: the label still wins
    out[1, 3, :2] = (np.inf, 0.0)         # negative whose target logit is +inf: not finite -> wrong
    return prop, out, gt, dict(n_obj_correct=6, n_sem_correct=1, n_pos=2, n_neg=6, obj_accuracy=6 / 8, sem_accuracy=0.5)


def case_no_positive():
    """No positive proposal: sem_accuracy is NaN (tf.reduce_mean of an empty tensor), obj_accuracy finite."""
    prop, out, gt = _blank(2, 4, 2)
    out[0, 2, :2] = (0.0, 3.0)            # one negative wrong
    prop[1, 0] = gt["bboxes_xyz"][1, 0] + np.float32(0.45)  # |(.45,.45,.45)| = 0.78 > 0.6: negative; (a proposal at 0.3..0.6 is neither)
    prop[1, 1] = gt["bboxes_xyz"][1, 0] + np.array([0.45, 0.0, 0.0], np.float32)  # 0.45: neither positive nor negative
    return prop, out, gt, dict(n_obj_correct=6, n_sem_correct=0, n_pos=0, n_neg=7, obj_accuracy=6 / 7, sem_accuracy=float("nan"))


def case_label_out_of_range():
    """A semantic label of nc or -1 is in nobody's top 1 (tf.nn.in_top_k: a target out of range is false) and is not turned into an
    index: the floats such an index would reach (the next row's first logit; the last size-residual slot) hold scores that would win."""
    prop, out, gt = _blank(2, 4, 2)
    gt["semantic_labels"][0] = (10, -1)
    gt["semantic_labels"][1] = (7, 4)
    for s, i, j in ((0, 0, 0), (0, 2, 1), (1, 1, 1)):
        prop[s, i] = gt["bboxes_xyz"][s, j]
        out[s, i, :2] = (0.0, 1.0)        # positive and says so: obj-correct
    out[0, 1, 0] = 5.0                    # what column 69 + 10 of row (0, 0) would be: the next row's first float
    out[0, 2, 68] = 5.0                   # what column 69 - 1 of row (0, 2) is
    out[1, 1, 69 + 4] = 2.0               # a valid label beside them: correct
    return prop, out, gt, dict(n_obj_correct=8, n_sem_correct=1, n_pos=3, n_neg=5, obj_accuracy=1.0, sem_accuracy=1 / 3)


HAND_CASES = dict(tie=case_tie, nan_target=case_nan_target, no_positive=case_no_positive, label_out_of_range=case_label_out_of_range)
