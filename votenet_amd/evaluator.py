"""Detection evaluation (evaluator.py:26-200 of the reference): VOC average precision per class at a 3D-IoU threshold.
The box overlaps -- the reference's shapely polygon loop over every (detection, ground-truth) pair -- come from the device
(votenet_iou3d_cross, the IoU kernel of the NMS); matching and the precision / recall curve are the reference's host logic
restated with numpy (they are O(detections)).

eval_det scores ONE batch.  DetectionAccumulator / evaluate score a whole validation set, as evaluator.py:217-233 collects every
scene before eval_det_cls ranks by confidence: each batch is matched on the device (votenet_eval_match, csrc/eval_match.hip) into
one 16-byte record per kept box, nothing is read back until result()."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import tf_nms3d
from .synth import MEAN_SIZES, NC


def box_corners(center, lwh, roty):
    """get_3d_box (dataset.py:92-109): (…,3), (…,3) l,w,h, (…) heading -> (…,8,3) corners, first four = top face."""
    c, s = np.cos(roty), np.sin(roty)
    l, w, h = lwh[..., 0], lwh[..., 1], lwh[..., 2]
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * 0.5
    sy = np.array([1, 1, 1, 1, -1, -1, -1, -1]) * 0.5
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * 0.5
    x0, y0, z0 = l[..., None] * sx, h[..., None] * sy, w[..., None] * sz
    x = c[..., None] * x0 + s[..., None] * z0
    z = -s[..., None] * x0 + c[..., None] * z0
    return (np.stack([x, y0, z], -1) + center[..., None, :]).astype(np.float32)


def voc_ap(rec, prec, use_07_metric=False):
    """evaluator.py:42-73."""
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap += p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def eval_det_cls(det_img, det_score, det_iou, gt_count, ovthresh=0.25, use_07_metric=False):
    """evaluator.py:76-161 for one class.  det_img[d]: image of detection d; det_score[d]; det_iou[d]: its IoU with every
    ground-truth box of this class in its image (1-D array, may be empty); gt_count {img: #gt boxes}.  -> rec, prec, ap."""
    npos = int(sum(gt_count.values()))
    order = np.argsort(-np.asarray(det_score, dtype=np.float64), kind="stable")
    taken = {img: np.zeros(c, bool) for img, c in gt_count.items()}
    tp, fp = np.zeros(len(order)), np.zeros(len(order))
    for r, d in enumerate(order):
        ov = det_iou[d]
        if len(ov) and ov.max() > ovthresh:
            j = int(ov.argmax())  # first maximum, as the reference's strict '>' scan
            if not taken[det_img[d]][j]:
                tp[r] = 1.0
                taken[det_img[d]][j] = True
            else:
                fp[r] = 1.0
        else:
            fp[r] = 1.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos) if npos else np.zeros_like(tp)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def _num_class(head, num_class, who):
    """The class count of a public function that takes head= and num_class=: the head's, else the keyword's, else the default head's."""
    if head is not None:
        from .head import resolve
        return resolve(head, 0, 0, 0)[2]
    if num_class is None:
        return NC
    if isinstance(num_class, bool) or not isinstance(num_class, (int, np.integer)) or not 1 <= int(num_class) <= 64:
        raise L.InvalidArgumentError("%s: num_class must be an integer in [1, 64], got %r" % (who, num_class))
    return int(num_class)


def eval_det(pred, gt, ovthresh=0.25, use_07_metric=False, head=None, num_class=None):
    """evaluator.py:164-200 on batched device tensors.
    pred: dict(bboxes (B,N,8,3) device, nms_idx (K,2) [scene, box] device, class_scores (B,N,NC) device) -- the predict
          tower's outputs; a kept box is ONE detection of its arg-max class with the max class score (evaluator.py:225-233).
    gt:   dict(boxes (B,G,8,3) numpy corners, labels (B,G) int, count (B,) valid boxes per scene).
    head / num_class: the classes scored are range(head.nc) / range(num_class) (neither: the default head's ten); a ground-truth
    label outside is counted nowhere.
    -> {class: ap}, mAP over the classes that occur in gt."""
    nc = _num_class(head, num_class, "eval_det")
    dev = pred["bboxes"].device
    gt_boxes = torch.from_numpy(np.ascontiguousarray(gt["boxes"], dtype=np.float32)).to(dev)
    iou = tf_nms3d.iou3d_cross(pred["bboxes"], gt_boxes).cpu().numpy()  # (B,N,G): every overlap the evaluation can ask for
    keep = pred["nms_idx"].cpu().numpy()
    cls_scores = pred["class_scores"].detach().cpu().numpy()
    labels, count = np.asarray(gt["labels"]), np.asarray(gt["count"])
    ap = {}
    for c in range(nc):
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
        ap[c] = eval_det_cls(d_img, d_score, d_iou, gt_count, ovthresh, use_07_metric)[2]
    return ap, (float(np.mean(list(ap.values()))) if ap else float("nan"))


def gt_for_eval(gt_np, counts=None, head=None):
    """synth.room_gt dict -> corners / labels / per-scene count (padding rows repeat the last box: counted once).  head: the
    HeadConfig the labels were made for; the labels pass through as they are (one outside [0, head.nc) is counted nowhere by
    eval_det and DetectionAccumulator)."""
    _num_class(head, None, "gt_for_eval")
    b, g = gt_np["bboxes_roty"].shape
    if counts is None:
        counts = []
        for s in range(b):
            n = g
            while n > 1 and np.array_equal(gt_np["bboxes_xyz"][s, n - 1], gt_np["bboxes_xyz"][s, n - 2]):
                n -= 1
            counts.append(n)
    return dict(boxes=box_corners(gt_np["bboxes_xyz"], gt_np["bboxes_lwh"], gt_np["bboxes_roty"]), labels=gt_np["semantic_labels"],
                count=np.asarray(counts))


def gt_to_device(gt, device):
    """gt_for_eval's dict (numpy or device tensors) -> the same dict as contiguous device tensors (boxes f32, labels / count int32):
    what DetectionAccumulator.add uses in place, so a validation set is uploaded once."""
    def conv(v, dtype):
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32 if dtype == torch.float32 else np.int32))
        return v.to(device=device, dtype=dtype).contiguous()
    return dict(boxes=conv(gt["boxes"], torch.float32), labels=conv(gt["labels"], torch.int32), count=conv(gt["count"], torch.int32))


def finalize_records(records, npos, thresholds, use_07_metric=False, head=None):
    """The host half of the streaming evaluation: records (K,4) int32 as votenet_eval_match writes them {score bits, class |
    tp_mask << 8, scene, arrival}, npos (NC,) ground-truth boxes per class over the whole set -> {threshold: dict(ap, mAP, rec,
    prec, npos)}.  Per class: sort by (-score, arrival) -- eval_det_cls's stable argsort of detections listed in arrival order --
    cumulative sums, voc_ap.  Classes without ground truth are left out, as eval_det leaves them out for a batch.  The class count is
    len(npos); with head it must be head.nc."""
    if head is not None and len(npos) != _num_class(head, None, "finalize_records"):
        raise L.InvalidArgumentError("finalize_records: npos holds %d classes, the head has %d" % (len(npos), head.nc))
    records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 4)
    score = records[:, 0].copy().view(np.float32).astype(np.float64)
    cls, mask = records[:, 1] & 0xff, (records[:, 1] >> 8) & 0xff
    arrival = records[:, 3].copy().view(np.uint32)
    order = np.lexsort((arrival, -score))
    cls_sorted, mask_sorted = cls[order], mask[order]
    out = {}
    for t, thr in enumerate(thresholds):
        res = dict(ap={}, rec={}, prec={}, npos={})
        for c in range(len(npos)):
            if npos[c] <= 0:
                continue
            tp = ((mask_sorted[cls_sorted == c] >> t) & 1).astype(np.float64)
            fp = 1.0 - tp
            fp, tp = np.cumsum(fp), np.cumsum(tp)
            rec = tp / float(npos[c])
            prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            res["rec"][c], res["prec"][c], res["npos"][c] = rec, prec, int(npos[c])
            res["ap"][c] = voc_ap(rec, prec, use_07_metric)
        res["mAP"] = float(np.mean(list(res["ap"].values()))) if res["ap"] else float("nan")
        out[thr] = res
    return out


class DetectionAccumulator:
    """Detection evaluation over any number of batches (evaluator.py:164-233).
        acc = DetectionAccumulator(device, thresholds=(0.25, 0.5), capacity=...)
        acc.add(pred, gt)      # enqueues one kernel; no host synchronisation
        res = acc.result()     # the one synchronisation: res[0.25] -> dict(ap, mAP, rec, prec, npos)
    capacity: the most detections (kept boxes) the whole set can offer; result() raises if more arrived.  records: an int32
    (rows >= capacity, 4) device tensor to use as the record buffer instead of allocating one.  Thresholds are compared in
    float32, as numpy compares a float32 overlap with a Python float.  Equal scores rank in arrival order (add call, then row).
    num_class (or head: its nc): the classes of the network whose predictions arrive, the default head's ten when neither is given;
    class_scores must have that many columns, and a ground-truth label outside [0, num_class) is counted nowhere."""
    FLAG_OVERFLOW, FLAG_BAD_ROW, FLAG_SCENE = 1, 2, 4

    def __init__(self, device, thresholds=(0.25, 0.5), capacity=1 << 21, records=None, num_class=None, head=None):
        self.device = torch.device(device)
        self.num_class = _num_class(head, num_class, "DetectionAccumulator")
        self.thresholds = tuple(float(t) for t in thresholds)
        if not 1 <= len(self.thresholds) <= 8:
            raise L.InvalidArgumentError("DetectionAccumulator: 1 to 8 IoU thresholds, got %d" % len(self.thresholds))
        self.capacity = int(capacity)
        if self.capacity < 0:
            raise L.InvalidArgumentError("DetectionAccumulator: negative capacity")
        if records is None:
            records = torch.empty((max(self.capacity, 1), 4), dtype=torch.int32, device=self.device)
        records = L.dev_i32(records, "DetectionAccumulator records", 2)
        if records.shape[1] != 4 or records.shape[0] < self.capacity:
            raise L.InvalidArgumentError("DetectionAccumulator: records must be (>= capacity, 4) int32, got %s" % (tuple(records.shape),))
        self._records = records
        self._thr = (ctypes.c_float * len(self.thresholds))(*self.thresholds)
        self._state = torch.zeros(2 + self.num_class, dtype=torch.int32, device=self.device)  # [records offered, flags, npos[num_class]]
        self._scene = self._arrival = 0

    def reset(self):
        self._state.zero_()
        self._scene = self._arrival = 0

    def add(self, pred, gt):
        """pred: what VoteNetHotPath.predict returns (sync=True: nms_idx (K,2); sync=False: padded nms_idx + nms_count on the
        device; protocol="per_class": det_rows (R,4) + det_offset (B+1,), matched row by row through votenet_eval_match_rows -- the
        arrival number then advances by R, the rows offered room for).  gt: gt_for_eval's dict, numpy (uploaded here) or device
        tensors (gt_to_device: used in place)."""
        boxes = L.dev_f32(pred["bboxes"].detach(), "DetectionAccumulator.add: bboxes (B,N,8,3)", 4, 3)
        b, n = boxes.shape[:2]
        if boxes.shape[2] != 8:
            raise L.InvalidArgumentError("DetectionAccumulator.add expects (B, N, 8, 3) boxes")
        if "det_rows" in pred:
            return self._add_rows(boxes, pred, gt)
        cls = L.dev_f32(pred["class_scores"].detach(), "DetectionAccumulator.add: class_scores (B,N,NC)", 3, self.num_class)
        if tuple(cls.shape[:2]) != (b, n):
            raise L.InvalidArgumentError("DetectionAccumulator.add: class_scores %s do not match boxes %s" % (tuple(cls.shape), tuple(boxes.shape)))
        rows = L.dev_i32(pred["nms_idx"], "DetectionAccumulator.add: nms_idx (K,2)", 2)
        if rows.shape[1] != 2:
            raise L.InvalidArgumentError("DetectionAccumulator.add: nms_idx must be (K, 2)")
        count = pred.get("nms_count")
        if count is not None:
            count = L.dev_i32(count, "DetectionAccumulator.add: nms_count")
        g, ng = self._gt(gt, b)
        k = rows.shape[0]
        if self._arrival + k > 0xffffffff:
            raise L.VotenetError("DetectionAccumulator: more than 2^32 kept rows offered")
        st = self._state
        with L.device_guard(self.device):
            L.check(L.lib().votenet_eval_match(b, n, ng, self.num_class, L.ptr(boxes), L.ptr(rows) if k else None, k, L.ptr(count), L.ptr(cls),
                                               L.ptr(g["boxes"]), L.ptr(g["labels"]), L.ptr(g["count"]), len(self.thresholds), self._thr,
                                               self._scene, self._arrival, L.ptr(self._records), self.capacity, st.data_ptr(),
                                               st.data_ptr() + 8, st.data_ptr() + 4, L.stream_ptr()))
        self._scene += b
        self._arrival += k

    def _gt(self, gt, b):
        g = gt_to_device(gt, self.device)
        if g["boxes"].dim() != 4 or tuple(g["boxes"].shape[2:]) != (8, 3) or g["boxes"].shape[0] != b:
            raise L.InvalidArgumentError("DetectionAccumulator.add expects (B, G, 8, 3) ground-truth boxes, got %s" % (tuple(g["boxes"].shape),))
        ng = g["boxes"].shape[1]
        if tuple(g["labels"].shape) != (b, ng) or tuple(g["count"].shape) != (b,):
            raise L.InvalidArgumentError("DetectionAccumulator.add: labels must be (B, G) and count (B,)")
        return g, ng

    def _add_rows(self, boxes, pred, gt):
        """add() for explicit detection rows (detections.class_nms3d): the same records, flags and capacity rule."""
        b, n = boxes.shape[:2]
        rows = L.dev_i32(pred["det_rows"], "DetectionAccumulator.add: det_rows (R,4)", 2)
        if rows.shape[1] != 4:
            raise L.InvalidArgumentError("DetectionAccumulator.add: det_rows must be (R, 4)")
        offset = L.dev_i32(pred["det_offset"], "DetectionAccumulator.add: det_offset (B+1,)", 1)
        if offset.shape[0] != b + 1:
            raise L.InvalidArgumentError("DetectionAccumulator.add: det_offset must be (B + 1,), got %s" % (tuple(offset.shape),))
        g, ng = self._gt(gt, b)
        k = rows.shape[0]
        if self._arrival + k > 0xffffffff:
            raise L.VotenetError("DetectionAccumulator: more than 2^32 detection rows offered")
        st = self._state
        with L.device_guard(self.device):
            L.check(L.side_lib("detect").votenet_eval_match_rows(
                b, n, ng, self.num_class, L.ptr(boxes), L.ptr(rows) if k else None, k, L.ptr(offset), L.ptr(g["boxes"]), L.ptr(g["labels"]),
                L.ptr(g["count"]), len(self.thresholds), self._thr, self._scene, self._arrival, L.ptr(self._records), self.capacity,
                st.data_ptr(), st.data_ptr() + 8, st.data_ptr() + 4, L.stream_ptr()), side="detect")
        self._scene += b
        self._arrival += k

    def result(self, use_07_metric=False):
        state = self._state.cpu().numpy()
        offered, flags, npos = int(state[0]), int(state[1]), state[2:]
        if flags & self.FLAG_OVERFLOW or offered > self.capacity:
            raise L.VotenetError("DetectionAccumulator: capacity %d, %d detections offered" % (self.capacity, offered))
        if flags & self.FLAG_BAD_ROW:
            raise L.InvalidArgumentError("DetectionAccumulator: a kept row names a scene or a box outside its batch")
        if flags & self.FLAG_SCENE:
            raise L.InvalidArgumentError("DetectionAccumulator: more than 1024 kept rows in one scene")
        return finalize_records(self._records[:offered].cpu().numpy(), npos, self.thresholds, use_07_metric)


def evaluate(net, batches, gts, thresholds=(0.25, 0.5), iou_threshold=0.25, protocol="reference", min_points=0, nms_overlap="rotated",
             nms_measure="iou"):
    """mAP of `net` over a validation set: batches[i] (B,n,3) device clouds -- or (cloud, feats (B,n,c)) pairs for a network built with
    point features --, gts[i] gt_for_eval's dict (numpy or device).  Every predict call is asynchronous with the next batch's
    geometry underneath it; one synchronisation at the end.  protocol: predict's ("reference", "per_class" or a dict of
    detections.class_nms3d's parameters); per class, every box offers a detection of every class.  min_points: predict's (5,
    box_points.PAPER_MIN_POINTS, with "per_class": boxes that hold fewer points of the cloud are dropped).  nms_overlap, nms_measure:
    predict's ("aabb3d", aabb_nms.PAPER_OVERLAP, with "per_class" and min_points=5 is the paper's protocol: the NMS suppresses by the
    overlap of the boxes' axis-aligned hulls; the matching below stays on the rotated-box IoU, as the paper's does).
    The classes are net.head's.
    -> {threshold: dict(ap, mAP, rec, prec, npos)}."""
    from . import aabb_nms
    head = getattr(net, "head", None)
    nc = _num_class(head, None, "evaluate")
    aabb_nms.check_overlap(protocol, nms_overlap, nms_measure, "evaluate")
    acc = None
    kw = {} if protocol == "reference" else dict(protocol=protocol)  # (the call of the reference's protocol, as it was)
    if min_points:
        kw["min_points"] = min_points
    if nms_overlap != "rotated":  # (the rotated overlap: predict is called without the arguments, as it was)
        kw.update(nms_overlap=nms_overlap, nms_measure=nms_measure)
    pairs = [tuple(v) if isinstance(v, (tuple, list)) else (v, None) for v in batches]
    for i, ((x, f), g) in enumerate(zip(pairs, gts)):
        nx, nf = pairs[i + 1] if i + 1 < len(pairs) else (None, None)
        if f is None:  # (the call of every network without point features, as it was)
            pred = net.predict(x, iou_threshold, next_x=nx, sync=False, **kw)
        else:
            pred = net.predict(x, iou_threshold, next_x=nx, sync=False, feats=f, next_feats=nf, **kw)
        if acc is None:  # every proposal of every scene kept (per class: offering every class): the most the set can offer
            per_box = nc if "det_rows" in pred else 1
            acc = DetectionAccumulator(x.device, thresholds, capacity=sum(int(v.shape[0]) for v, _ in pairs) * int(pred["bboxes"].shape[1]) * per_box,
                                       **(dict(num_class=nc) if head is not None and not head.is_default else {}))
        acc.add(pred, g)
    if acc is None:
        raise L.InvalidArgumentError("evaluate: no batches")
    return acc.result()
