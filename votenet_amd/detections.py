"""Per-class detections: the VoteNet paper's evaluation protocol on the device (libvotenet_detect.so, include/votenet_detections.h).

The reference's protocol (model.py:133, evaluator.py:224-231; tf_nms3d.NMS3D, votenet_eval_match) orders boxes by their largest class
logit, suppresses across classes, gates on o1 > o0 and offers one detection per kept box.  The paper's orders by P(object), suppresses
inside a class, drops boxes below a confidence threshold and offers one detection per class and kept box, scored P(object) P(class).
The rules are stated once, in the header; tests/detections_ref.py restates them in numpy."""
import math

import numpy as np
import torch

from . import _lib as L

PAPER = dict(iou_threshold=0.25, conf_thresh=0.05, class_nms=True, per_class=True)  # the protocol's defaults
MAX_BOXES, MAX_CLASSES = 512, 64


def conf_logit(c):
    """T = float32(log(c) - log1p(-c)), in double: P(object) > c  <=>  o1 - o0 > T.  0 -> -inf, 0.5 -> 0.0 exactly."""
    c = float(c)
    if not 0.0 <= c < 1.0:
        raise L.InvalidArgumentError("conf_thresh must be in [0, 1), got %r" % (c,))
    if c == 0.0:
        return float("-inf")
    return float(np.float32(math.log(c) - math.log1p(-c)))


def protocol_params(protocol, iou_threshold=0.25):
    """predict / evaluate's `protocol` -> None for "reference", else the four parameters of class_nms3d: "per_class" is the paper's
    defaults with the caller's iou_threshold, a dict overrides any of the four."""
    if protocol == "reference":
        return None
    params = dict(PAPER, iou_threshold=iou_threshold)
    if isinstance(protocol, dict):
        unknown = sorted(set(protocol) - set(PAPER))
        if unknown:
            raise L.InvalidArgumentError("protocol: unknown parameter(s) %s (the four are %s)" % (unknown, sorted(PAPER)))
        params.update(protocol)
    elif protocol != "per_class":
        raise L.InvalidArgumentError("protocol must be \"reference\", \"per_class\" or a dict of %s, got %r" % (sorted(PAPER), protocol))
    return params


def _entry(side, who):
    """What _class_nms needs of an entry votenet_<who> of side library `side`, formed once: the names and the three shape messages."""
    return (side, "votenet_" + who, "votenet_%s_workspace_bytes" % who, "%s expects (batch_size, nbbox, 8, 3) bbox shape." % who,
            "%s expects (batch_size, nbbox, 2) objectness shape." % who, "%s expects (batch_size, nbbox, num_class) class_scores shape." % who)


def _class_nms(entry, tail, bboxes, objectness, class_scores, iou_threshold, conf_thresh, class_nms, per_class):
    """class_nms3d and aabb_nms.class_nms_aabb: the shape checks, the buffers and the call of an _entry (its library is loaded here,
    so only when it is asked for); `tail`: the entry's arguments between per_class and det_rows."""
    side, fn, ws_fn, box_shape, obj_shape, cls_shape = entry
    bboxes = L.dev_f32(bboxes.detach(), box_shape, 4, 3)
    if bboxes.shape[2] != 8:
        raise L.InvalidArgumentError(box_shape)
    b, n = bboxes.shape[:2]
    objectness = L.dev_f32(objectness.detach(), obj_shape, 3, 2)
    if tuple(objectness.shape) != (b, n, 2):
        raise L.InvalidArgumentError(obj_shape)
    class_scores = L.dev_f32(class_scores.detach(), cls_shape, 3)
    if tuple(class_scores.shape[:2]) != (b, n):
        raise L.InvalidArgumentError(cls_shape)
    nc = class_scores.shape[2]
    t = conf_logit(conf_thresh)
    lib = L.side_lib(side)
    cap = b * n * (nc if per_class else 1)
    rows = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=bboxes.device)
    offset = torch.empty(b + 1, dtype=torch.int32, device=bboxes.device)
    wbytes = getattr(lib, ws_fn)(b, n, nc)
    ws = torch.empty(wbytes, dtype=torch.uint8, device=bboxes.device)
    with L.device_guard(bboxes.device):
        L.check(getattr(lib, fn)(b, n, nc, L.ptr(bboxes), L.ptr(objectness), L.ptr(class_scores), float(iou_threshold), t,
                                 1 if class_nms else 0, 1 if per_class else 0, *tail, L.ptr(rows), cap, L.ptr(offset), L.ptr(ws), wbytes,
                                 L.stream_ptr()), side=side)
    return dict(det_rows=rows[:cap], det_offset=offset)


_CLASS_NMS3D = _entry("detect", "class_nms3d")


def class_nms3d(bboxes, objectness, class_scores, iou_threshold=0.25, conf_thresh=0.05, class_nms=True, per_class=True):
    """(B,N,8,3) boxes, (B,N,2) objectness logits, (B,N,NC) class logits, all f32 on the device ->
    dict(det_rows (B*N*NC or B*N, 4) int32 {scene, box, class, score bits}, det_offset (B+1,) int32): scene s owns
    det_rows[det_offset[s]:det_offset[s+1]], the total is det_offset[B]; rows beyond it are not written.  Everything stays on the
    device and nothing synchronises (rows_to_host does).  N <= 512, NC <= 64."""
    return _class_nms(_CLASS_NMS3D, (), bboxes, objectness, class_scores, iou_threshold, conf_thresh, class_nms, per_class)


def rows_to_host(det):
    """class_nms3d's / predict's dict -> (scene, box, class int32 arrays, score float32 array, offset (B+1,) int32) of the valid rows,
    as numpy.  The one call of this module that synchronises."""
    offset = det["det_offset"].cpu().numpy()
    rows = det["det_rows"][:int(offset[-1])].cpu().numpy()
    return rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy(), rows[:, 3].copy().view(np.float32), offset
