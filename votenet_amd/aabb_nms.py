"""Axis-aligned NMS overlaps: the overlap rule of the VoteNet paper's parse_predictions on the device (libvotenet_aabb.so,
include/votenet_aabb_nms.h).

The paper suppresses by the overlap of each box's axis-aligned hull -- in 3D (nms_3d_faster, its default) or on the ground plane
(nms_2d_faster) -- as IoU or as its "old type" measure, intersection over the later box.  detections.class_nms3d suppresses by the
rotated-box IoU of the rest of the project; class_nms_aabb is that NMS, rule for rule, with the hull overlap in its place, and
overlap_matrix is the table it decides on.  The rules are stated once, in the header; tests/aabb_nms_ref.py restates them in numpy
float32."""
import torch

from . import _lib as L
from .detections import _class_nms, _entry

OVERLAPS = ("rotated", "aabb3d", "bev")  # predict / evaluate's nms_overlap; "rotated" is detections.class_nms3d
PAPER_OVERLAP = "aabb3d"  # parse_predictions' default: use_3d_nms
MEASURES = ("iou", "over_later")  # "over_later": the paper's use_old_type_nms
_MODE = dict(aabb3d=0, bev=1)  # VOTENET_AABB_3D, VOTENET_AABB_BEV
_MEASURE = dict(iou=0, over_later=1)  # VOTENET_AABB_IOU, VOTENET_AABB_OVER_LATER


_CLASS_NMS_AABB = _entry("aabb", "class_nms_aabb")


def check_overlap(protocol, nms_overlap, nms_measure, who):
    """predict / evaluate's keywords: raises InvalidArgumentError for a combination that names no NMS."""
    if nms_overlap not in OVERLAPS:
        raise L.InvalidArgumentError("%s: nms_overlap must be one of %s, got %r" % (who, ", ".join(map(repr, OVERLAPS)), nms_overlap))
    if nms_measure not in MEASURES:
        raise L.InvalidArgumentError("%s: nms_measure must be one of %s, got %r" % (who, ", ".join(map(repr, MEASURES)), nms_measure))
    if nms_overlap == "rotated" and nms_measure != "iou":
        raise L.InvalidArgumentError("%s: nms_measure %r needs nms_overlap \"aabb3d\" or \"bev\" (the rotated-box overlap is an IoU)"
                                     % (who, nms_measure))
    if protocol == "reference" and nms_overlap != "rotated":
        raise L.InvalidArgumentError("%s: nms_overlap %r needs protocol \"per_class\" or a dict (the reference's protocol suppresses by "
                                     "the rotated-box IoU)" % (who, nms_overlap))


def _codes(overlap, measure, who):
    if overlap not in _MODE:
        raise L.InvalidArgumentError("%s: overlap must be \"aabb3d\" or \"bev\", got %r" % (who, overlap))
    if measure not in _MEASURE:
        raise L.InvalidArgumentError("%s: measure must be \"iou\" or \"over_later\", got %r" % (who, measure))
    return _MODE[overlap], _MEASURE[measure]


def overlap_matrix(bboxes, overlap="aabb3d", measure="iou"):
    """(B,N,8,3) f32 boxes on the device -> (B,N,N) f32 on the device: [s][j][i] is the overlap of box j, as the later box, against
    box i, as the earlier one (the measures differ in that: "over_later" divides by the later box's size).  Nothing synchronises."""
    mode, meas = _codes(overlap, measure, "overlap_matrix")
    bboxes = L.dev_f32(bboxes.detach(), "overlap_matrix expects (batch_size, nbbox, 8, 3) bbox shape.", 4, 3)
    if bboxes.shape[2] != 8:
        raise L.InvalidArgumentError("overlap_matrix expects (batch_size, nbbox, 8, 3) bbox shape.")
    b, n = bboxes.shape[:2]
    out = torch.empty((b, n, n), dtype=torch.float32, device=bboxes.device)
    with L.device_guard(bboxes.device):
        L.check(L.side_lib("aabb").votenet_aabb_overlap_matrix(b, n, L.ptr(bboxes), mode, meas, L.ptr(out), L.stream_ptr()), side="aabb")
    return out


def class_nms_aabb(bboxes, objectness, class_scores, iou_threshold=0.25, conf_thresh=0.05, class_nms=True, per_class=True,
                   overlap="aabb3d", measure="iou"):
    """detections.class_nms3d deciding on the axis-aligned overlap: the same arguments, the same dict(det_rows, det_offset), the same
    rows wherever the two overlaps agree on which side of iou_threshold every pair falls.  N <= 512, NC <= 64."""
    return _class_nms(_CLASS_NMS_AABB, _codes(overlap, measure, "class_nms_aabb"), bboxes, objectness, class_scores, iou_threshold,
                      conf_thresh, class_nms, per_class)
