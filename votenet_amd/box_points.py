"""Points inside predicted boxes: the `remove_empty_box` step of the VoteNet paper's parse_predictions on the device
(libvotenet_boxpts.so, include/votenet_box_points.h).

The paper counts the points of the input cloud inside every predicted box and keeps a box with fewer than 5 out of the NMS and the
detections.  Here the count decides a gated COPY of the objectness logits -- NaN where a box holds fewer than min_points points -- and
the NMS entries that exist do the rest: neither tf_nms3d.NMS3D (o1 > o0 is false for a NaN) nor detections.class_nms3d (a NaN margin
is never a candidate) makes such a box a candidate.  The rule is stated once, in the header; tests/box_points_ref.py restates it in
numpy float32."""
import operator

import torch

from . import _lib as L

PAPER_MIN_POINTS = 5  # parse_predictions' remove_empty_box: a box with fewer points is dropped
MAX_BOXES = 1024


def box_point_counts(bboxes, points):
    """(B,N,8,3) f32 boxes in decode_boxes' corner layout, (B,NPTS,3) f32 points, both on the device -> (B,N) int32 on the device:
    the points of scene s inside (faces, edges and corners included) box i of scene s.  NaN points and boxes count nothing.  Nothing
    synchronises.  N <= 1024, NPTS < 2^24."""
    bboxes = L.dev_f32(bboxes.detach(), "box_point_counts expects (batch_size, nbbox, 8, 3) bbox shape.", 4, 3)
    if bboxes.shape[2] != 8:
        raise L.InvalidArgumentError("box_point_counts expects (batch_size, nbbox, 8, 3) bbox shape.")
    b, n = bboxes.shape[:2]
    points = L.dev_f32(points.detach(), "box_point_counts expects (batch_size, npoint, 3) points shape.", 3, 3)
    if points.shape[0] != b:
        raise L.InvalidArgumentError("box_point_counts expects (batch_size, npoint, 3) points shape.")
    if points.device != bboxes.device:
        raise L.InvalidArgumentError("box_point_counts: bboxes and points live on different devices")
    counts = torch.empty((b, n), dtype=torch.int32, device=bboxes.device)
    with L.device_guard(bboxes.device):
        L.check(L.side_lib("boxpts").votenet_box_point_counts(b, n, points.shape[1], L.ptr(bboxes), L.ptr(points), L.ptr(counts),
                                                               L.stream_ptr()), side="boxpts")
    return counts


def gate_objectness(objectness, counts, min_points=PAPER_MIN_POINTS):
    """(B,N,2) f32 objectness logits, (B,N) int32 counts -> a new (B,N,2) tensor: the logits bit for bit where counts >= min_points,
    NaN elsewhere (min_points = 0: an exact copy).  Hand it to NMS3D / class_nms3d in objectness' place."""
    objectness = L.dev_f32(objectness.detach(), "gate_objectness expects (batch_size, nbbox, 2) objectness shape.", 3, 2)
    b, n = objectness.shape[:2]
    counts = L.dev_i32(counts, "gate_objectness expects (batch_size, nbbox) int32 counts.", 2)
    if tuple(counts.shape) != (b, n):
        raise L.InvalidArgumentError("gate_objectness expects (batch_size, nbbox) int32 counts.")
    if counts.device != objectness.device:
        raise L.InvalidArgumentError("gate_objectness: objectness and counts live on different devices")
    try:
        min_points = operator.index(min_points)
    except TypeError:
        raise L.InvalidArgumentError("gate_objectness: min_points must be an integer, got %r" % (min_points,)) from None
    gated = torch.empty_like(objectness)
    with L.device_guard(objectness.device):
        L.check(L.side_lib("boxpts").votenet_gate_objectness(b, n, L.ptr(counts), min_points, L.ptr(objectness), L.ptr(gated),
                                                              L.stream_ptr()), side="boxpts")
    return gated
