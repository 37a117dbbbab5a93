"""Ground-truth boxes from instance-labelled points on the device (libvotenet_instbox.so, include/votenet_instance_boxes.h).

Data without annotated boxes -- ScanNet-style scans, simulator output -- comes as a cloud with an instance id and a semantic label per
point.  The boxes are the extents of the instances in the cloud the network sees, as the VoteNet paper's second benchmark forms them:
axis-aligned, heading 0, the class of the instance's label mapped through `class_map` into the network's classes.  The rule is stated
once, in the header; tests/instance_boxes_ref.py restates it in numpy and every output is compared by bit pattern."""
import operator
import os
import re

import numpy as np
import torch

from . import _lib as L
from .synth import NC

MAX_K = 1024
MAX_SEM = 65536
STATUS = ("kept", "no_class", "few_points", "absent")  # the codes 0 .. 3 of `status`


def _tile():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", L.SIDE_LIBS["instbox"])) as f:
        return int(re.search(r"#define\s+VOTENET_INSTANCE_BOXES_TILE\s+(\d+)", f.read()).group(1))


TILE = _tile()  # the points one workgroup of the tile pass folds: the header states it


def _int(v, name, lo, hi=None):
    try:
        v = operator.index(v)
    except TypeError:
        raise L.InvalidArgumentError("boxes_from_labels: %s must be an integer, got %r" % (name, v)) from None
    if v < lo or (hi is not None and v > hi):
        raise L.InvalidArgumentError("boxes_from_labels: %s must be %s, got %d"
                                     % (name, ">= %d" % lo if hi is None else "in [%d, %d]" % (lo, hi), v))
    return v


def _labels(t, name, shape, dev):
    if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
        raise L.InvalidArgumentError("boxes_from_labels: %s must be a tensor on points' device" % name)
    if t.dtype != torch.int32:
        raise L.InvalidArgumentError("boxes_from_labels: %s must be int32, got %s" % (name, t.dtype))
    if tuple(t.shape) != shape:
        raise L.InvalidArgumentError("boxes_from_labels: %s must have shape %s, got %s" % (name, shape, tuple(t.shape)))
    if not t.is_contiguous():
        raise L.InvalidArgumentError("boxes_from_labels: %s must be contiguous" % name)
    return t


def boxes_from_labels(points, instance, semantic, class_map, k=256, n_class=NC, min_points=1, want_point_box=False, head=None):
    """points (b, n, 3) float32 -- the cloud the network sees, i.e. subsample_augment's output --, instance (b, n) and semantic (b, n)
    int32, all contiguous on one device; class_map (n_sem) int32, a device tensor or a host array: semantic label -> class of the
    network, or -1.  Ids outside [0, k), non-finite points and negative ("unlabelled") ids are ignored.
    -> dict: center (nkept, 3), size (nkept, 3), heading (nkept) float64 and cls (nkept) int32 device tensors, scene order then
    ascending id -- what augment_boxes takes; box_offset host int64 (b+1), the one read-back; instance_id, n_points (nkept) int32;
    status (STATUS), inst_count, slot (b, k) int32; ignored (b, 3) int32: unlabelled, id out of the table, non-finite;
    point_box (b, n) int32 if asked: the row of each point's instance within its scene, -1 where it has none.
    head: a HeadConfig whose class count stands in n_class's place."""
    if head is not None:
        from .head import resolve
        n_class = resolve(head, 0, 0, n_class)[2]
    if not torch.is_tensor(points) or not points.is_cuda:
        raise L.InvalidArgumentError("boxes_from_labels: points must be a device tensor")
    if points.dtype != torch.float32:
        raise L.InvalidArgumentError("boxes_from_labels: points must be float32, got %s" % points.dtype)
    if points.dim() != 3 or points.shape[2] != 3:
        raise L.InvalidArgumentError("boxes_from_labels: points must have shape (b, n, 3), got %s" % (tuple(points.shape),))
    if not points.is_contiguous():
        raise L.InvalidArgumentError("boxes_from_labels: points must be contiguous")
    dev = points.device
    b, n = int(points.shape[0]), int(points.shape[1])
    if not 1 <= b <= 65535 or not 1 <= n < 2 ** 24:
        raise L.InvalidArgumentError("boxes_from_labels: 1 <= b <= 65535 and 1 <= n < 2^24, got points of shape %s" % (tuple(points.shape),))
    instance = _labels(instance, "instance", (b, n), dev)
    semantic = _labels(semantic, "semantic", (b, n), dev)
    if not torch.is_tensor(class_map):
        cm = np.asarray(class_map)
        if cm.dtype.kind not in "iu" or cm.ndim != 1:
            raise L.InvalidArgumentError("boxes_from_labels: class_map must be a 1-D integer array")
        class_map = torch.from_numpy(np.ascontiguousarray(cm, dtype=np.int32)).to(dev)
    if class_map.dim() != 1 or not 1 <= class_map.shape[0] <= MAX_SEM:
        raise L.InvalidArgumentError("boxes_from_labels: class_map must hold 1 to %d labels, got shape %s" % (MAX_SEM, tuple(class_map.shape)))
    class_map = _labels(class_map, "class_map", tuple(class_map.shape), dev)
    k = _int(k, "k", 1, MAX_K)
    n_class = _int(n_class, "n_class", 0)
    min_points = _int(min_points, "min_points", 1)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    center, size, heading = f64(b * k, 3), f64(b * k, 3), f64(b * k)
    cls, instance_id, n_points = i32(b * k), i32(b * k), i32(b * k)
    kept, slot, status, inst_count, ignored = i32(b), i32(b, k), i32(b, k), i32(b, k), i32(b, 3)
    S = L.side_lib("instbox")
    wsb = int(S.votenet_instance_boxes_workspace_bytes(b, k))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    point_box = i32(b, n) if want_point_box else None
    with L.device_guard(dev):
        L.check(S.votenet_instance_boxes(b, n, k, class_map.shape[0], n_class, min_points, L.ptr(points), L.ptr(instance), L.ptr(semantic),
                                         L.ptr(class_map), L.ptr(center), L.ptr(size), L.ptr(heading), L.ptr(cls), L.ptr(instance_id),
                                         L.ptr(n_points), L.ptr(kept), L.ptr(slot), L.ptr(status), L.ptr(inst_count), L.ptr(ignored),
                                         L.ptr(ws), wsb, L.stream_ptr()), side="instbox")
        if want_point_box:
            L.check(S.votenet_instance_point_box(b, n, k, L.ptr(points), L.ptr(instance), L.ptr(slot), L.ptr(point_box), L.stream_ptr()),
                    side="instbox")
    box_offset = np.zeros(b + 1, np.int64)
    box_offset[1:] = np.cumsum(kept.cpu().numpy())  # (waits for the stream: the workspace may go)
    nk = int(box_offset[-1])
    res = {"center": center[:nk], "size": size[:nk], "heading": heading[:nk], "cls": cls[:nk], "box_offset": box_offset,
           "instance_id": instance_id[:nk], "n_points": n_points[:nk], "status": status, "inst_count": inst_count, "slot": slot,
           "ignored": ignored}
    if want_point_box:
        res["point_box"] = point_box
    return res
