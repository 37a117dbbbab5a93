"""Host mirror of the reference's input pipeline for the step before the hot path.

The reference builds every training sample in numpy inside MyDataFlow.__iter__ (dataset.py:183-189 random subsample to
config.POINT_NUM points + depth->camera axes, :219-231 the augmentation draws, :262-276 the box side, :302-308 the point
side) and pads the ragged ground truth in BatchData2Biggest (run.py:14-24,60-64).  Here the DRAWS stay on the host, in the
reference's order, and the work is two kernels over the whole batch (votenet_subsample_augment, votenet_augment_boxes).
Which labelled objects a scene trains on (dataset.py:237-283,300: image frustum, 3D box, at least 5 points) is decided on
the device too (votenet_select_boxes); build_batch chains the three from parsed scene files (sunrgbd.py) to the model's inputs.
Scenes without annotated boxes -- an instance id and a semantic label per point -- go through build_batch_from_labels, whose boxes are
the extents of the instances in the augmented points (instance_boxes.py; beyond the reference).
There is no CPU path: without libvotenet_hip.so these functions raise.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .synth import MEAN_SIZES, NH

POINT_NUM = 20480  # config.py:1


class Augmentation:
    """Per-scene draws of dataset.py:219-231: flip_x, flip_z (bools), angle (rad), scale; float64 like numpy."""

    def __init__(self, flip_x, flip_z, angle, scale):
        self.flip_x = np.ascontiguousarray(flip_x, dtype=bool)
        self.flip_z = np.ascontiguousarray(flip_z, dtype=bool)
        self.angle = np.ascontiguousarray(angle, dtype=np.float64)
        self.scale = np.ascontiguousarray(scale, dtype=np.float64)
        self.b = len(self.angle)

    def host_arrays(self):
        flip = (self.flip_x.astype(np.int32) | (self.flip_z.astype(np.int32) << 1)).astype(np.int32)
        return flip, self.angle, np.cos(self.angle), np.sin(self.angle), self.scale  # np.cos / np.sin: sunutils.py:135-136


def draw_augmentation(b, rand=np.random):
    """The four np.random.rand() draws per scene in the reference's order (dataset.py:219-231)."""
    fx, fz, ang, sc = [], [], [], []
    for _ in range(b):
        fx.append(rand.rand() > 0.5)
        fz.append(rand.rand() > 0.5)
        ang.append((rand.rand() * 2 - 1.) * 5. / 180 * np.pi)
        sc.append((rand.rand() * 2 - 1.) * 0.1 + 1.)
    return Augmentation(fx, fz, ang, sc)


def draw_choice(rng, n_raw, n_out=POINT_NUM):
    """dataset.py:185-186: self.rng.choice(n, POINT_NUM, replace=False) per scene -> (b, n_out) int32."""
    return np.stack([rng.choice(int(n), n_out, replace=False) for n in n_raw]).astype(np.int32)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def pack_ragged(arrays, device, dtype=None):
    """list of per-scene (n_s, ...) arrays -> (device tensor of the concatenation, host int64 offsets (b+1))."""
    off = np.zeros(len(arrays) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    cat = np.ascontiguousarray(np.concatenate(arrays, 0))
    if dtype is not None:
        cat = cat.astype(dtype, copy=False)
    return torch.from_numpy(cat).to(device), off


def subsample_augment(raw, raw_offset, n_out=POINT_NUM, aug=None, choice=None, seed=0, scene0=0, depth_to_camera=True):
    """raw: device tensor (sum n_s, stride) float32 or float64 in upright-depth coordinates (or already camera frame with
    depth_to_camera=False); raw_offset: host int64 (b+1).  choice: (b, n_out) int32 (host or device) -- the caller's
    rng.choice -- or None: the device draws a keyed permutation (seed, scene0 + s).  aug: Augmentation or None (evaluation).
    -> (b, n_out, 3) float32 device tensor: the `points` input of model.py:22."""
    if raw.dim() != 2 or raw.dtype not in (torch.float32, torch.float64) or not raw.is_cuda:
        raise L.InvalidArgumentError("subsample_augment: raw must be a 2-D float32 / float64 device tensor")
    raw = raw.contiguous()
    off = np.ascontiguousarray(raw_offset, dtype=np.int64)
    b = len(off) - 1
    if off[0] < 0 or off[-1] > raw.shape[0] or np.any(np.diff(off) < 0):
        raise L.InvalidArgumentError("subsample_augment: raw_offset does not describe rows of raw")
    if aug is not None and aug.b != b:
        raise L.InvalidArgumentError("subsample_augment: %d scenes but %d augmentation draws" % (b, aug.b))
    ch = None
    if choice is not None:
        if tuple(choice.shape) != (b, n_out):
            raise L.InvalidArgumentError("subsample_augment: choice must be (b, n_out)")
        if torch.is_tensor(choice) and choice.is_cuda:  # already on the device: not read back (the kernel clamps the index)
            ch = choice.to(torch.int32).contiguous()
        else:
            chn = np.asarray(choice)
            if np.any(chn < 0) or np.any(chn >= np.diff(off)[:, None]):
                raise L.InvalidArgumentError("subsample_augment: choice index out of range")
            ch = torch.from_numpy(np.ascontiguousarray(chn, dtype=np.int32)).to(raw.device)
    out = torch.empty((b, n_out, 3), dtype=torch.float32, device=raw.device)
    flip = ang = c = s = sc = None
    if aug is not None:
        flip, ang, c, s, sc = aug.host_arrays()
    with L.device_guard(raw.device):
        L.check(L.lib().votenet_subsample_augment(b, n_out, L.ptr(raw), 1 if raw.dtype == torch.float64 else 0, raw.shape[1], _hp(off),
                                                  L.ptr(ch), int(seed) & (2 ** 64 - 1), int(scene0), 1 if depth_to_camera else 0,
                                                  _hp(flip), _hp(c), _hp(s), _hp(sc), L.ptr(out), L.stream_ptr()))
    return out


def subsample_augment_features(raw, raw_offset, n_out=POINT_NUM, aug=None, choice=None, seed=0, scene0=0, depth_to_camera=True,
                               height=True, extra_cols=0, order_stats=None):
    """subsample_augment plus the input features of a network built with point_features = height + extra_cols (beyond the reference,
    which drops the colour, dataset.py:310): the same points bit for bit, feats (b, n_out, c) = [height above the scene's floor | raw
    columns 3 .. 3+extra_cols of the rows the points came from, rounded to float, un-augmented], floor (b) float32 -- the
    np.percentile(-y, 0.99) of the OUTPUT points of each scene (votenet_subsample_augment_features); None without height.
    order_stats: None, or a (b, 2) float32 device tensor that receives the two order statistics the floor interpolates (tests).
    -> (points, feats, floor), all on the device; nothing is read back."""
    raw, off, b, ch = _check_raw(raw, raw_offset, n_out, choice, "subsample_augment_features")
    if aug is not None and aug.b != b:
        raise L.InvalidArgumentError("subsample_augment_features: %d scenes but %d augmentation draws" % (b, aug.b))
    want_height, extra_cols = (1 if height else 0), int(extra_cols)
    c = want_height + extra_cols
    if not 0 <= extra_cols <= 4 or not 1 <= c <= 5:
        raise L.InvalidArgumentError("subsample_augment_features: height + extra_cols must be in [1, 5] with extra_cols in [0, 4], "
                                     "got height=%r, extra_cols=%d" % (bool(height), extra_cols))
    if 3 + extra_cols > raw.shape[1]:
        raise L.InvalidArgumentError("subsample_augment_features: extra_cols = %d needs raw rows of %d elements, raw has %d"
                                     % (extra_cols, 3 + extra_cols, raw.shape[1]))
    out = torch.empty((b, n_out, 3), dtype=torch.float32, device=raw.device)
    feats = torch.empty((b, n_out, c), dtype=torch.float32, device=raw.device)
    floor = torch.empty((b,), dtype=torch.float32, device=raw.device) if want_height else None
    if order_stats is not None and (order_stats.dtype != torch.float32 or tuple(order_stats.shape) != (b, 2) or order_stats.device != raw.device
                                    or not order_stats.is_contiguous()):
        raise L.InvalidArgumentError("subsample_augment_features: order_stats must be a contiguous (b, 2) float32 tensor on raw's device")
    flip = c_ = s = sc = None
    if aug is not None:
        flip, _, c_, s, sc = aug.host_arrays()
    with L.device_guard(raw.device):
        L.check(L.side_lib("features").votenet_subsample_augment_features(b, n_out, L.ptr(raw), 1 if raw.dtype == torch.float64 else 0, raw.shape[1],
                                                           _hp(off), L.ptr(ch), int(seed) & (2 ** 64 - 1), int(scene0),
                                                           1 if depth_to_camera else 0, _hp(flip), _hp(c_), _hp(s), _hp(sc), want_height,
                                                           extra_cols, L.ptr(out), L.ptr(feats), L.ptr(floor), L.ptr(order_stats),
                                                           L.stream_ptr()), side="features")
    return out, feats, floor


GT_FIELDS = (("bboxes_xyz", 3, torch.float32), ("bboxes_lwh", 3, torch.float32), ("bboxes_roty", 0, torch.float32),
             ("semantic_labels", 0, torch.int32), ("heading_labels", 0, torch.int32), ("heading_residuals", 0, torch.float32),
             ("size_labels", 0, torch.int32), ("size_residuals", 3, torch.float32))


def augment_boxes(center, size, heading, cls, box_offset, aug=None, mean_size=MEAN_SIZES, nh=NH):
    """center (nbox,3), size (nbox,3), heading (nbox) float64 and cls (nbox) int32 device tensors in the upright-camera
    frame (dataset.py:253-259), box_offset host int64 (b+1).  -> dict of the eight ground-truth inputs of model.py:23-32 on
    the device, every scene padded to the longest by repeating its last box (run.py:14-24)."""
    off = np.ascontiguousarray(box_offset, dtype=np.int64)
    b = len(off) - 1
    cnt = np.diff(off)
    if b < 1 or np.any(cnt < 1):
        raise L.InvalidArgumentError("augment_boxes: every scene needs at least one box (dataset.py:300 skips the others)")
    if aug is not None and aug.b != b:
        raise L.InvalidArgumentError("augment_boxes: %d scenes but %d augmentation draws" % (b, aug.b))
    dev = center.device
    center, size, heading = (t.to(torch.float64).contiguous() for t in (center, size, heading))
    cls = cls.to(torch.int32).contiguous()
    if off[-1] > center.shape[0] or center.shape != size.shape or heading.shape[0] != center.shape[0] or cls.shape[0] != center.shape[0]:
        raise L.InvalidArgumentError("augment_boxes: box arrays do not match box_offset")
    bb = int(cnt.max())
    ms = np.ascontiguousarray(mean_size, dtype=np.float64)
    out = {k: torch.empty((b, bb, w) if w else (b, bb), dtype=dt, device=dev) for k, w, dt in GT_FIELDS}
    flip = ang = c = s = sc = None
    if aug is not None:
        flip, ang, c, s, sc = aug.host_arrays()
    with L.device_guard(dev):
        L.check(L.lib().votenet_augment_boxes(b, bb, _hp(off), L.ptr(center), L.ptr(size), L.ptr(heading), L.ptr(cls), _hp(flip),
                                              _hp(ang), _hp(c), _hp(s), _hp(sc), _hp(ms), ms.shape[0], nh,
                                              *[L.ptr(out[k]) for k, _, _ in GT_FIELDS], L.stream_ptr()))
    return out


def _calib_arrays(calib, b, what):
    """calib: (Rtilt (b,3,3), K (b,3,3)) or a list of b (Rtilt, K) pairs (sunrgbd.parse_calib) -> two host (b,9) float64."""
    if isinstance(calib, (list,)) or (isinstance(calib, tuple) and len(calib) and isinstance(calib[0], (tuple, list))):
        if len(calib) != b:
            raise L.InvalidArgumentError("%s: %d scenes but %d calibrations" % (what, b, len(calib)))
        calib = (np.stack([np.asarray(c[0], np.float64) for c in calib]), np.stack([np.asarray(c[1], np.float64) for c in calib]))
    rt, km = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1, 9) for a in calib)
    if rt.shape[0] != b or km.shape[0] != b:
        raise L.InvalidArgumentError("%s: %d scenes but %d / %d calibrations" % (what, b, rt.shape[0], km.shape[0]))
    return rt, km


def _check_raw(raw, raw_offset, n_out, choice, what):
    """The argument checks subsample_augment makes, for the entries that pick the same rows.  -> (raw, off, b, choice tensor)."""
    if not torch.is_tensor(raw) or raw.dim() != 2 or raw.dtype not in (torch.float32, torch.float64) or not raw.is_cuda:
        raise L.InvalidArgumentError("%s: raw must be a 2-D float32 / float64 device tensor" % what)
    raw = raw.contiguous()
    off = np.ascontiguousarray(raw_offset, dtype=np.int64)
    b = len(off) - 1
    if b < 1 or off[0] < 0 or off[-1] > raw.shape[0] or np.any(np.diff(off) < 0):
        raise L.InvalidArgumentError("%s: raw_offset does not describe rows of raw" % what)
    ch = None
    if choice is not None:
        if tuple(choice.shape) != (b, n_out):
            raise L.InvalidArgumentError("%s: choice must be (b, n_out)" % what)
        if torch.is_tensor(choice) and choice.is_cuda:  # already on the device: not read back (the kernel clamps the index)
            ch = choice.to(torch.int32).contiguous()
        else:
            chn = np.asarray(choice)
            if np.any(chn < 0) or np.any(chn >= np.diff(off)[:, None]):
                raise L.InvalidArgumentError("%s: choice index out of range" % what)
            ch = torch.from_numpy(np.ascontiguousarray(chn, dtype=np.int32)).to(raw.device)
    return raw, off, b, ch


_OBJECT_KEYS = (("cls", 0, torch.int32), ("box2d", 4, torch.float64), ("centroid", 3, torch.float64),
                ("half_extent", 3, torch.float64), ("heading", 0, torch.float64))


def select_boxes(raw, raw_offset, calib, objects, n_out=POINT_NUM, choice=None, seed=0, scene0=0, want_inside=False):
    """Which labelled objects become ground truth (dataset.py:237-283): whitelisted, not degenerate, at least 5 of the
    subsampled points inside both the 2D box's frustum and the 3D box.  raw, raw_offset, n_out, choice, seed, scene0 as for
    subsample_augment: the points tested are the rows it picks, un-augmented, upright-depth.  calib: (Rtilt (b,3,3),
    K (b,3,3)) or a list of (Rtilt, K) pairs.  objects: sunrgbd.pack_objects' dict (host arrays or device tensors: cls,
    box2d, centroid, half_extent, heading; host obj_offset (b+1)).
    -> dict: center (nkept,3), size (nkept,3), heading (nkept) float64 and cls (nkept) int32 device tensors, in label order
    -- what augment_boxes takes; box_offset host int64 (b+1), the one read-back; n_inside, status (one per input object,
    device int32; 0 kept, 1 not whitelisted, 2 degenerate, 3 fewer than 5 points); inside (objects, n_out) uint8 if asked."""
    raw, off, b, ch = _check_raw(raw, raw_offset, n_out, choice, "select_boxes")
    if np.any(np.diff(off) < n_out):
        raise L.InvalidArgumentError("select_boxes: a scene has fewer than n_out = %d points" % n_out)
    rt, km = _calib_arrays(calib, b, "select_boxes")
    ooff = np.ascontiguousarray(objects["obj_offset"], dtype=np.int64)
    if len(ooff) != b + 1 or ooff[0] != 0 or np.any(np.diff(ooff) < 0):
        raise L.InvalidArgumentError("select_boxes: obj_offset must have b + 1 = %d non-decreasing entries from 0" % (b + 1))
    n_obj = int(ooff[-1])
    dev = raw.device
    obj = {}
    for k, w, dt in _OBJECT_KEYS:
        t = objects[k]
        t = (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))).to(device=dev, dtype=dt).contiguous()
        if tuple(t.shape) != ((n_obj, w) if w else (n_obj,)):
            raise L.InvalidArgumentError("select_boxes: objects[%r] has shape %s, obj_offset describes %d objects"
                                         % (k, tuple(t.shape), n_obj))
        obj[k] = t
    center = torch.empty((n_obj, 3), dtype=torch.float64, device=dev)
    size = torch.empty((n_obj, 3), dtype=torch.float64, device=dev)
    heading = torch.empty((n_obj,), dtype=torch.float64, device=dev)
    cls = torch.empty((n_obj,), dtype=torch.int32, device=dev)
    kept = torch.empty((b,), dtype=torch.int32, device=dev)
    n_inside = torch.empty((n_obj,), dtype=torch.int32, device=dev)
    status = torch.empty((n_obj,), dtype=torch.int32, device=dev)
    inside = torch.empty((n_obj, n_out), dtype=torch.uint8, device=dev) if want_inside else None
    wsb = int(L.lib().votenet_select_boxes_workspace_bytes(b, n_obj))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    with L.device_guard(dev):
        L.check(L.lib().votenet_select_boxes(b, n_out, L.ptr(raw), 1 if raw.dtype == torch.float64 else 0, raw.shape[1], _hp(off),
                                             L.ptr(ch), int(seed) & (2 ** 64 - 1), int(scene0), _hp(rt), _hp(km), _hp(ooff),
                                             *[L.ptr(obj[k]) for k, _, _ in _OBJECT_KEYS], L.ptr(center), L.ptr(size),
                                             L.ptr(heading), L.ptr(cls), L.ptr(kept), L.ptr(n_inside), L.ptr(status),
                                             L.ptr(inside), L.ptr(ws), wsb, L.stream_ptr()))
    box_offset = np.zeros(b + 1, np.int64)
    box_offset[1:] = np.cumsum(kept.cpu().numpy())
    nk = int(box_offset[-1])
    res = {"center": center[:nk], "size": size[:nk], "heading": heading[:nk], "cls": cls[:nk], "box_offset": box_offset,
           "n_inside": n_inside, "status": status}
    if want_inside:
        res["inside"] = inside
    return res


def build_batch(raw, raw_offset, calib, objects, aug=None, choice=None, seed=0, scene0=0, n_out=POINT_NUM, height=False, extra_cols=0,
                head=None):
    """Parsed scenes -> model inputs: select_boxes, then subsample_augment and augment_boxes with the same choice / seed for
    the scenes that kept at least one box (the reference skips the others, dataset.py:300).  aug holds one draw per INPUT
    scene: the reference draws before it looks at the objects (dataset.py:219-231), so a dropped scene consumes its draw.
    -> (points (k, n_out, 3) float32, gt dict of augment_boxes, scene_index host int64 (k)); (None, None, empty) when every
    scene is dropped.  height / extra_cols (subsample_augment_features): the dict also holds "features" (k, n_out, c), the input
    features of a network built with point_features = c, and the points come from that entry (the same bits); the boxes are
    selected on the same un-augmented rows either way.  head: the HeadConfig whose heading bins and size templates encode the labels
    (None: the default head's, as augment_boxes' own defaults)."""
    b = len(raw_offset) - 1
    if aug is not None and aug.b != b:
        raise L.InvalidArgumentError("build_batch: %d scenes but %d augmentation draws" % (b, aug.b))
    sel = select_boxes(raw, raw_offset, calib, objects, n_out, choice, seed, scene0)
    cnt = np.diff(sel["box_offset"])
    scene_index = np.nonzero(cnt > 0)[0].astype(np.int64)
    if len(scene_index) == 0:
        return None, None, scene_index
    # every input scene goes through the point kernel with its own rows and its own draw; the dropped ones are left out after
    feats = None
    if height or extra_cols:
        points, feats, _ = subsample_augment_features(raw, raw_offset, n_out, aug, choice, seed, scene0, height=height, extra_cols=extra_cols)
    else:
        points = subsample_augment(raw, raw_offset, n_out, aug, choice, seed, scene0)
    if len(scene_index) < b:
        keep = torch.from_numpy(scene_index).to(points.device)
        points = points[keep]
        feats = feats[keep] if feats is not None else None
        if aug is not None:
            aug = Augmentation(aug.flip_x[scene_index], aug.flip_z[scene_index], aug.angle[scene_index], aug.scale[scene_index])
    box_offset = np.concatenate([[0], np.cumsum(cnt[scene_index])]).astype(np.int64)
    gt = augment_boxes(sel["center"], sel["size"], sel["heading"], sel["cls"], box_offset, aug, **_head_kw(head))
    if feats is not None:
        gt["features"] = feats
    return points, gt, scene_index


def _head_kw(head):
    """augment_boxes' mean_size / nh of a HeadConfig; nothing for None (the call as it always was)."""
    if head is None:
        return {}
    from .head import resolve
    return dict(mean_size=head.mean_sizes_f64, nh=resolve(head, 0, 0, 0)[0])


def _ragged_labels(t, total, dev, name):
    """(sum n_s) int32 labels beside raw's rows, host or device -> on the device."""
    t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    if t.dim() != 1 or t.shape[0] != total or t.dtype != torch.int32:
        raise L.InvalidArgumentError("build_batch_from_labels: %s must be %d int32 labels, one per row of raw, got %s %s"
                                     % (name, total, t.dtype, tuple(t.shape)))
    return t.to(dev)


def build_batch_from_labels(raw, raw_offset, instance, semantic, class_map, choice, aug=None, n_out=POINT_NUM, k=256, min_points=1,
                            height=False, extra_cols=0, point_box=False, head=None):
    """Scenes without annotated boxes -> model inputs: raw, raw_offset, aug, n_out, height, extra_cols as for build_batch; instance,
    semantic (sum n_s) int32, host or device: an instance id (negative: none) and a semantic label per row of raw; class_map (n_sem)
    int32: label -> class of the network, or -1; choice (b, n_out), host or device (draw_choice makes one): the rows
    subsample_augment picks, by which the labels are gathered on the device.  The boxes are the extents of the instances in the
    AUGMENTED points (instance_boxes.boxes_from_labels: ids in [0, k), at least min_points points), so they are axis-aligned in the
    frame the network sees, and augment_boxes encodes them without a draw.
    -> (points, gt, scene_index) with build_batch's contract; a scene that keeps no box is dropped.
    point_box: the dict also holds "point_box" (k, n_out) int32, the row of every point's box within its scene's ground truth, -1 where
    the point has none (one more launch, instance_boxes.boxes_from_labels(want_point_box=True)): what
    VoteNetHotPath.enable_instance_votes() supervises the votes by.  False: the launches and the keys of a call without it.
    head: the HeadConfig of the network the batch is for: class_map maps into its nc classes, its templates and heading bins encode
    the labels (None: the default head)."""
    from . import instance_boxes as IB  # (the only place of this module that loads libvotenet_instbox.so)
    if choice is None:
        raise L.InvalidArgumentError("build_batch_from_labels: choice is required (draw_choice makes one): the labels follow its rows")
    raw, off, b, ch = _check_raw(raw, raw_offset, n_out, choice, "build_batch_from_labels")
    if aug is not None and aug.b != b:
        raise L.InvalidArgumentError("build_batch_from_labels: %d scenes but %d augmentation draws" % (b, aug.b))
    if np.any(np.diff(off) < 1):
        raise L.InvalidArgumentError("build_batch_from_labels: a scene has no points")
    dev = raw.device
    instance = _ragged_labels(instance, raw.shape[0], dev, "instance")
    semantic = _ragged_labels(semantic, raw.shape[0], dev, "semantic")
    feats = None
    if height or extra_cols:
        points, feats, _ = subsample_augment_features(raw, raw_offset, n_out, aug, ch, height=height, extra_cols=extra_cols)
    else:
        points = subsample_augment(raw, raw_offset, n_out, aug, ch)
    # the rows the point kernel reads: raw_offset[s] + the choice clamped into the scene, as the kernel clamps it
    start = torch.from_numpy(off[:-1].copy()).to(dev)[:, None]
    last = torch.from_numpy(np.diff(off) - 1).to(dev)[:, None]
    rows = start + torch.minimum(ch.to(torch.int64).clamp(min=0), last)
    boxes = IB.boxes_from_labels(points, instance[rows], semantic[rows], class_map, k=k, min_points=min_points,
                                 **(dict(want_point_box=True) if point_box else {}), **(dict(head=head) if head is not None else {}))
    rows_of = boxes["point_box"] if point_box else None  # (of the un-dropped batch: a dropped scene's rows are all -1)
    cnt = np.diff(boxes["box_offset"])
    scene_index = np.nonzero(cnt > 0)[0].astype(np.int64)
    if len(scene_index) == 0:
        return None, None, scene_index
    if len(scene_index) < b:
        keep = torch.from_numpy(scene_index).to(dev)
        points = points[keep]
        feats = feats[keep] if feats is not None else None
        rows_of = rows_of[keep] if rows_of is not None else None
    box_offset = np.concatenate([[0], np.cumsum(cnt[scene_index])]).astype(np.int64)  # (the rows are compact: a dropped scene has none)
    gt = augment_boxes(boxes["center"], boxes["size"], boxes["heading"], boxes["cls"], box_offset, None, **_head_kw(head))
    if feats is not None:
        gt["features"] = feats
    if rows_of is not None:  # (augment_boxes keeps the row order and pads at the end: the rows index the padded ground truth)
        gt["point_box"] = rows_of
    return points, gt, scene_index
