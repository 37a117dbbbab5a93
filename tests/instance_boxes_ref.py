"""The rule of include/votenet_instance_boxes.h restated in numpy: ground-truth boxes from instance-labelled points.

Minimum, maximum, count and first index are exact and the same in any order; the rows' arithmetic is two float64 operations on exactly
converted float32 values.  So the device result is held to these arrays by bit pattern (float64 viewed as int64)."""
import numpy as np

F = np.float32
ROW_KEYS = ("center", "size", "heading", "cls", "instance_id", "n_points")
TABLE_KEYS = ("status", "inst_count", "slot", "ignored")


def takes_part(points, instance, k):
    """-> (mask (b, n) of the points that take part, ignored (b, 3) int32: unlabelled, id out of the table, non-finite -- a point is
    counted by the first of the three tests that holds)."""
    instance = np.asarray(instance, np.int32)
    finite = np.isfinite(np.asarray(points, F)).all(-1)
    unlabelled = instance < 0
    outside = ~unlabelled & (instance >= k)
    nonfinite = ~unlabelled & ~outside & ~finite
    ignored = np.stack([unlabelled.sum(1), outside.sum(1), nonfinite.sum(1)], 1).astype(np.int32)
    return ~(unlabelled | outside | nonfinite), ignored


def boxes_from_labels(points, instance, semantic, class_map, k=256, n_class=10, min_points=1):
    """points (b, n, 3) float32, instance, semantic (b, n) int32, class_map (n_sem) int32 -> dict of numpy arrays with the keys and the
    layout of votenet_amd.instance_boxes.boxes_from_labels (want_point_box=True)."""
    points = np.asarray(points, F)
    instance, semantic, class_map = (np.asarray(a, np.int32) for a in (instance, semantic, class_map))
    b, n = instance.shape
    part, ignored = takes_part(points, instance, k)
    xyz = points + F(0.0)  # -0 takes part as +0
    rows = {key: [] for key in ROW_KEYS}
    status = np.full((b, k), 3, np.int32)
    inst_count = np.zeros((b, k), np.int32)
    slot = np.full((b, k), -1, np.int32)
    kept = np.zeros(b, np.int64)
    for s in range(b):
        ids = np.where(part[s], instance[s], -1)
        inst_count[s] = np.bincount(ids[ids >= 0], minlength=k)[:k]
        for i in np.nonzero(inst_count[s])[0]:
            idx = np.nonzero(ids == i)[0]
            sem = int(semantic[s, idx[0]])  # the label of the lowest-index point decides
            cls = int(class_map[sem]) if 0 <= sem < len(class_map) else -1
            if cls < 0 or cls >= n_class:
                status[s, i] = 1
            elif len(idx) < min_points:
                status[s, i] = 2
            else:
                status[s, i] = 0
                lo, hi = xyz[s, idx].min(0).astype(np.float64), xyz[s, idx].max(0).astype(np.float64)
                slot[s, i] = kept[s]
                kept[s] += 1
                rows["center"].append((lo + hi) * 0.5)
                rows["size"].append(hi - lo)
                rows["heading"].append(0.0)
                rows["cls"].append(cls)
                rows["instance_id"].append(i)
                rows["n_points"].append(len(idx))
    nk = int(kept.sum())
    out = {"center": np.array(rows["center"], np.float64).reshape(nk, 3), "size": np.array(rows["size"], np.float64).reshape(nk, 3),
           "heading": np.array(rows["heading"], np.float64).reshape(nk)}
    for key in ("cls", "instance_id", "n_points"):
        out[key] = np.array(rows[key], np.int32).reshape(nk)
    out["box_offset"] = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    out.update(status=status, inst_count=inst_count, slot=slot, ignored=ignored)
    safe = np.clip(instance, 0, k - 1)
    out["point_box"] = np.where(part, np.take_along_axis(slot, safe, 1), -1).astype(np.int32)
    return out


def bits(a):
    """float64 as int64, so that -0.0 / +0.0 and NaN payloads compare as bytes; integers as they are."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bytes(got, exp, keys=None):
    """The keys (default: all of exp) on which two result dicts differ in dtype, shape or bit pattern."""
    bad = []
    for key in (keys or exp):
        g, e = np.asarray(got[key]), np.asarray(exp[key])
        if g.dtype != e.dtype or g.shape != e.shape or not np.array_equal(bits(g), bits(e)):
            bad.append(key)
    return bad
