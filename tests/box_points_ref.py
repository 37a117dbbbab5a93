"""Host restatement (numpy float32, operation for operation) of include/votenet_box_points.h: the points inside each box by the
closed analytic rule, their counts, and the objectness gate.  Every product and sum below is one float32 operation in the header's
order (numpy does not fuse them), so the integers equal the device's bit for bit."""
import numpy as np

F = np.float32


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz  # (x + y) + z, un-fused


def box_constants(boxes):
    """(..., 8, 3) -> c0 (..., 3), e (3, ..., 3) [width, length, height axis], ee (3, ...), all float32."""
    boxes = np.asarray(boxes, F)
    with np.errstate(all="ignore"):
        c0 = boxes[..., 0, :]
        e = np.stack([boxes[..., 1, :] - c0, boxes[..., 3, :] - c0, boxes[..., 4, :] - c0])
        ee = _dot(e[..., 0], e[..., 1], e[..., 2], e[..., 0], e[..., 1], e[..., 2])
    assert c0.dtype == F and e.dtype == F and ee.dtype == F
    return c0, e, ee


def projections(boxes, points):
    """boxes (N, 8, 3), points (P, 3) -> t (3, N, P) float32, ee (3, N) float32."""
    c0, e, ee = box_constants(boxes)
    p = np.asarray(points, F)
    with np.errstate(all="ignore"):
        q = p[None, :, :] - c0[:, None, :]  # (N, P, 3)
        t = np.stack([_dot(q[..., 0], q[..., 1], q[..., 2], e[k][:, None, 0], e[k][:, None, 1], e[k][:, None, 2]) for k in range(3)])
    assert t.dtype == F
    return t, ee


def inside(boxes, points):
    """boxes (N, 8, 3), points (P, 3) -> (N, P) bool: t_k >= 0 and t_k <= ee_k for the three axes; a NaN fails."""
    t, ee = projections(boxes, points)
    with np.errstate(invalid="ignore"):
        return ((t >= 0) & (t <= ee[:, :, None])).all(0)


def counts(bboxes, points):
    """bboxes (B, N, 8, 3), points (B, P, 3) -> (B, N) int32."""
    bboxes, points = np.asarray(bboxes, F), np.asarray(points, F)
    out = np.zeros(bboxes.shape[:2], np.int32)
    for s in range(bboxes.shape[0]):
        if points.shape[1]:
            out[s] = inside(bboxes[s], points[s]).sum(1)
    return out


def near_face(boxes, points, rel=1e-5):
    """(N, P) bool: some t_k lies within rel * max(ee_k, 1) of 0 or of ee_k -- where a hull test in float64 and this rule in float32
    cannot be held to agree."""
    t, ee = projections(boxes, points)
    tol = rel * np.maximum(ee.astype(np.float64), 1.0)[:, :, None]
    t = t.astype(np.float64)
    return ((np.abs(t) <= tol) | (np.abs(t - ee.astype(np.float64)[:, :, None]) <= tol)).any(0)


def gate(objectness, cnt, min_points):
    """(B, N, 2) float32, (B, N) int -> the logits where cnt >= min_points, the quiet NaN 0x7fc00000 elsewhere."""
    out = np.array(objectness, F, copy=True)
    out.view(np.uint32)[np.asarray(cnt) < min_points] = 0x7fc00000
    return out
