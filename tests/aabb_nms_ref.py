"""Host restatement (numpy float32) of include/votenet_aabb_nms.h: the box rule and the overlap rule, operation for operation and in
the header's order, so that a comparison with the device is bit for bit.  The NMS itself is not restated here: it is
tests/detections_ref.class_nms3d over the table this module (or the device) writes."""
import numpy as np

F = np.float32
MODES = ("aabb3d", "bev")
MEASURES = ("iou", "over_later")


def extents(boxes):
    """(..., 8, 3) -> lo, hi (..., 3): over corners 0..7 in corner order, a NaN sticky."""
    c = np.asarray(boxes, F)
    lo, hi = c[..., 0, :].copy(), c[..., 0, :].copy()
    with np.errstate(invalid="ignore"):
        for t in range(1, 8):
            ct = c[..., t, :]
            nan = ct != ct
            lo = np.where((ct < lo) | nan, ct, lo)
            hi = np.where((ct > hi) | nan, ct, hi)
    return lo, hi


def sizes(lo, hi, mode):
    """v = (e_x e_y) e_z, or e_x e_z for the bird's-eye rectangle (x, z)."""
    with np.errstate(all="ignore"):
        e = (hi - lo).astype(F)
        if mode == "bev":
            return (e[..., 0] * e[..., 2]).astype(F)
        return ((e[..., 0] * e[..., 1]).astype(F) * e[..., 2]).astype(F)


def overlap_table(boxes, mode="aabb3d", measure="iou"):
    """(B, N, 8, 3) -> (B, N, N) float32, [s][later j][earlier i]."""
    assert mode in MODES and measure in MEASURES
    lo, hi = extents(boxes)
    v = sizes(lo, hi, mode)
    loj, hij, loi, hii = lo[:, :, None], hi[:, :, None], lo[:, None, :], hi[:, None, :]
    with np.errstate(all="ignore"):
        t = (np.where(hij < hii, hij, hii) - np.where(loj < loi, loi, loj)).astype(F)
        side = np.where(t > 0, t, F(0)).astype(F)
        if mode == "bev":
            inter = (side[..., 0] * side[..., 2]).astype(F)
        else:
            inter = ((side[..., 0] * side[..., 1]).astype(F) * side[..., 2]).astype(F)
        vj, vi = v[:, :, None], v[:, None, :]
        if measure == "over_later":
            return (inter / vj).astype(F)
        return (inter / ((vj + vi).astype(F) - inter).astype(F)).astype(F)
