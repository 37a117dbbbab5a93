"""A float64 numpy restatement of the reference's ground-truth selection (dataset.py:237-283,300 around sunutils.py:85-99,
199-241) with the closed analytic box test in place of the Delaunay hull, term by term in the order votenet_select_boxes
evaluates it.  Test infrastructure: tests/golden/select_boxes.npz pins it to the reference's own functions."""
import numpy as np

MIN_POINTS = 5        # dataset.py:283
DEGENERATE = 1e-7     # dataset.py:254
KEPT, NOT_WHITELISTED, DEGENERATE_BOX, TOO_FEW = 0, 1, 2, 3
EXCLUDE = 1e-9        # a point closer than this to a box face (normalised) or a 2D-box side (pixels) may be left out of a comparison


def project_to_image(pts, rtilt, k):
    """sunutils.py:79-99 for (n,3) upright-depth points -> u, v."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    d0 = rtilt[0, 0] * x + rtilt[1, 0] * y + rtilt[2, 0] * z       # R^T p
    d1 = rtilt[0, 1] * x + rtilt[1, 1] * y + rtilt[2, 1] * z
    d2 = rtilt[0, 2] * x + rtilt[1, 2] * y + rtilt[2, 2] * z
    c0, c1, c2 = d0, -d2, d1                                        # flip_axis_to_camera
    uv0 = k[0, 0] * c0 + k[0, 1] * c1 + k[0, 2] * c2
    uv1 = k[1, 0] * c0 + k[1, 1] * c1 + k[1, 2] * c2
    uv2 = k[2, 0] * c0 + k[2, 1] * c1 + k[2, 2] * c2
    with np.errstate(divide="ignore", invalid="ignore"):
        return uv0 / uv2, uv1 / uv2


def box_corners_upright_camera(centroid, half_extent, heading):
    """compute_box_3d (sunutils.py:212-241) then flip_axis_to_camera -> (8,3), and the rotation's cos / sin."""
    t = -1 * heading
    c, s = np.cos(t), np.sin(t)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    l, w, h = half_extent
    xs = np.array([-l, l, l, -l, -l, l, l, -l])
    ys = np.array([w, w, -w, -w, w, w, -w, -w])
    zs = np.array([h, h, h, h, -h, -h, -h, -h])
    p = [(R[a, 0] * xs + R[a, 1] * ys + R[a, 2] * zs) + centroid[a] for a in range(3)]
    return np.stack([p[0], -p[2], p[1]], 1), c, s


def select_scene(pts, rtilt, k, cls, box2d, centroid, half_extent, heading):
    """One scene: pts (n,3) float64 upright-depth rows AFTER the subsample.  -> dict: inside (nobj, n) bool, n_inside, status,
    kept (indices, label order), center / size / heading / cls of the kept ones, and `margin` (nobj, n): how far each point
    is from changing its answer (min of the normalised distance to a box face and the pixel distance to a 2D-box side)."""
    pts = np.asarray(pts, np.float64)[:, :3]
    n, nobj = len(pts), len(cls)
    u, v = project_to_image(pts, rtilt, k)
    inside = np.zeros((nobj, n), bool)
    margin = np.full((nobj, n), np.inf)
    n_inside = np.zeros(nobj, np.int32)
    status = np.zeros(nobj, np.int32)
    centers = np.zeros((nobj, 3))
    for o in range(nobj):
        corners, c, s = box_corners_upright_camera(centroid[o], half_extent[o], heading[o])
        centers[o] = (corners[0] + corners[6]) / 2                                   # dataset.py:259
        if cls[o] < 0:
            status[o] = NOT_WHITELISTED
            continue
        if np.max(corners[:, 1]) - np.min(corners[:, 1]) < DEGENERATE:
            status[o] = DEGENERATE_BOX
            continue
        xmin, ymin, xmax, ymax = box2d[o]
        fov = (u < xmax) & (u >= xmin) & (v < ymax) & (v >= ymin)                    # dataset.py:243-244
        dx, dy, dz = pts[:, 0] - centroid[o][0], pts[:, 1] - centroid[o][1], pts[:, 2] - centroid[o][2]
        lx = c * dx + s * dy
        ly = -s * dx + c * dy
        ext = np.abs(half_extent[o])
        inside[o] = fov & (np.abs(lx) <= ext[0]) & (np.abs(ly) <= ext[1]) & (np.abs(dz) <= ext[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            face = np.minimum.reduce([np.abs(np.abs(lx) - ext[0]) / ext[0], np.abs(np.abs(ly) - ext[1]) / ext[1],
                                      np.abs(np.abs(dz) - ext[2]) / ext[2]])
            side = np.minimum.reduce([np.abs(u - xmin), np.abs(u - xmax), np.abs(v - ymin), np.abs(v - ymax)])
        margin[o] = np.fmin(face, side)
        n_inside[o] = inside[o].sum()
        status[o] = TOO_FEW if n_inside[o] < MIN_POINTS else KEPT
    kept = np.nonzero(status == KEPT)[0]
    return {"inside": inside, "n_inside": n_inside, "status": status, "kept": kept, "margin": margin, "center": centers[kept],
            "size": 2 * np.asarray(half_extent, np.float64).reshape(-1, 3)[kept], "heading": np.asarray(heading, np.float64)[kept],
            "cls": np.asarray(cls, np.int32)[kept]}
