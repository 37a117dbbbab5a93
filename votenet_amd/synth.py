"""Synthetic SUN RGB-D-like scenes (the dataset is not available).

"room" generator: 60 % of the points on the floor and two walls of a 5 x 5 x 3 m room (y up,
camera at the origin looking +z: the upright-camera frame of dataset.py:188), 40 % on the
surfaces of 6-10 random upright boxes with SUN RGB-D class mean sizes (dataset.py:36-45),
plus N(0, 5 mm) noise.  Deterministic per (seed, scene).
"""
import numpy as np

# type_mean_size of the ten SUN RGB-D classes (l, w, h), dataset.py:36-45
MEAN_SIZES = np.array([[2.114256, 1.620300, 0.927272], [0.791118, 1.279516, 0.718182], [0.923508, 1.867419, 0.845495],
                       [0.591958, 0.552978, 0.827272], [0.699104, 0.454178, 0.75625], [0.69519, 1.346299, 0.736364],
                       [0.528526, 1.002642, 1.172878], [0.500618, 0.632163, 0.683424], [0.404671, 1.071108, 1.688889],
                       [0.76584, 1.398258, 0.472728]], dtype=np.float64)


def room_head(nh, nc):
    """A deterministic head for the synthetic rooms: nh heading bins and nc classes whose size templates are the SUN RGB-D ones taken
    round and round, each round 15 % larger: MEAN_SIZES[c % 10] * (1 + 0.15 * (c // 10)).  room_head(12, 10) is the default head."""
    from .head import HeadConfig
    if isinstance(nc, bool) or not isinstance(nc, (int, np.integer)) or nc < 1:
        from ._lib import InvalidArgumentError
        raise InvalidArgumentError("room_head: nc must be an integer >= 1, got %r" % (nc,))
    return HeadConfig(nh, [MEAN_SIZES[c % 10] * (1 + 0.15 * (c // 10)) for c in range(int(nc))])


def _head_sizes(head):
    """(class count, templates, one heading bin only?) of head; the default head's for None."""
    if head is None:
        return 10, MEAN_SIZES, False
    return head.nc, head.mean_sizes_f64, head.nh == 1


def room_scene(n, seed, size=(5.0, 3.0, 5.0), nbox=(6, 10), head=None):
    """head (head.HeadConfig; synth.room_head makes one): the boxes' classes are drawn from range(head.nc), their sizes around the
    head's templates, and with one heading bin every heading is 0 (axis-aligned boxes).  None, or the default head: the output of
    every seed is what it always was."""
    ncls, templates, upright = _head_sizes(head)
    rng = np.random.default_rng(seed)
    sx, sy, sz = size
    n_struct = int(n * 0.6)
    n_obj = n - n_struct
    pts = np.empty((n, 3), np.float64)
    # floor (y = -sy/2 ... camera height), back wall (z = sz), left wall (x = -sx/2)
    which = rng.integers(0, 3, n_struct)
    u, v = rng.random(n_struct), rng.random(n_struct)
    floor = np.stack([(u - 0.5) * sx, np.full(n_struct, -1.2), v * sz], 1)
    back = np.stack([(u - 0.5) * sx, v * sy - 1.2, np.full(n_struct, sz)], 1)
    left = np.stack([np.full(n_struct, -sx / 2), u * sy - 1.2, v * sz], 1)
    pts[:n_struct] = np.where(which[:, None] == 0, floor, np.where(which[:, None] == 1, back, left))
    k = int(rng.integers(nbox[0], nbox[1] + 1))
    per = np.full(k, n_obj // k)
    per[: n_obj - per.sum()] += 1
    o = n_struct
    boxes = []
    for i in range(k):
        cls = int(rng.integers(0, ncls))  # SUN RGB-D class of the box (dataset.py:31-32); same draw as before: clouds unchanged
        l, w, h = templates[cls] * rng.uniform(0.8, 1.2, 3)
        ang = rng.uniform(0, 2 * np.pi)
        if upright:  # (drawn all the same: the generator's state does not depend on nh)
            ang = 0.0
        cx, cz = rng.uniform(-sx / 2 + 0.8, sx / 2 - 0.8), rng.uniform(0.8, sz - 0.8)
        cy = -1.2 + h / 2
        q = rng.uniform(-0.5, 0.5, (per[i], 3)) * np.array([l, h, w])
        face = rng.integers(0, 3, per[i])
        sign = rng.choice([-0.5, 0.5], per[i])
        dims = np.array([l, h, w])
        for a in range(3):
            sel = face == a
            q[sel, a] = sign[sel] * dims[a]
        c, s = np.cos(ang), np.sin(ang)
        x = c * q[:, 0] + s * q[:, 2]
        z = -s * q[:, 0] + c * q[:, 2]
        pts[o:o + per[i]] = np.stack([x + cx, q[:, 1] + cy, z + cz], 1)
        o += per[i]
        boxes.append((cx, cy, cz, l, w, h, ang, cls))
    pts += rng.normal(0, 0.005, pts.shape)
    rng.shuffle(pts)  # the reference subsamples at random: no spatial order in the index
    return pts.astype(np.float32), np.array(boxes, np.float32)


def room_scene_labels(n, seed, size=(5.0, 3.0, 5.0), nbox=(6, 10), head=None):
    """The labels of room_scene(n, seed, size, nbox)'s points -> (instance (n,) int32: the index of the box a point was drawn on, -1
    for the floor and the walls; semantic (n,) int32: that box's SUN RGB-D class, -1 likewise).  room_scene's draws are replayed in
    its order, so the generator is in room_scene's state when the rows are shuffled, and the labels -- shuffled as rows of a 2-D array,
    as the points are -- take the points' permutation.  head: room_scene's."""
    ncls = _head_sizes(head)[0]
    rng = np.random.default_rng(seed)
    n_struct = int(n * 0.6)
    n_obj = n - n_struct
    rng.integers(0, 3, n_struct)
    rng.random(n_struct), rng.random(n_struct)
    k = int(rng.integers(nbox[0], nbox[1] + 1))
    per = np.full(k, n_obj // k)
    per[: n_obj - per.sum()] += 1
    labels = np.full((n, 2), -1, np.int32)
    o = n_struct
    for i in range(k):
        cls = int(rng.integers(0, ncls))
        rng.uniform(0.8, 1.2, 3)                               # l, w, h
        rng.uniform(0, 2 * np.pi)                              # ang
        rng.uniform(0.0, 1.0), rng.uniform(0.0, 1.0)           # cx, cz (one double each, whatever the bounds)
        rng.uniform(-0.5, 0.5, (per[i], 3))
        rng.integers(0, 3, per[i])
        rng.choice([-0.5, 0.5], per[i])
        labels[o:o + per[i]] = (i, cls)
        o += per[i]
    rng.normal(0, 0.005, (n, 3))
    rng.shuffle(labels)
    return labels[:, 0].copy(), labels[:, 1].copy()


def room_batch(b, n, seed0=1000, **kw):  # (kw: room_scene's, head= among them)
    return np.stack([room_scene(n, seed0 + i, **kw)[0] for i in range(b)])


def uniform_batch(b, n, seed0=1000, extent=5.0):
    """Worst case for the ball query: uniform in a cube, no ball fills K -> full n-scan."""
    return np.stack([np.random.default_rng(seed0 + i).random((n, 3), dtype=np.float32) * extent for i in range(b)])


NH, NS, NC = 12, 10, 10  # config.py: heading bins, size classes, semantic classes


def angle2class(angle, num_class=NH):
    """dataset.py:52-67: heading angle -> (bin, residual from the bin centre)."""
    angle = angle % (2 * np.pi)
    per = 2 * np.pi / float(num_class)
    shifted = (angle + per / 2) % (2 * np.pi)
    cid = int(shifted / per)
    res = shifted - (cid * per + per / 2)
    # deviates from dataset.py: within an ulp of 2 pi the quotient rounds to num_class; that bin is class 0 with the residual as computed
    return (0 if cid >= num_class else cid), res


def room_gt(b, n, seed0=1000, head=None, **kw):
    """Ground truth of room_batch(b, n, seed0) in the reference's input layout (model.py:22-32, dataset.py:279-299): the
    generating boxes, ragged lists padded to the longest by repeating the last box (run.py:14-24, np.pad mode='edge').
    -> dict of float32 / int32 arrays: bboxes_xyz (b,BB,3), bboxes_lwh (b,BB,3), bboxes_roty (b,BB), semantic_labels,
    heading_labels (b,BB), heading_residuals (b,BB), size_labels (b,BB), size_residuals (b,BB,3).
    head: room_scene's; its heading bins and templates encode the labels."""
    _, templates, _ = _head_sizes(head)
    nh = head.nh if head is not None else NH
    if head is not None:
        kw["head"] = head
    per_scene = []
    for i in range(b):
        boxes = room_scene(n, seed0 + i, **kw)[1].astype(np.float64)
        rows = []
        for cx, cy, cz, l, w, h, ang, cls in boxes:
            cls = int(cls)
            hc, hr = angle2class(ang, nh)
            size = np.array([l, w, h])
            rows.append((np.array([cx, cy, cz]), size, ang, cls, hc, hr / (np.pi / nh), cls, (size - templates[cls]) / templates[cls]))
        per_scene.append(rows)
    bb = max(len(r) for r in per_scene)
    for r in per_scene:
        r += [r[-1]] * (bb - len(r))
    col = lambda k, dt: np.array([[row[k] for row in r] for r in per_scene], dtype=dt)
    return dict(bboxes_xyz=col(0, np.float32), bboxes_lwh=col(1, np.float32), bboxes_roty=col(2, np.float32),
                semantic_labels=col(3, np.int32), heading_labels=col(4, np.int32), heading_residuals=col(5, np.float32),
                size_labels=col(6, np.int32), size_residuals=col(7, np.float32))
