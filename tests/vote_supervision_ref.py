"""Two restatements of the paper's vote supervision (include/votenet_vote_supervision.h).  Test infrastructure.

  the rule in numpy float32, operation for operation (constants, inside, targets, loss): what the device must reproduce bit for bit in
  its decisions and cotangents;
  an independent float64 form (inside64, near_face64, loss64): membership by the half-spaces of the box evaluator.box_corners draws, a
  plain minimum over the centres of ALL containing boxes, torch double autograd for the gradient."""
import numpy as np

F = np.float32


# ------------------------------------------------------------------ float32, operation for operation
def constants(xyz, lwh, roty):
    """(bb,3), (bb,3), (bb,) -> cx, cy, cz, c, s, hl, hh, hw, each (bb,) float32; the trigonometry in double, rounded once."""
    xyz, lwh = np.asarray(xyz, F), np.asarray(lwh, F)
    a = np.asarray(roty, F).astype(np.float64)
    c, s = np.cos(a).astype(F), np.sin(a).astype(F)
    return xyz[:, 0], xyz[:, 1], xyz[:, 2], c, s, F(0.5) * lwh[:, 0], F(0.5) * lwh[:, 2], F(0.5) * lwh[:, 1]


def inside(seeds, xyz, lwh, roty):
    """(n,3) seeds and one scene's boxes -> (n,bb) bool: the closed rule; a NaN fails it."""
    cx, cy, cz, c, s, hl, hh, hw = constants(xyz, lwh, roty)
    p = np.asarray(seeds, F)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy, qz = p[:, None, 0] - cx[None], p[:, None, 1] - cy[None], p[:, None, 2] - cz[None]
        x0 = c[None] * qx - s[None] * qz
        z0 = s[None] * qx + c[None] * qz
        assert x0.dtype == F and z0.dtype == F
        return (np.abs(x0) <= hl[None]) & (np.abs(qy) <= hh[None]) & (np.abs(z0) <= hw[None])


def targets(seeds, gt):
    """(b,n,3) seeds, numpy ground truth -> slots (b,n,3) int32, inside_count (b,n) int32."""
    b, n = seeds.shape[:2]
    slots, count = np.full((b, n, 3), -1, np.int32), np.zeros((b, n), np.int32)
    for sc in range(b):
        ins = inside(seeds[sc], gt["bboxes_xyz"][sc], gt["bboxes_lwh"][sc], gt["bboxes_roty"][sc])
        count[sc] = ins.sum(1)
        for i in np.nonzero(count[sc])[0]:
            j = np.nonzero(ins[i])[0]
            slots[sc, i] = (j[0], j[1] if len(j) >= 2 else j[0], j[-1] if len(j) >= 3 else j[0])
    return slots, count


def loss(seeds, votes, gt):
    """-> dict(L float32, P int, inv float32, d_votes (b,n,3) float32, minima (b,n) float32 (0 where unsupervised), pick (b,n) int32
    (the charged box, -1 where unsupervised), gap: the smallest difference between two distinct slot distances of a seed)."""
    slots, count = targets(seeds, gt)
    votes = np.asarray(votes, F)
    b, n = count.shape
    P = int((count > 0).sum())
    inv = F(1.0) / (F(P) + F(1e-6))
    d_votes, minima, pick = np.zeros((b, n, 3), F), np.zeros((b, n), F), np.full((b, n), -1, np.int32)
    gap = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for sc, i in zip(*np.nonzero(count)):
            v = votes[sc, i]
            best, g = None, -1
            dist = {}  # box -> its distance, the distinct slots only
            for m in range(3):
                t = gt["bboxes_xyz"][sc, slots[sc, i, m]].astype(F)
                d = (np.abs(v[0] - t[0]) + np.abs(v[1] - t[1])) + np.abs(v[2] - t[2])
                assert d.dtype == F
                dist[int(slots[sc, i, m])] = float(d)
                if m == 0 or d < best:  # the first strict minimum
                    best, g = d, slots[sc, i, m]
            minima[sc, i], pick[sc, i] = best, g
            ds = sorted(x for x in dist.values() if x == x)
            gap = min([gap] + [hi - lo for lo, hi in zip(ds, ds[1:])])
            e = v - gt["bboxes_xyz"][sc, g].astype(F)
            sgn = (e > 0).astype(F) - (e < 0).astype(F)
            d_votes[sc, i] = sgn * inv
    L = F(minima[count > 0].astype(np.float64).sum() * float(inv))
    return dict(L=L, P=P, inv=inv, d_votes=d_votes, minima=minima, pick=pick, slots=slots, count=count, gap=gap)


def total(losses, L):
    """losses[0] re-formed as votenet_loss composes it (csrc/loss.hip), in float32, from the stored components."""
    l = np.asarray(losses, F)
    return (F(L) + F(0.5) * l[2] + l[9]) + F(0.1) * l[8]


# ------------------------------------------------------------------ float64, independent
def _axes64(xyz, lwh, roty):
    """corner 0 and the three edges from it (width, length, height) of every box of a scene, from evaluator.box_corners."""
    from votenet_amd import evaluator
    c = evaluator.box_corners(np.asarray(xyz, np.float64), np.asarray(lwh, np.float64), np.asarray(roty, np.float64)).astype(np.float64)
    return c[:, 0], np.stack([c[:, 1] - c[:, 0], c[:, 3] - c[:, 0], c[:, 4] - c[:, 0]], 1)  # (bb,3), (bb,3 edges,3)


def _faces64(seeds, xyz, lwh, roty):
    """signed distances (n,bb,3 axes,2 faces) in metres to the two face planes of every axis: both >= 0 inside."""
    c0, e = _axes64(xyz, lwh, roty)
    q = np.asarray(seeds, np.float64)[:, None, :] - c0[None]
    length = np.linalg.norm(e, axis=-1)                           # (bb,3)
    t = np.einsum("nbk,bak->nba", q, e) / length[None]            # metres along each edge
    return np.stack([t, length[None] - t], -1)


def inside64(seeds, xyz, lwh, roty):
    return (_faces64(seeds, xyz, lwh, roty) >= 0).all((-1, -2))


def near_face64(seeds, xyz, lwh, roty, margin=1e-5):
    """pairs within `margin` metres of a face plane of the box: float32 and float64 may decide them differently."""
    return (np.abs(_faces64(seeds, xyz, lwh, roty)) < margin).any((-1, -2))


def loss64(seeds, votes, gt):
    """-> L (a torch double scalar with a graph), votes (the leaf), P, the containing sets as a (b,n,bb) bool array."""
    import torch
    b, n = seeds.shape[:2]
    ins = np.stack([inside64(seeds[sc], gt["bboxes_xyz"][sc], gt["bboxes_lwh"][sc], gt["bboxes_roty"][sc]) for sc in range(b)])
    v = torch.tensor(np.asarray(votes, np.float64), requires_grad=True)
    centres = torch.tensor(np.asarray(gt["bboxes_xyz"], np.float64))
    d = (v[:, :, None, :] - centres[:, None, :, :]).abs().sum(-1)               # (b,n,bb)
    mask = torch.tensor(ins)
    d = torch.where(mask, d, torch.full_like(d, float("inf")))
    sup = mask.any(-1)
    P = int(sup.sum())
    L = d.min(-1).values[sup].sum() / (P + 1e-6)
    return L, v, P, ins


# ------------------------------------------------------------------ cases
def nested_boxes(k, centre=(0.0, 0.0, 0.0)):
    """k concentric axis-aligned boxes (roty = 0), box j with half extents (j + 1) / 4, and box centres moved apart along x by j / 64
    (so the targets differ): a point at distance r from `centre` along y lies in the boxes j with (j + 1) / 4 >= r."""
    xyz = np.array([[centre[0] + j / 64.0, centre[1], centre[2]] for j in range(k)], F)
    lwh = np.array([[(j + 1) / 2.0 + 1.0] * 3 for j in range(k)], F)
    lwh[:, 2] = [(j + 1) / 2.0 for j in range(k)]  # h: the axis that decides
    return xyz, lwh, np.zeros(k, F)


def edge_pad(gt, extra):
    """Ground truth padded by repeating every scene's last box `extra` times (run.py:14-24, np.pad mode='edge')."""
    return {k: np.concatenate([v, np.repeat(v[:, -1:], extra, axis=1)], axis=1) for k, v in gt.items()}


def device_case(b, n, bb, seed):
    """Seeds, votes and ground truth for the device tests at shape (b, n, bb): per scene a nest of up to five concentric dyadic boxes
    (roty = 0) with seeds exactly ON their faces, rotated random boxes, zero-size boxes, the last box repeated (edge padding), and NaN /
    Inf seeds.  Every box kind is there as far as bb allows."""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((b, bb, 3)) * np.array([4, 1, 4]) + np.array([-2, -1, 1])).astype(F)
    lwh = (rng.random((b, bb, 3)) * 1.5 + 0.4).astype(F)
    roty = (rng.random((b, bb)) * 6.28).astype(F)
    nest = min(5, bb)
    for sc in range(b):
        nx, nl, nr = nested_boxes(nest, centre=(-1.0 + sc, 0.0, 2.0))
        xyz[sc, :nest], lwh[sc, :nest], roty[sc, :nest] = nx, nl, nr
        if bb >= 8:
            lwh[sc, 6] = 0.0                                  # a zero-size box: holds its own centre only
            xyz[sc, -2:], lwh[sc, -2:], roty[sc, -2:] = xyz[sc, -3], lwh[sc, -3], roty[sc, -3]  # edge padding
    pick = rng.integers(0, bb, (b, n))
    seeds = (xyz[np.arange(b)[:, None], pick] + rng.normal(0, 0.5, (b, n, 3))).astype(F)
    for sc in range(b):
        m = 0
        for j in range(nest):                                 # on the +y / -y faces of nest box j, dyadic: exactly representable
            for sign in (1.0, -1.0):
                if m < n:
                    seeds[sc, m] = (xyz[sc, 0, 0], xyz[sc, 0, 1] + sign * (j + 1) / 4.0, xyz[sc, 0, 2])
                    m += 1
        if m < n:
            seeds[sc, m] = xyz[sc, 0]                         # the nest's centre: in all of its boxes
            m += 1
        if bb >= 8 and m < n:
            seeds[sc, m] = xyz[sc, 6]                         # the zero-size box's centre
            m += 1
        for bad in ((np.nan, 0, 2), (0, np.inf, 2), (-np.inf, 0, np.nan), (np.inf, np.inf, np.inf)):
            if n - m > 4:
                seeds[sc, m] = bad
                m += 1
    votes = (seeds + rng.normal(0, 0.3, (b, n, 3))).astype(F)
    votes[~np.isfinite(votes)] = 0.25
    gt = dict(bboxes_xyz=xyz, bboxes_lwh=lwh, bboxes_roty=roty)
    return seeds, votes, gt


def cube_case(seed, b=2, n=200, bb=4):
    """The five-tuple of loss_ref.random_case on axis-aligned unit cubes three apart (roty = 0: the reference's abs-before-rotate and
    its y / w, z / h comparison cannot matter), seeds within 0.9 of a centre per axis and at least 1e-3 off every face: a seed in a cube
    is in that cube only and that cube's centre is the nearest, so the two rules supervise the same seeds with the same targets and
    differ in the divisor alone.  One proposal per scene sits next to a centre, so that every term of the reference's loss is finite."""
    import loss_ref
    rng = np.random.default_rng(seed)
    seeds, votes, prop, out, gt = loss_ref.random_case(seed, b=b, n=n, p=16, bb=bb)
    for sc in range(b):
        for j in range(bb):
            gt["bboxes_xyz"][sc, j] = (3.0 * j - 4.0, 0.25 * sc, 2.0 + 3.0 * sc)
    gt["bboxes_lwh"][:] = 1.0
    gt["bboxes_roty"][:] = 0.0
    prop[:, 0] = gt["bboxes_xyz"][:, 0] + F(0.0625)
    prop[:, 1] = gt["bboxes_xyz"][:, 0] + F(8.0)
    off = rng.uniform(-0.9, 0.9, (b, n, 3))
    off[np.abs(np.abs(off) - 0.5) < 1e-3] = 0.25
    seeds = (gt["bboxes_xyz"][np.arange(b)[:, None], rng.integers(0, bb, (b, n))] + off).astype(F)
    votes = (seeds + rng.normal(0, 0.3, seeds.shape)).astype(F)
    return seeds, votes, prop, out, gt
