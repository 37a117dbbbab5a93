"""Two restatements of the vote supervision from instance labels (include/votenet_instance_votes.h).  Test infrastructure.

  the rule in numpy float32, operation for operation and un-fused (chain, loss; the sum in the device's order: ordered_sum): what the
  device must reproduce bit for bit in its picks, counts and cotangents;
  an independent float64 form (loss64): the chain walked seed by seed with plain Python comparisons, torch double autograd for the
  gradient."""
import numpy as np

F = np.float32
THREADS, WAVE = 256, 64  # the workgroup of instance_vote_loss_kernel: seed j of a scene belongs to lane j % THREADS
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------------------ float32, operation for operation
def chain(idx1, idx2, point_box, bb):
    """idx1 (b,n1), idx2 (b,n), point_box (b,n0) int32 -> seed_point (b,n) int32 (-1: an index of the chain out of range), row (b,n)
    int32 (the box row of a supervised seed, -1 otherwise), supervised (b,n) bool, counted (b,n) bool: the seeds of Q.  Every index is
    compared with its bound before it is used; one that fails is replaced by 0 and its result discarded."""
    idx1, idx2, point_box = (np.asarray(a, np.int32) for a in (idx1, idx2, point_box))
    n1, n0 = idx1.shape[1], point_box.shape[1]
    i = idx2.astype(np.int64)
    vi = (i >= 0) & (i < n1)
    p = np.take_along_axis(idx1, np.where(vi, i, 0), 1).astype(np.int64)
    vp = vi & (p >= 0) & (p < n0)
    r = np.take_along_axis(point_box, np.where(vp, p, 0), 1).astype(np.int64)
    sup = vp & (r >= 0) & (r < bb)
    counted = ~vp | (r >= bb)
    return np.where(vp, p, -1).astype(np.int32), np.where(sup, r, -1).astype(np.int32), sup, counted


def seed_points(idx1, idx2, n0):
    return chain(idx1, idx2, np.zeros((np.shape(idx1)[0], n0), np.int32), 1)[0]


def ordered_sum(d):
    """(b,n) float32, zeros at the unsupervised seeds -> the float32 sum in the device's order: a lane adds its seeds in ascending
    order, a wave its lanes by the shuffle tree (offsets 32 .. 1), the workgroup its four waves in order, the last workgroup the scenes
    in order."""
    d = np.asarray(d, F)
    b, n = d.shape
    total = F(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for sc in range(b):
            rows = np.zeros(((n + THREADS - 1) // THREADS) * THREADS, F)
            rows[:n] = d[sc]
            lanes = np.zeros(THREADS, F)
            for row in rows.reshape(-1, THREADS):
                lanes = lanes + row
            v = lanes.reshape(THREADS // WAVE, WAVE)
            off = WAVE // 2
            while off:
                nxt = v.copy()
                nxt[:, :WAVE - off] = v[:, :WAVE - off] + v[:, off:]
                v, off = nxt, off // 2
            s = F(0.0)
            for w in range(THREADS // WAVE):
                s = s + v[w, 0]
            total = total + s
            assert total.dtype == F
    return total


def loss(idx1, idx2, point_box, votes, xyz):
    """-> dict(L float32, P, Q int, inv float32, d_votes (b,n,3) float32, dist (b,n) float32 (0 where unsupervised), seed_point, row
    (b,n) int32, supervised (b,n) bool)."""
    votes, xyz = np.asarray(votes, F), np.asarray(xyz, F)
    bb = xyz.shape[1]
    seed_point, row, sup, counted = chain(idx1, idx2, point_box, bb)
    P, Q = int(sup.sum()), int(counted.sum())
    inv = F(1.0) / (F(P) + F(1e-6))
    t = np.take_along_axis(xyz, np.where(sup, row, 0)[..., None].astype(np.int64), 1)  # (b,n,3)
    with np.errstate(invalid="ignore", over="ignore"):
        e = votes - t
        d = (np.abs(e[..., 0]) + np.abs(e[..., 1])) + np.abs(e[..., 2])
        sgn = (e > 0).astype(F) - (e < 0).astype(F)
        g = sgn * inv
        assert e.dtype == F and d.dtype == F and g.dtype == F
        dist = np.where(sup, d, F(0.0))
        d_votes = np.where(sup[..., None], g, F(0.0))
        L = ordered_sum(dist) * inv
    return dict(L=L, P=P, Q=Q, inv=inv, d_votes=d_votes, dist=dist, seed_point=seed_point, row=row, supervised=sup)


def total(losses, L):
    """losses[0] re-formed as votenet_loss composes it (csrc/loss.hip), in float32, from the stored components."""
    l = np.asarray(losses, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F(L) + F(0.5) * l[2] + l[9]) + F(0.1) * l[8]


# ------------------------------------------------------------------ float64, independent
def loss64(idx1, idx2, point_box, votes, xyz):
    """-> L (a torch double scalar with a graph), votes (the leaf), P, Q, seed_point as a list of lists.  The chain seed by seed."""
    import torch
    b, n = np.shape(idx2)
    n1, n0, bb = np.shape(idx1)[1], np.shape(point_box)[1], np.shape(xyz)[1]
    v = torch.tensor(np.asarray(votes, np.float64), requires_grad=True)
    centres = torch.tensor(np.asarray(xyz, np.float64))
    S, J, R_, Q, seed_point = [], [], [], 0, []
    for s in range(b):
        seed_point.append([])
        for j in range(n):
            i = int(idx2[s][j])
            p = int(idx1[s][i]) if 0 <= i < n1 else None
            if p is None or not 0 <= p < n0:
                seed_point[-1].append(-1)
                Q += 1
                continue
            seed_point[-1].append(p)
            r = int(point_box[s][p])
            if r >= bb:
                Q += 1
            elif r >= 0:
                S.append(s), J.append(j), R_.append(r)
    P = len(S)
    L = (v[S, J] - centres[S, R_]).abs().sum() / (P + 1e-6) if P else (v * 0.0).sum()
    return L, v, P, Q, seed_point


# ------------------------------------------------------------------ cases
def levels_case(b, n, seed, repeated=False):
    """idx1 (b, n1 = 2n), idx2 (b, n) int32 for a cloud of n0 = 4n + 5 points: prefixes of random permutations, as farthest-point
    sampling picks (no index twice); repeated: indices drawn with replacement, so several seeds are one cloud point."""
    rng = np.random.default_rng(seed)
    n1, n0 = 2 * n, 4 * n + 5
    if repeated:
        idx1, idx2 = rng.integers(0, max(n0 // 3, 1), (b, n1)), rng.integers(0, max(n1 // 3, 1), (b, n))
    else:
        idx1 = np.stack([rng.permutation(n0)[:n1] for _ in range(b)])
        idx2 = np.stack([rng.permutation(n1)[:n] for _ in range(b)])
    return idx1.astype(np.int32), idx2.astype(np.int32), n0


def labels_case(b, n0, bb, seed, unlabelled=0.4):
    """point_box (b, n0) int32: a row in [0, bb), or -1 for about `unlabelled` of the points; xyz (b, bb, 3) float32 box centres."""
    rng = np.random.default_rng(seed)
    point_box = rng.integers(0, bb, (b, n0)).astype(np.int32)
    point_box[rng.random((b, n0)) < unlabelled] = -1
    xyz = (rng.random((b, bb, 3)) * np.array([4, 1, 4]) + np.array([-2, -1, 1])).astype(F)
    return point_box, xyz


def votes_case(b, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((b, n, 3)) * np.array([5, 2, 5]) + np.array([-2.5, -1.5, 0.5])).astype(F)
