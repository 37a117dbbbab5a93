"""The rule of include/votenet_vote_sampling.h restated in numpy float32, operation for operation, independent of the oracle and of the
device code: sampling under the tie key (distance descending, k mod 512 ascending, k ascending) with the non-finite rule, the raw
centres, the ball query against a threshold T that is passed in, the pad and zero-row rules.  Every intermediate is a float32 array, so
every product and sum rounds to float32 before the next (no fused multiply-add)."""
import numpy as np

F = np.float32
BIG = F(1e38)


def ball_threshold(r):
    """The smallest float32 T whose correctly rounded square root is >= r (numpy's float32 sqrt is correctly rounded)."""
    r = F(r)
    t = F(r * r)
    while t > 0 and np.sqrt(t) >= r:
        t = np.nextafter(t, F(0))
    while np.sqrt(t) < r:
        t = np.nextafter(t, F(np.inf))
    return F(t)


def threshold(radius):
    """T as the entry forms it: nothing is closer than a radius <= 1e-20."""
    return F(-1.0) if F(radius) <= F(1e-20) else ball_threshold(radius)


def as_sampled(scene):
    """The cloud as sampling reads it: point 0's non-finite components are 0; a point with a non-finite component is a copy of it."""
    p = np.array(scene, F, copy=True)
    p[0, ~np.isfinite(p[0])] = 0
    p[~np.isfinite(p).all(axis=1)] = p[0]
    return p


def sample(scene, m):
    """-> fps_idx (m,) int32 and what the ties did: rounds whose maximum several points held, and among them the rounds the key
    decided AGAINST index order (the winner is not the smallest index of those that hold the maximum)."""
    p = as_sampled(scene)
    n = len(p)
    k = np.arange(n)
    key = (k % 512) * 4096 + k
    t = np.full(n, BIG, F)
    out = np.zeros(m, np.int32)
    ties = against = 0
    last = 0
    with np.errstate(all="ignore"):
        for j in range(1, m):
            d = p - p[last]
            d = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            t = np.where(d < t, d, t)
            held = np.nonzero(t == t.max())[0]
            last = int(held[np.argmin(key[held])])
            if len(held) > 1 and t.max() > 0:
                ties += 1
                against += last != held[0]
            out[j] = last
    return out, dict(ties=ties, against=against)


def ball_query(scene, centres, T, nsample):
    """raw coordinates -> idx (m, nsample) int32, pts_cnt (m,) int32, hits (m,): the number of candidates inside, uncapped."""
    p, q = np.asarray(scene, F), np.asarray(centres, F)
    with np.errstate(all="ignore"):
        d = q[:, None, :] - p[None, :, :]
        s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        inside = s < F(T)  # a NaN is no hit
    m = len(q)
    idx = np.zeros((m, nsample), np.int32)
    cnt = np.zeros(m, np.int32)
    for j in range(m):
        hit = np.nonzero(inside[j])[0][:nsample]
        c = len(hit)
        if c:
            idx[j, :c] = hit
            idx[j, c:] = hit[0]
        cnt[j] = c
    return idx, cnt, inside.sum(axis=1)


def cluster_votes(votes, m, T, nsample):
    """votes (b,n,3) -> dict fps_idx (b,m), new_xyz (b,m,3) -- the raw votes, bit for bit --, idx (b,m,nsample), pts_cnt (b,m), and
    for the tests' property checks hits (b,m) and the scenes' tie counts."""
    votes = np.ascontiguousarray(votes, F)
    res = dict(fps_idx=[], new_xyz=[], idx=[], pts_cnt=[], hits=[], ties=0, against=0)
    for scene in votes:
        f, info = sample(scene, m)
        centres = scene[f]
        i, c, h = ball_query(scene, centres, T, nsample)
        for name, v in (("fps_idx", f), ("new_xyz", centres), ("idx", i), ("pts_cnt", c), ("hits", h)):
            res[name].append(v)
        res["ties"] += info["ties"]
        res["against"] += info["against"]
    return {k: (np.stack(v) if isinstance(v, list) else v) for k, v in res.items()}
