"""Two restatements of the paper's objectness and centre supervision (include/votenet_proposal_supervision.h).  Test infrastructure.

  (a) the rule in numpy float32, operation for operation (real_boxes, nearest, targets, loss): what the device must reproduce bit for
      bit in its decisions and centre cotangents;
  (b) an independent float64 form in torch on the CPU (loss64): labels and arg-mins from float64 distances taken as constants, the
      cross-entropy from torch.nn.functional, the Chamfer sums from indexed minima, the cotangents from torch.autograd."""
import numpy as np

F = np.float32
NH, NS, NC = 12, 10, 10
W = 5 + 2 * NH + 4 * NS + NC
POS_THR, NEG_THR = 0.3, 0.6  # config.py, as loss.POSITIVE_THRES / NEGATIVE_THRES
W0, W1 = F(0.2), F(0.8)
QUIET = dict(invalid="ignore", over="ignore")


# ------------------------------------------------------------------ (a) float32, operation for operation
def real_boxes(xyz):
    """(bb,3) centres of one scene -> g: trailing rows equal to their predecessor (three ==) are padding."""
    g = len(xyz)
    while g > 1 and xyz[g - 1, 0] == xyz[g - 2, 0] and xyz[g - 1, 1] == xyz[g - 2, 1] and xyz[g - 1, 2] == xyz[g - 2, 2]:
        g -= 1
    return g


def first_min(q):
    """(n,m) -> best (n,), index (n,) along axis 1 by `first || q < best`: the first minimum wins, a NaN in the first candidate sticks."""
    best, idx = q[:, 0].copy(), np.zeros(len(q), np.int32)
    with np.errstate(**QUIET):
        for j in range(1, q.shape[1]):
            upd = q[:, j] < best
            best, idx = np.where(upd, q[:, j], best), np.where(upd, np.int32(j), idx)
    return best, idx


def nearest(pts, centres):
    """nearest_box (csrc/nearest_box.h): (p,3), (bb,3) float32 -> dmin (p,), box (p,)."""
    pts, centres = np.asarray(pts, F), np.asarray(centres, F)
    with np.errstate(**QUIET):
        dx, dy, dz = (pts[:, None, k] - centres[None, :, k] for k in range(3))
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    assert d.dtype == F
    return first_min(d)


def sqdist(c, centres):
    """(p,3) predicted centres, (g,3) -> q (p,g) float32: ((cx-gx)(cx-gx) + (cy-gy)(cy-gy)) + (cz-gz)(cz-gz)."""
    with np.errstate(**QUIET):
        dx, dy, dz = (c[:, None, k] - centres[None, :, k] for k in range(3))
        q = (dx * dx + dy * dy) + dz * dz
    assert q.dtype == F
    return q


def scene(pxyz, pout, gxyz, pos_thr=POS_THR, neg_thr=NEG_THR):
    """One scene -> dict(label (p,), pos, neg, c (p,3), g, e (p,), j1 (p,), f (g,), i2 (g,))."""
    pxyz, pout, gxyz = np.asarray(pxyz, F), np.asarray(pout, F), np.asarray(gxyz, F)
    dmin, _ = nearest(pxyz, gxyz)
    with np.errstate(**QUIET):
        pos, neg = dmin < F(pos_thr), dmin > F(neg_thr)
        c = pxyz + pout[:, 2:5]
    g = real_boxes(gxyz)
    q = sqdist(c, gxyz[:g])
    e, j1 = first_min(q)
    f, i2 = first_min(np.ascontiguousarray(q.T))
    return dict(label=np.where(pos, 1, np.where(neg, 0, -1)).astype(np.int32), pos=pos, neg=neg, c=c, g=g, e=e, j1=j1, f=f, i2=i2, q=q)


def targets(pxyz, pout, gxyz, pos_thr=POS_THR, neg_thr=NEG_THR):
    """-> label (b,p), near_box (b,p), dual_prop (b,bb), real_boxes (b,), all int32, as votenet_proposal_targets writes them."""
    b, p = pxyz.shape[:2]
    bb = gxyz.shape[1]
    label, near = np.empty((b, p), np.int32), np.empty((b, p), np.int32)
    dual, real = np.full((b, bb), -1, np.int32), np.empty(b, np.int32)
    for s in range(b):
        r = scene(pxyz[s], pout[s], gxyz[s], pos_thr, neg_thr)
        label[s], near[s] = r["label"], np.where(r["pos"], r["j1"], -1)
        dual[s, :r["g"]], real[s] = r["i2"], r["g"]
    return label, near, dual, real


def reform(losses, obj, center):
    """The loss vector with losses[2], [3] replaced and losses[9], [0] re-formed in csrc/loss.hip's expressions and order, float32."""
    l = np.array(losses, F)
    l[2], l[3] = F(obj), F(center)
    with np.errstate(**QUIET):
        l[9] = (((l[3] + F(0.1) * l[4]) + l[5]) + F(0.1) * l[6]) + l[7]
        l[0] = ((l[1] + F(0.5) * l[2]) + l[9]) + F(0.1) * l[8]
    return l


def loss(pxyz, pout, gxyz, losses=None, pos_thr=POS_THR, neg_thr=NEG_THR):
    """-> dict(obj, center float32; Np, Nn, G ints; d_obj (b,p,2), d_ctr (b,p,3) float32 cotangents; scenes: the per-scene dicts;
    losses: the re-formed vector where one was given)."""
    pxyz, pout, gxyz = np.asarray(pxyz, F), np.asarray(pout, F), np.asarray(gxyz, F)
    b, p = pxyz.shape[:2]
    sc = [scene(pxyz[s], pout[s], gxyz[s], pos_thr, neg_thr) for s in range(b)]
    Np, Nn, G = int(sum(r["pos"].sum() for r in sc)), int(sum(r["neg"].sum() for r in sc)), int(sum(r["g"] for r in sc))
    inv_m, inv_p, inv_g = F(1.0) / (F(Np + Nn) + F(1e-6)), F(1.0) / (F(Np) + F(1e-6)), F(1.0) / (F(G) + F(1e-6))
    d_obj, d_ctr = np.zeros((b, p, 2), F), np.zeros((b, p, 3), F)
    osum = esum = fsum = 0.0
    with np.errstate(**QUIET):
        for s, r in enumerate(sc):
            pos, neg, c, gc = r["pos"], r["neg"], r["c"], gxyz[s]
            o0, o1 = pout[s, :, 0], pout[s, :, 1]
            mx = np.maximum(o0, o1)
            e0, e1 = np.exp(o0 - mx), np.exp(o1 - mx)
            ssum = e0 + e1
            lse = mx + np.log(ssum)
            w = np.where(pos, W1, W0)
            ce = w * (lse - np.where(pos, o1, o0))
            rcp = F(1.0) / ssum
            lab = pos | neg
            d_obj[s, :, 0] = np.where(lab, ((F(0.5) * w) * (e0 * rcp - np.where(pos, F(0), F(1)))) * inv_m, F(0))
            d_obj[s, :, 1] = np.where(lab, ((F(0.5) * w) * (e1 * rcp - np.where(pos, F(1), F(0)))) * inv_m, F(0))
            assert ce.dtype == F and d_obj.dtype == F
            osum += float(ce[lab].astype(np.float64).sum())
            esum += float(r["e"][pos].astype(np.float64).sum())
            fsum += float(r["f"].astype(np.float64).sum())
            d = np.where(pos[:, None], (F(2.0) * (c - gc[r["j1"]])) * inv_p, F(0.0)).astype(F)
            for j in range(r["g"]):  # the dual terms, in ascending box order
                i = r["i2"][j]
                d[i] = d[i] + (F(2.0) * (c[i] - gc[j])) * inv_g
            assert d.dtype == F
            d_ctr[s] = d
    obj = F(osum * float(inv_m))
    center = F(F(esum * float(inv_p)) + F(fsum * float(inv_g)))
    out = dict(obj=obj, center=center, Np=Np, Nn=Nn, G=G, d_obj=d_obj, d_ctr=d_ctr, scenes=sc)
    if losses is not None:
        out["losses"] = reform(losses, obj, center)
    return out


# ------------------------------------------------------------------ (b) float64, independent
def loss64(pxyz, pout, gxyz, pos_thr=POS_THR, neg_thr=NEG_THR):
    """-> dict(obj, center: python floats; d_out (b,p,5), d_xyz (b,p,3): float64 cotangents of 0.5 obj + center by autograd; Np, Nn, G;
    margin_thr: the smallest |dmin - threshold|; margin_arg: the smallest gap between the two smallest candidates of any arg-min taken
    (inf where there is one candidate))."""
    import torch
    import torch.nn.functional as Fn
    b, p = pxyz.shape[:2]
    xyz = torch.tensor(np.asarray(pxyz, np.float64), requires_grad=True)
    o = torch.tensor(np.asarray(pout, np.float64)[..., :5], requires_grad=True)
    g = torch.tensor(np.asarray(gxyz, np.float64))
    with torch.no_grad():
        dmin = (xyz[:, :, None] - g[:, None]).norm(dim=-1).min(-1).values
        pos, neg = dmin < pos_thr, dmin > neg_thr
        margin_thr = float(torch.minimum((dmin - pos_thr).abs(), (dmin - neg_thr).abs()).min())
    Np, Nn = int(pos.sum()), int(neg.sum())
    ce = Fn.cross_entropy(o[..., :2].reshape(-1, 2), pos.reshape(-1).long(), reduction="none").reshape(b, p)
    w = torch.where(pos, torch.tensor(0.8, dtype=torch.float64), torch.tensor(0.2, dtype=torch.float64))
    obj = (ce * w)[pos | neg].sum() / (Np + Nn + 1e-6)
    c = xyz + o[..., 2:5]
    E = F_ = torch.zeros((), dtype=torch.float64)
    G, margin_arg = 0, float("inf")
    for s in range(b):
        gs = gxyz.shape[1]
        while gs > 1 and np.array_equal(gxyz[s, gs - 1], gxyz[s, gs - 2]):
            gs -= 1
        G += gs
        q = ((c[s][:, None] - g[s, :gs][None]) ** 2).sum(-1)  # (p, gs)
        qd = q.detach()
        j1, i2 = qd.argmin(1), qd.argmin(0)
        E = E + q[torch.arange(p), j1][pos[s]].sum()
        F_ = F_ + q[i2, torch.arange(gs)].sum()
        if gs > 1 and bool(pos[s].any()):
            top = qd[pos[s]].sort(1).values
            margin_arg = min(margin_arg, float((top[:, 1] - top[:, 0]).min()))
        if p > 1:
            top = qd.sort(0).values
            margin_arg = min(margin_arg, float((top[1] - top[0]).min()))
    center = E / (Np + 1e-6) + F_ / (G + 1e-6)
    (0.5 * obj + center).backward()
    return dict(obj=float(obj.detach()), center=float(center.detach()), d_out=o.grad.numpy(), d_xyz=xyz.grad.numpy(), Np=Np, Nn=Nn, G=G,
                margin_thr=margin_thr, margin_arg=margin_arg)


# ------------------------------------------------------------------ cases
def edge_pad(gxyz, extra):
    """(b,bb,3) centres padded by repeating every scene's last box `extra` times (np.pad mode='edge')."""
    return np.concatenate([gxyz, np.repeat(gxyz[:, -1:], extra, axis=1)], axis=1)


def random_case(seed, b, p, real, bb=None, margin=1e-4):
    """Proposals scattered around `real` distinct boxes per scene (edge-padded to bb), offsets that pull them towards a box, random head
    output in the other columns: positives, negatives and grey proposals all occur where p allows.  Drawn again (at most 200 times) until
    every threshold and arg-min margin exceeds `margin` in float64, which is then ASSERTED: the float32 and the float64 form decide
    alike on what this returns.  -> pxyz (b,p,3), pout (b,p,W), gxyz (b,bb,3)."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        gxyz = (rng.random((b, real, 3)) * np.array([4, 1, 4]) + np.array([-2, -1, 1])).astype(F)
        pick = rng.integers(0, real, (b, p))
        spread = rng.choice([0.15, 0.45, 2.0], (b, p, 1))
        pxyz = (gxyz[np.arange(b)[:, None], pick] + rng.normal(0, 1.0, (b, p, 3)) * spread).astype(F)
        pout = rng.normal(0, 1.5, (b, p, W)).astype(F)
        pout[..., 2:5] = (0.7 * (gxyz[np.arange(b)[:, None], pick] - pxyz) + rng.normal(0, 0.2, (b, p, 3))).astype(F)
        if bb is not None and bb > real:
            gxyz = edge_pad(gxyz, bb - real)
        r = loss64(pxyz, pout, gxyz)
        if r["margin_thr"] > margin and r["margin_arg"] > margin:
            break
    assert r["margin_thr"] > margin and r["margin_arg"] > margin, (r["margin_thr"], r["margin_arg"])
    return pxyz, pout, gxyz


def fake_losses(seed=3):
    """12 floats as votenet_loss leaves them: every component its own value, box loss and total composed from them."""
    l = np.random.default_rng(seed).random(12).astype(F) + F(0.25)
    l[10], l[11] = F(17.0), F(23.0)
    return reform(l, l[2], l[3])
