"""An independent torch restatement of the reference's loss graph (model.py:61-84, 141-231), used (float64, autograd) to
check the numpy oracle's values and the HIP kernel's cotangents.  Test infrastructure."""
import torch
import torch.nn.functional as Fn


def rotate_pc_along_y(pc, ang):
    """model.py:63-72.  pc (B,N,BB,3), ang (B,BB)."""
    c, s = torch.cos(ang), torch.sin(ang)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    rot = torch.stack([c, z, s, z, o, z, -s, z, c], -1).reshape(ang.shape[0], -1, 3, 3)  # B,BB,3,3
    return torch.einsum("ijkl,imjl->imjk", rot, pc)


def huber(labels, predictions):
    return Fn.huber_loss(predictions, labels, reduction="none", delta=1.0)


def sparse_ce(logits, labels):
    """Mean of tf.nn.sparse_softmax_cross_entropy_with_logits as a GPU computes it: a label outside [0, classes) makes that row's loss
    NaN and, through the product with a NaN constant, the gradient of every logit of the row NaN.  All labels in range: the same
    cross_entropy call as ever."""
    labels = labels.long()
    valid = (labels >= 0) & (labels < logits.shape[1])
    if bool(valid.all()):
        return Fn.cross_entropy(logits, labels, reduction="mean")
    rows = Fn.cross_entropy(logits, labels.clamp(0, logits.shape[1] - 1), reduction="none")
    nan = torch.full_like(rows, float("nan"))
    return (rows * torch.where(valid, torch.ones_like(rows), nan)).mean()


def one_hot(labels, depth, dtype):
    """tf.one_hot: a label outside [0, depth) gives an all-zero row."""
    return (labels.long()[:, None] == torch.arange(depth, device=labels.device)[None, :]).to(dtype)


def votenet_loss(seeds_xyz, votes_xyz, proposals_xyz, out, gt, nh=12, ns=10, nc=10, pos_thr=0.3, neg_thr=0.6):
    """Labels outside their range are defined as TensorFlow defines them for the reference's ops on a GPU: the class term of a proposal
    assigned to such a box is NaN with a NaN cotangent over its class block (sparse_ce); its residual prediction is selected by an
    all-zero one-hot row (model.py:189-193, 200-205), so it is 0 -- Huber of (0 - label residual), no cotangent."""
    bx, lwh, roty = gt["bboxes_xyz"], gt["bboxes_lwh"], gt["bboxes_roty"]
    d2c = (seeds_xyz[:, :, None] - bx[:, None]).abs()
    d2c = rotate_pc_along_y(d2c, -roty)
    inside = ((d2c < lwh[:, None] / 2.0).sum(-1) == 3)
    surface = inside.sum(-1) >= 1
    vassign = d2c.norm(dim=-1).argmin(-1)
    gt_c = torch.gather(bx, 1, vassign[..., None].expand(-1, -1, 3))
    vote = ((votes_xyz - gt_c).abs().sum(-1) * surface.to(votes_xyz.dtype)).mean()
    dist = (proposals_xyz[:, :, None] - bx[:, None]).norm(dim=-1)
    passign = dist.argmin(-1)
    mind = dist.min(-1).values
    pb, pp = torch.nonzero(mind < pos_thr, as_tuple=True)
    nb, npp = torch.nonzero(mind > neg_thr, as_tuple=True)
    pg = passign[pb, pp]
    ce = sparse_ce
    obj = ce(out[pb, pp, :2], torch.ones_like(pb)) + ce(out[nb, npp, :2], torch.zeros_like(nb))
    center = huber(bx[pb, pg] - proposals_xyz[pb, pp], out[pb, pp, 2:5]).sum(-1).mean()
    dual = dist.argmin(1)
    bi = torch.arange(bx.shape[0], device=bx.device)[:, None].expand_as(dual)
    center = center + huber(bx - proposals_xyz[bi, dual], out[bi, dual, 2:5]).sum(-1).mean()
    hl = gt["heading_labels"][pb, pg].long()
    hcls = ce(out[pb, pp, 5:5 + nh], hl)
    hres = huber(gt["heading_residuals"][pb, pg], (out[pb, pp, 5 + nh:5 + 2 * nh] * one_hot(hl, nh, out.dtype)).sum(1)).mean()
    sl = gt["size_labels"][pb, pg].long()
    o = 5 + 2 * nh
    scls = ce(out[pb, pp, o:o + ns], sl)
    sres_pred = (out[pb, pp, o + ns:o + 4 * ns].reshape(-1, ns, 3) * one_hot(sl, ns, out.dtype)[:, :, None]).sum(1)
    sres = huber(gt["size_residuals"][pb, pg], sres_pred).sum(-1).mean()
    sem = ce(out[pb, pp, -nc:], gt["semantic_labels"][pb, pg])
    box = center + 0.1 * hcls + hres + 0.1 * scls + sres
    total = vote + 0.5 * obj + box + 0.1 * sem
    return dict(total_cost=total, vote_reg_loss=vote, obj_cls_loss=obj, center_loss=center, heading_cls_loss=hcls,
                heading_residual_loss=hres, size_cls_loss=scls, size_residual_loss=sres, sem_cls_loss=sem, box_loss=box,
                n_pos=len(pb), n_neg=len(nb), votes_assignment=vassign, surface_ind=surface, bboxes_assignment=passign,
                positive=mind < pos_thr, negative=mind > neg_thr, dual_assignment=dual)


def random_case(seed, b=2, n=256, p=64, bb=5, nh=12, ns=10, nc=10):
    """Seeds / votes / proposals scattered around a few boxes so that positive and negative proposals both occur."""
    import numpy as np
    rng = np.random.default_rng(seed)
    F = np.float32
    bx = (rng.random((b, bb, 3)) * np.array([4, 1, 4]) + np.array([-2, -1, 1])).astype(F)
    gt = dict(bboxes_xyz=bx, bboxes_lwh=(rng.random((b, bb, 3)) * 1.5 + 0.4).astype(F), bboxes_roty=(rng.random((b, bb)) * 6.28).astype(F),
              semantic_labels=rng.integers(0, nc, (b, bb)).astype(np.int32), heading_labels=rng.integers(0, nh, (b, bb)).astype(np.int32),
              heading_residuals=(rng.random((b, bb)) - 0.5).astype(F), size_labels=rng.integers(0, ns, (b, bb)).astype(np.int32),
              size_residuals=((rng.random((b, bb, 3)) - 0.5) * 0.4).astype(F))
    pick = rng.integers(0, bb, (b, n))
    seeds = (bx[np.arange(b)[:, None], pick] + rng.normal(0, 0.6, (b, n, 3))).astype(F)
    votes = (seeds + rng.normal(0, 0.3, (b, n, 3))).astype(F)
    pick = rng.integers(0, bb, (b, p))
    prop = (bx[np.arange(b)[:, None], pick] + rng.normal(0, 0.35, (b, p, 3)) * rng.choice([0.3, 3.0], (b, p, 1))).astype(F)
    out = (rng.normal(0, 1.5, (b, p, 5 + 2 * nh + 4 * ns + nc))).astype(F)
    return seeds, votes, prop, out, gt


def _dec64(seeds, prop, gt):
    """float64 decision margins of a case: (proposal -> nearest centre distance (B,P), seed-to-face distance relative to the half
    extent in the rotated frame (B,N,BB,3))."""
    import numpy as np
    bx = gt["bboxes_xyz"].astype(np.float64)
    mind = np.linalg.norm(prop.astype(np.float64)[:, :, None] - bx[:, None], axis=-1).min(-1)
    d = np.abs(seeds.astype(np.float64)[:, :, None] - bx[:, None])
    a = -gt["bboxes_roty"].astype(np.float64)[:, None]
    c, s = np.cos(a), np.sin(a)
    r = np.stack([c * d[..., 0] + s * d[..., 2], d[..., 1], -s * d[..., 0] + c * d[..., 2]], -1)
    half = gt["bboxes_lwh"].astype(np.float64)[:, None] / 2.0
    return mind, np.abs(r - half) / half


def shape_case(seed, b, n, p, bb, nh, ns, nc, pos_thr=0.3, neg_thr=0.6):
    """random_case at a shape chosen for the kernel's control flow, moved away from every decision that float32 and float64 could take
    differently: at least one positive and one negative proposal in the batch, every proposal's nearest-centre distance >= 1e-3 from both
    thresholds, every seed >= 1e-4 (relative to the half extent, rotated frame) from every box face.  Offenders are drawn again."""
    import numpy as np
    seeds, votes, prop, out, gt = random_case(seed, b=b, n=n, p=p, bb=bb, nh=nh, ns=ns, nc=nc)
    rng = np.random.default_rng(1000003 + seed)
    F = np.float32
    bx = gt["bboxes_xyz"]
    mind, _ = _dec64(seeds, prop, gt)
    if not (mind < pos_thr).any():    # scene 0, proposal 0 next to the scene's first centre
        prop[0, 0] = bx[0, 0] + np.array([0.05, -0.02, 0.03], F)
    if not (mind > neg_thr).any():    # last scene, last proposal far above every centre
        prop[-1, -1] = bx[-1].max(0) + np.array([0.5, 3.0, 0.5], F)
    for _ in range(100):
        mind, face = _dec64(seeds, prop, gt)
        badp = (np.abs(mind - pos_thr) < 1e-3) | (np.abs(mind - neg_thr) < 1e-3)
        bads = (face < 1e-4).any((-1, -2))
        if not badp.any() and not bads.any():
            break
        for s, i in zip(*np.nonzero(badp)):
            prop[s, i] = (bx[s, rng.integers(0, bb)] + rng.normal(0, 0.35, 3) * rng.choice([0.3, 3.0])).astype(F)
        for s, i in zip(*np.nonzero(bads)):
            seeds[s, i] = (bx[s, rng.integers(0, bb)] + rng.normal(0, 0.6, 3)).astype(F)
            votes[s, i] = (seeds[s, i] + rng.normal(0, 0.3, 3)).astype(F)
    else:
        raise AssertionError("shape_case: no draw clear of the decision margins")
    mind, _ = _dec64(seeds, prop, gt)
    assert (mind < pos_thr).any() and (mind > neg_thr).any()
    return seeds, votes, prop, out, gt


# ---- labels at or past their range.  LABEL_BASES[base] -> shape of a shape_case whose LAST proposal of the LAST scene (the last row of
# proposals_output and of its cotangent) is moved next to the box of that scene that already holds the most positives: label_box(base).
# LABEL_CASES[name] = (ground-truth field, bad value, base): the base with that one label of that one box replaced.  nh, ns, nc = 12, 10, 10.
LABEL_BASES = {"p64": dict(seed=301, b=2, n=70, p=64, bb=5), "p256": dict(seed=302, b=2, n=70, p=256, bb=5)}
LABEL_CASES = {
    "heading-nh": ("heading_labels", 12, "p64"),          # what the box encoder used to emit at a bin edge
    "heading-minus1": ("heading_labels", -1, "p64"),
    "size-ns": ("size_labels", 10, "p64"),
    "size-minus1": ("size_labels", -1, "p64"),
    "size-ns-plus-1000": ("size_labels", 1010, "p64"),    # an index far outside the row: past the buffer for the last rows
    "size-ns-plus-1000-p256": ("size_labels", 1010, "p256"),
    "sem-nc": ("semantic_labels", 10, "p64"),
    "sem-minus1": ("semantic_labels", -1, "p64"),
}
# the entries of the loss vector (loss_cases.NAMES) a bad label of each field makes NaN or changes; every other entry keeps its bits
LABEL_AFFECTS = {"heading_labels": ("total_cost", "heading_cls_loss", "heading_residual_loss", "box_loss"),
                 "size_labels": ("total_cost", "size_cls_loss", "size_residual_loss", "box_loss"),
                 "semantic_labels": ("total_cost", "sem_cls_loss")}
LABEL_NAN = {"heading_labels": ("total_cost", "heading_cls_loss", "box_loss"), "size_labels": ("total_cost", "size_cls_loss", "box_loss"),
             "semantic_labels": ("total_cost", "sem_cls_loss")}


def label_blocks(field, valid_label, nh=12, ns=10, nc=10):
    """-> (columns of the class block, columns of the residual slot the VALID label selects) of proposals_output for that field."""
    so = 5 + 2 * nh
    if field == "heading_labels":
        return range(5, 5 + nh), [5 + nh + valid_label]
    if field == "size_labels":
        return range(so, so + ns), [so + ns + 3 * valid_label + k for k in range(3)]
    return range(so + 4 * ns, so + 4 * ns + nc), []


def label_base(base):
    """-> (five-tuple of random_case, (scene, box)).  Decisions keep the margins of shape_case; the moved proposal is positive on its box
    with the second nearest centre at least 1e-3 further away."""
    import numpy as np
    kw = dict(LABEL_BASES[base])
    seeds, votes, prop, out, gt = shape_case(kw.pop("seed"), nh=12, ns=10, nc=10, **kw)
    bx = gt["bboxes_xyz"].astype(np.float64)
    s = prop.shape[0] - 1
    d = np.linalg.norm(prop.astype(np.float64)[s, :, None] - bx[s][None], axis=-1)
    j = int(np.bincount(d.argmin(-1)[d.min(-1) < 0.3], minlength=bx.shape[1]).argmax())
    prop[s, -1] = gt["bboxes_xyz"][s, j] + np.array([0.05, -0.02, 0.03], np.float32)
    mind, _ = _dec64(seeds, prop, gt)
    assert not ((np.abs(mind - 0.3) < 1e-3) | (np.abs(mind - 0.6) < 1e-3)).any()
    dl = np.sort(np.linalg.norm(prop.astype(np.float64)[s, -1] - bx[s], axis=-1))
    assert dl[0] < 0.3 - 1e-3 and dl[1] - dl[0] >= 1e-3
    return (seeds, votes, prop, out, gt), (s, j)


def label_case(name):
    """-> (five-tuple with the bad label, (scene, box), the valid label it replaced)."""
    field, value, base = LABEL_CASES[name]
    (seeds, votes, prop, out, gt), (s, j) = label_base(base)
    gt = {k: v.copy() for k, v in gt.items()}
    valid = int(gt[field][s, j])
    gt[field][s, j] = value
    return (seeds, votes, prop, out, gt), (s, j), valid


# ---- hand-made cases of the loss kernel's decisions.  Every coordinate, extent, residual and hand-written logit is a multiple of 1/64 and
# roty = 0 (cos = 1, sin = 0 exactly), every distance that decides something lies along one axis: each decision is exact in float32 and in
# float64 alike.  HAND_CASES[name]() -> the five-tuple of random_case; HAND_EXPECT[name] -> what the float64 reference must say of it
# (checked in test_loss_cases_cpu.py; the device is then compared with that reference).
def _q(a):
    import numpy as np
    return (np.round(np.asarray(a, np.float64) * 64.0) / 64.0).astype(np.float32)


def _hand_blank(seed, b, n, p, bb, nh=12, ns=10, nc=10):
    """Boxes of extent 1 three apart on a line, labels and residuals all different; every proposal far away (negative), every seed
    outside every box, logits random multiples of 1/64."""
    import numpy as np
    rng = np.random.default_rng(seed)
    F = np.float32
    gt = dict(bboxes_xyz=np.zeros((b, bb, 3), F), bboxes_lwh=np.ones((b, bb, 3), F), bboxes_roty=np.zeros((b, bb), F),
              semantic_labels=np.zeros((b, bb), np.int32), heading_labels=np.zeros((b, bb), np.int32),
              heading_residuals=np.zeros((b, bb), F), size_labels=np.zeros((b, bb), np.int32), size_residuals=np.zeros((b, bb, 3), F))
    for s in range(b):
        for j in range(bb):
            gt["bboxes_xyz"][s, j] = (3.0 * j, 0.0, 2.0 + 5.0 * s)
            gt["semantic_labels"][s, j] = (1 + 3 * j + s) % nc
            gt["heading_labels"][s, j] = (3 + 4 * j + s) % nh
            gt["size_labels"][s, j] = (2 + 3 * j + s) % ns
            gt["heading_residuals"][s, j] = (j - 1 + s) / 8.0
            gt["size_residuals"][s, j] = ((j + 1) / 16.0, -(j + 2) / 32.0, (s + 1) / 64.0)
    prop = np.zeros((b, p, 3), F)
    prop[:, :, 0] = 100.0 + np.arange(p)[None, :] / 4.0
    prop[:, :, 1] = 50.0
    seeds = np.zeros((b, n, 3), F)
    seeds[:, :, 0] = -60.0 - np.arange(n)[None, :] / 2.0
    seeds[:, :, 1] = 40.0
    votes = _q(seeds + rng.normal(0, 0.3, seeds.shape))
    out = _q(rng.normal(0, 1.5, (b, p, 5 + 2 * nh + 4 * ns + nc)))
    return seeds, votes, prop, out, gt


def case_box_ties():
    """First-minimum ties of the box arg-min.  Scene 0: boxes 0 and 1 share a centre (labels, residuals, sizes differ), box 2 is half a
    unit along x: a proposal on the shared centre's side takes box 0, a proposal and a seed midway between the pair and box 2 take box 0
    of three.  Scene 1: boxes 1 and 2 share a centre and box 0 is four units off: the tie is won by box 1, not by index 0; a seed midway
    between box 0 and the pair takes box 0."""
    import numpy as np
    seeds, votes, prop, out, gt = _hand_blank(21, 2, 5, 4, 3)
    bx, lwh = gt["bboxes_xyz"], gt["bboxes_lwh"]
    bx[0] = [(0, 0, 2), (0, 0, 2), (0.5, 0, 2)]
    lwh[0] = [(1, 1, 1), (2, 2, 2), (1, 1, 1)]
    bx[1] = [(4, 0, 7), (0, 0, 7), (0, 0, 7)]
    lwh[1] = [(5, 1, 1), (0.5, 0.5, 0.5), (1, 1, 1)]
    prop[0, 0] = (0, 1 / 64, 2)        # 1/64 from boxes 0 and 1: box 0
    prop[0, 1] = (0.25, 0, 2)          # 0.25 from all three: box 0
    prop[0, 3] = (0, 0.375, 2)         # dead zone
    prop[1, 0] = (0, 0, 7.125)         # 0.125 from boxes 1 and 2: box 1
    prop[1, 3] = (4, 0.125, 7)         # box 0
    seeds[0, 0] = (0.25, 0, 2)         # three-way tie, inside all: target = centre of box 0, not of box 2
    seeds[0, 1] = (0.125, 0, 2)        # tie of the pair
    seeds[0, 3] = (0.75, 0, 2)         # box 2 alone
    seeds[1, 0] = (2, 0, 7)            # 2 from box 0 and from the pair, inside box 0 (half extent 2.5) only: box 0
    seeds[1, 1] = (0, 0.25, 7)         # tie of the pair, on the small box's face, inside the large one: box 1
    votes[:, :4] = _q(seeds[:, :4] + np.array([0.25, -0.125, 0.5], np.float32))
    return seeds, votes, prop, out, gt


def case_dual_ties():
    """First-minimum ties of the dual term's wave arg-min, P = 130 (lanes hold p, p + 64, p + 128).  Each tied group is a set of proposals
    at one point, nearest to one box; the lowest index is pulled.  The others carry a centre prediction equal to their own target: their
    centre cotangents are exactly zero unless the box pulls them too."""
    seeds, votes, prop, out, gt = _hand_blank(22, 2, 4, 130, 3)
    bx = gt["bboxes_xyz"]
    groups = {(0, 0): (5, 6),          # neighbouring lanes
              (0, 1): (3, 67),         # one lane, two rounds
              (0, 2): (128, 129),      # third round of lanes 0 and 1
              (1, 0): (70, 71),
              (1, 1): (1, 65, 129),    # one lane, three rounds
              (1, 2): (66, 10)}        # the lower index sits in the higher lane
    for (s, j), idx in groups.items():
        for i in idx:
            prop[s, i] = bx[s, j] + _q((0.125, 0, 0) if j != 1 else (0, -0.125, 0))
            if i != min(idx):
                out[s, i, 2:5] = bx[s, j] - prop[s, i]
    return seeds, votes, prop, out, gt


def _case_many_boxes(seed, p, bb, which):
    import numpy as np
    seeds, votes, prop, out, gt = _hand_blank(seed, 2, 3, p, bb)
    for s in range(2):
        for j in range(bb):
            gt["bboxes_xyz"][s, j] = ((j % 8) / 4.0, 0.0, 2.0 + 5.0 * s + (j // 8) / 4.0)
    prop[0, which] = (1 - 1 / 64, 1 / 64, 2.5 + 1 / 64) if bb > 8 else (0.25 + 1 / 64, 1 / 64, 2.0)
    if p > 1:
        prop[1, which] = (1.0, 2.0, 7.5)  # scene 1: the nearest of three again, but two units above the boxes (negative): every pull is linear
    seeds[0, 0] = (0.25, 0.125, 2.125)
    return seeds, votes, prop, out, gt


def case_one_proposal_five_boxes():
    """P = 1: every box of a scene pulls the only proposal (positive in scene 0, negative in scene 1); the pulls add up in box order."""
    return _case_many_boxes(23, 1, 5, 0)


def case_three_proposals_forty_boxes():
    """P = 3, BB = 40: proposal 1 is the nearest of every box; proposals 0 and 2 get no pull at all."""
    return _case_many_boxes(24, 3, 40, 1)


def case_seed_on_face():
    """|seed - centre| equal to the half extent on one axis (or on all three) is outside (strict <): no vote loss, d_votes row exactly 0."""
    seeds, votes, prop, out, gt = _hand_blank(25, 2, 8, 2, 2)
    gt["bboxes_lwh"][:, 0] = (1.0, 0.5, 2.0)
    for s in range(2):
        c = gt["bboxes_xyz"][s, 0]
        off = [(0.5, 0, 0), (0, 0.25, 0), (0, 0, 1.0), (-0.5, 0, 0), (0.5, 0.25, 1.0), (0, -0.25, -1.0),
               (0.5 - 1 / 64, 0.25 - 1 / 64, 1.0 - 1 / 64), (-0.5 + 1 / 64, 0, 0)]  # the last two are inside
        for i, o in enumerate(off):
            seeds[s, i] = c + _q(o)
        prop[s, 0] = c + _q((0, 1 / 64, 0))
    return seeds, votes, prop, out, gt


def case_vote_on_target():
    """A vote exactly on its target centre (all three components, or one of them): that cotangent is exactly 0."""
    seeds, votes, prop, out, gt = _hand_blank(26, 2, 6, 2, 2)
    for s in range(2):
        c = gt["bboxes_xyz"][s, 1]
        for i in range(4):
            seeds[s, i] = c + _q((0.125 * (i - 1), 0.0625, -0.25))
        votes[s, 0] = c
        votes[s, 1] = c + _q((0.5, 0, -0.25))
        votes[s, 2] = c + _q((0, -1 / 64, 0))
        votes[s, 3] = c + _q((1 / 64, 0.25, 0))
        prop[s, 0] = c + _q((0, 0, 1 / 64))
    return seeds, votes, prop, out, gt


def case_huber_knee():
    """Centre, heading-residual and size-residual errors of exactly +-1 and +-(1 + 1/64) (and 0, +-63/64 beside them): the quadratic /
    linear switch of the Huber loss and of its gradient, in the proposals' own terms and in the dual term."""
    seeds, votes, prop, out, gt = _hand_blank(27, 2, 3, 10, 2)
    E = [1.0, -1.0, 1 + 1 / 64, -1 - 1 / 64, 63 / 64, -63 / 64, 0.0, 1.0]
    for s in range(2):
        for i in range(8):
            j = i % 2
            gi = (s, j)
            prop[s, i] = gt["bboxes_xyz"][gi] + _q(((i + 1) / 64, 0, -(i // 2) / 64))
            cg = gt["bboxes_xyz"][gi] - prop[s, i]
            e = [E[i], E[(i + 3) % 8], E[(i + 5) % 8]]
            out[s, i, 2:5] = cg + _q(e)
            hl, sl = int(gt["heading_labels"][gi]), int(gt["size_labels"][gi])
            out[s, i, 5 + 12 + hl] = gt["heading_residuals"][gi] + _q(E[(i + 1) % 8])
            so = 5 + 24 + 10 + 3 * sl
            out[s, i, so:so + 3] = gt["size_residuals"][gi] + _q([E[(i + 2) % 8], E[(i + 4) % 8], E[(i + 6) % 8]])
    return seeds, votes, prop, out, gt


THRESHOLDS = (0.25, 0.5)  # of case_thresholds: exact in float32, passed through the C ABI


def case_thresholds():
    """pos_thr = 0.25, neg_thr = 0.5.  Proposals at distance 0.25 and 0.5 exactly (neither positive nor negative: strict < and >), 0.375
    (dead zone) and 1/64 inside / outside each threshold, along each axis in turn."""
    seeds, votes, prop, out, gt = _hand_blank(28, 2, 3, 9, 2)
    D = [0.25, 0.5, 0.375, 0.25 - 1 / 64, 0.25 + 1 / 64, 0.5 - 1 / 64, 0.5 + 1 / 64, 0.0]
    for s in range(2):
        for i, d in enumerate(D):
            o = [0.0, 0.0, 0.0]
            o[(i + s) % 3] = d if (i + s) % 2 == 0 else -d
            prop[s, i] = gt["bboxes_xyz"][s, (i + s) % 2] + _q(o)
    return seeds, votes, prop, out, gt


HAND_CASES = dict(box_ties=case_box_ties, dual_ties=case_dual_ties, one_proposal_five_boxes=case_one_proposal_five_boxes,
                  three_proposals_forty_boxes=case_three_proposals_forty_boxes, seed_on_face=case_seed_on_face,
                  vote_on_target=case_vote_on_target, huber_knee=case_huber_knee, thresholds=case_thresholds)

# What the reference must decide for each hand case: counts, and (scene, index) -> value for the entries a case is about.
# zero_rows: (cotangent, scene, index) rows that must be exactly zero ("centre" = columns 2:5 of proposals_output's cotangent).
_T, _F = True, False
HAND_EXPECT = dict(
    box_ties=dict(n_pos=4, n_neg=3, bboxes_assignment={(0, 0): 0, (0, 1): 0, (1, 0): 1, (1, 3): 0},
                  votes_assignment={(0, 0): 0, (0, 1): 0, (0, 3): 2, (1, 0): 0, (1, 1): 1},
                  surface_ind={(0, 0): _T, (0, 1): _T, (0, 2): _F, (0, 3): _T, (0, 4): _F, (1, 0): _T, (1, 1): _T},
                  dual_assignment={(0, 0): 0, (0, 1): 0, (0, 2): 1, (1, 0): 3, (1, 1): 0, (1, 2): 0}),
    dual_ties=dict(n_pos=13, n_neg=247, dual_assignment={(0, 0): 5, (0, 1): 3, (0, 2): 128, (1, 0): 70, (1, 1): 1, (1, 2): 10},
                   zero_rows=[(c, s, i) for c in ("proposals_xyz", "centre")
                              for s, i in ((0, 6), (0, 67), (0, 129), (1, 71), (1, 65), (1, 129), (1, 66))]),
    one_proposal_five_boxes=dict(n_pos=1, n_neg=1, bboxes_assignment={(0, 0): 1}, votes_assignment={(0, 0): 1},
                                 dual_assignment={(s, j): 0 for s in range(2) for j in range(5)}),
    three_proposals_forty_boxes=dict(n_pos=1, n_neg=5, bboxes_assignment={(0, 1): 20}, votes_assignment={(0, 0): 1},
                                     dual_assignment={(s, j): 1 for s in range(2) for j in range(40)},
                                     zero_rows=[(c, s, i) for c in ("proposals_xyz", "centre") for s in range(2) for i in (0, 2)]),
    seed_on_face=dict(n_pos=2, n_neg=2, surface_ind={(s, i): i >= 6 for s in range(2) for i in range(8)},
                      zero_rows=[("votes_xyz", s, i) for s in range(2) for i in range(6)]),
    vote_on_target=dict(n_pos=2, n_neg=2, surface_ind={(s, i): i < 4 for s in range(2) for i in range(6)},
                        votes_assignment={(s, i): 1 for s in range(2) for i in range(4)},
                        zero_rows=[("votes_xyz", s, i) for s in range(2) for i in (0, 4, 5)]),
    huber_knee=dict(n_pos=16, n_neg=4, bboxes_assignment={(s, i): i % 2 for s in range(2) for i in range(8)},
                    dual_assignment={(s, j): j for s in range(2) for j in range(2)}),
    thresholds=dict(n_pos=4, n_neg=4, thr=THRESHOLDS,
                    positive={(s, i): i in (3, 7) for s in range(2) for i in range(9)},
                    negative={(s, i): i in (6, 8) for s in range(2) for i in range(9)}),
)
