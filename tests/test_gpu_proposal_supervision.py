"""GPU: the paper's objectness and centre supervision on the device -- votenet_proposal_targets and votenet_paper_proposal_loss
(csrc/propsup/proposal_supervision.hip) against the float32 restatement tests/proposal_supervision_ref.py (form a), bit for bit in every
decision and centre cotangent, and against the independent float64 form (b) in the objectness columns and the loss values; what the
launch leaves alone; and VoteNetHotPath.enable_proposal_supervision: a step with the mode on changes the two terms, their cotangents,
the box loss and the total and nothing else, on the plain path and through the replayed graphs; a step with the mode off never loads the
library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402
import proposal_supervision_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W = R.W
# (b, p, real boxes, bb, pitch): p = 40 is no multiple of the wave, 64 one wave, 256 the training size (four waves); one box, five
# edge-padded to eight, LOSS_MAXBOX; dense rows and rows 128 floats apart
SHAPES = [(1, 40, 1, 1, W), (3, 40, 5, 8, 128), (1, 64, 5, 8, W), (3, 64, 256, 256, 128), (3, 256, 5, 8, W), (1, 256, 256, 256, 128),
          (3, 256, 1, 1, 128)]
SHAPE_IDS = ["b%d-p%d-g%d-bb%d-pitch%d" % s for s in SHAPES]
B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_monitors.py)
GUARD = 64
KEEP = [1, 4, 5, 6, 7, 8, 10, 11]  # the loss values the launch does not write
PATTERN = -7.0


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    t = t.detach().contiguous().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def close(got, want, floor=1.0):
    """the bar of tests/test_gpu_loss.py: 1e-5 relative, floor 1.0 for loss values, 1e-3 for cotangents"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.abs(got - want).max() <= 1e-5 * max(floor, np.abs(want).max()))


def pitched(pout, pitch, dev):
    """(b,p,W) numpy -> a device view of that shape whose rows are `pitch` floats apart (the rest of a row holds other numbers)."""
    b, p, w = pout.shape
    wide = torch.full((b, p, pitch), 3.25, device=dev)
    wide[..., :w] = T(pout, dev)
    return wide[..., :w] if pitch > w else wide


def guarded(shape, dev, dtype=torch.float32):
    """A pattern-filled contiguous tensor of `shape` with GUARD pattern elements before and behind it -> (tensor, whole buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), PATTERN, device=dev).to(dtype)
    return whole[GUARD:GUARD + n].view(shape), whole


def guards_intact(whole):
    return bool((whole[:GUARD] == PATTERN).all() and (whole[-GUARD:] == PATTERN).all())


_cases = {}


def case(shape):
    """The inputs of a shape and both references' results, computed once and shared."""
    if shape not in _cases:
        b, p, real, bb, _ = shape
        pxyz, pout, gxyz = R.random_case(31 + p + bb, b, p, real, bb)
        l0 = R.fake_losses(3 + p)
        _cases[shape] = (pxyz, pout, gxyz, l0, R.loss(pxyz, pout, gxyz, losses=l0), R.loss64(pxyz, pout, gxyz))
    return _cases[shape]


def totals64(l0, obj, center):
    """losses[9], losses[0] in float64 from the float64 terms and the untouched components."""
    l = np.asarray(l0, np.float64)
    box = center + 0.1 * l[4] + l[5] + 0.1 * l[6] + l[7]
    return box, l[1] + 0.5 * obj + box + 0.1 * l[8]


def run_loss(dev, pxyz, pout, gxyz, l0, pitch=W, work=None):
    """One guarded launch -> dict of numpy results and the guard verdict."""
    from votenet_amd import proposal_supervision as PS
    b, p = pxyz.shape[:2]
    out = dict(proposals_xyz=T(pxyz, dev), proposals_output=pitched(pout, pitch, dev))
    d_xyz, wx = guarded((b, p, 3), dev)
    d_out, wo = guarded((b, p, W), dev)
    losses, wl = guarded((12,), dev)
    losses.copy_(T(l0, dev))
    counts, wc = guarded((3,), dev, torch.int32)
    rx, ro, rc = PS.paper_proposal_loss(out, dict(bboxes_xyz=T(gxyz, dev)), losses, d_xyz=d_xyz, d_out=d_out, counts=counts, work=work)
    assert rx is d_xyz and ro is d_out and rc is counts
    torch.cuda.synchronize()
    return dict(d_xyz=d_xyz.cpu().numpy(), d_out=d_out.cpu().numpy(), losses=losses.cpu().numpy(), counts=counts.cpu().numpy().tolist(),
                guards=all(guards_intact(w) for w in (wx, wo, wl, wc)))


# ------------------------------------------------------------------ targets
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_targets_equal_the_restatement(hiplib, dev, shape):
    from votenet_amd import proposal_supervision as PS
    b, p, real, bb, pitch = shape
    pxyz, pout, gxyz, _, _, _ = case(shape)
    out = dict(proposals_xyz=T(pxyz, dev), proposals_output=pitched(pout, pitch, dev))
    got = PS.proposal_targets(out, dict(bboxes_xyz=T(gxyz, dev)))
    want = R.targets(pxyz, pout, gxyz)
    for g, w, name, shp in zip(got, want, ("label", "near_box", "dual_prop", "real_boxes"), ((b, p), (b, p), (b, bb), (b,))):
        assert g.dtype == torch.int32 and tuple(g.shape) == shp, name
        assert np.array_equal(g.cpu().numpy(), w), name
    label, near, dual, rb = (g.cpu().numpy() for g in got)
    print(shape, "labels 1/0/-1:", [(label == k).sum() for k in (1, 0, -1)], "real", rb.tolist())
    assert (rb == real).all() and (dual[:, real:] == -1).all() and (dual[:, :real] >= 0).all() and dual.max() < p
    assert (label == 1).any() and ((near >= 0) == (label == 1)).all() and near.max() < real


# ------------------------------------------------------------------ the loss
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_loss_and_cotangents_equal_the_references(hiplib, dev, shape):
    from votenet_amd import proposal_supervision as PS
    b, p, real, bb, pitch = shape
    pxyz, pout, gxyz, l0, a, ref = case(shape)
    work = PS.workspace(b, dev)
    runs = [run_loss(dev, pxyz, pout, gxyz, l0, pitch, work) for _ in range(2)]  # twice over one workspace: the launch leaves it zero
    assert not work.any() and runs[0]["guards"] and runs[1]["guards"]
    for k in ("d_xyz", "d_out", "losses"):
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), k  # the same bytes
    r = runs[0]
    l, d_out = r["losses"], r["d_out"]
    box64, total64 = totals64(l0, ref["obj"], ref["center"])
    print(shape, "Np Nn G", r["counts"], (a["Np"], a["Nn"], a["G"]), "obj", l[2], ref["obj"], "center", l[3], ref["center"],
          "box", l[9], box64, "total", l[0], total64)
    assert r["counts"] == [a["Np"], a["Nn"], a["G"]] == [ref["Np"], ref["Nn"], ref["G"]]
    # the centre columns and d_proposals_xyz: the restatement's bits, and each other's
    assert np.array_equal(d_out[..., 2:5].view(np.int32), a["d_ctr"].view(np.int32))
    assert np.array_equal(r["d_xyz"].view(np.int32), d_out[..., 2:5].view(np.int32))
    # the objectness columns and the four loss values: the float64 form, at the bar of tests/test_gpu_loss.py
    assert close(d_out[..., :2], ref["d_out"][..., :2], 1e-3) and close(d_out[..., 2:5], ref["d_out"][..., 2:5], 1e-3)
    assert close(l[2], ref["obj"]) and close(l[3], ref["center"]) and close(l[9], box64) and close(l[0], total64)
    assert np.array_equal(l.view(np.int32), R.reform(l0, l[2], l[3]).view(np.int32))  # re-formed in loss.hip's expressions and order
    grey = np.stack([~(s["pos"] | s["neg"]) for s in a["scenes"]])
    assert not d_out[..., :2][grey].view(np.int32).any()  # +0.0f in both columns
    # what is left alone
    assert (d_out[..., 5:] == PATTERN).all() and np.array_equal(l[KEEP].view(np.int32), l0[KEEP].view(np.int32))
    fx, fo, fc = PS.paper_proposal_loss(dict(proposals_xyz=T(pxyz, dev), proposals_output=T(pout, dev)), dict(bboxes_xyz=T(gxyz, dev)),
                                        T(l0, dev))  # for a caller of the operator layer: fresh buffers, dense rows
    assert torch.equal(bits(fx), bits(r["d_xyz"])) and torch.equal(bits(fo[..., :5]), bits(d_out[..., :5])) and not fo[..., 5:].any()


def test_counts_are_votenet_loss_s_and_the_rest_of_its_results_keep_their_bits(hiplib, dev):
    """Behind a real votenet_loss, into its own buffers: Np, Nn are losses[10], losses[11]; columns 5..W of d_proposals_output,
    d_votes_xyz and the eight other loss values keep their bits."""
    from votenet_amd import loss as VL
    from votenet_amd import proposal_supervision as PS
    seeds, votes, prop, pout, gt = loss_ref.shape_case(21, b=3, n=70, p=64, bb=5, nh=12, ns=10, nc=10)
    out = dict(seeds_xyz=T(seeds, dev), votes_xyz=T(votes, dev), proposals_xyz=T(prop, dev), proposals_output=T(pout, dev))
    g = VL.gt_to_device(gt, dev)
    losses, cot = VL.votenet_loss(out, g)
    l_ref, before = losses.cpu().numpy().copy(), {k: v.clone() for k, v in cot.items()}
    _, _, counts = PS.paper_proposal_loss(out, g, losses, d_xyz=cot["proposals_xyz"], d_out=cot["proposals_output"])
    l, c = losses.cpu().numpy(), counts.cpu().numpy().tolist()
    a = R.loss(prop, pout, gt["bboxes_xyz"], losses=l_ref)
    print("Np Nn G", c, "votenet_loss n_pos n_neg", l_ref[10], l_ref[11], "obj", l_ref[2], "->", l[2], "center", l_ref[3], "->", l[3])
    assert c[0] == l_ref[10] > 0 and c[1] == l_ref[11] > 0 and c == [a["Np"], a["Nn"], a["G"]] and c[2] == 15
    assert np.array_equal(l[KEEP].view(np.int32), l_ref[KEEP].view(np.int32)) and np.isfinite(l).all()
    assert l[2] != l_ref[2] and l[3] != l_ref[3] and np.array_equal(l.view(np.int32), R.reform(l_ref, l[2], l[3]).view(np.int32))
    assert torch.equal(bits(cot["votes_xyz"]), bits(before["votes_xyz"]))
    assert torch.equal(bits(cot["proposals_output"][..., 5:]), bits(before["proposals_output"][..., 5:]))
    assert torch.equal(bits(cot["proposals_output"][..., 2:5]), bits(a["d_ctr"])) and torch.equal(bits(cot["proposals_xyz"]), bits(a["d_ctr"]))
    assert not torch.equal(bits(cot["proposals_xyz"]), bits(before["proposals_xyz"]))


# ------------------------------------------------------------------ edge cases
def same(got, want):
    """equal where the restatement is NaN or infinite, at the loss bar elsewhere"""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    fin = np.isfinite(want)
    return bool(np.array_equal(got[~fin], want[~fin], equal_nan=True) and (not fin.any() or close(got[fin], want[fin])))


def test_ties_the_first_index_wins_and_dual_terms_add_in_box_order(hiplib, dev):
    from votenet_amd import proposal_supervision as PS
    # scene 0: proposals 0 and 1 are duplicates and win all four boxes (i2 = 0 everywhere); boxes 0, 1 and 2, 3 are near pairs.
    # scene 1: boxes 0 and 1 are DUPLICATE real boxes (an interior repetition is not padding), boxes 2, 3 edge padding of box 2's copy.
    p = 70
    rng = np.random.default_rng(4)
    gxyz = np.array([[[0, 0, 0], [1e-3, 0, 0], [3, 0, 0], [3, 1e-4, 0]], [[1, 0, 2], [1, 0, 2], [-1, 0.5, 2], [-1, 0.5, 2]]], F)
    pxyz = (np.array([9, 9, 9], F) + rng.random((2, p, 3))).astype(F)
    pout = rng.normal(0, 1, (2, p, W)).astype(F)
    pout[..., 2:5] = 0
    pxyz[0, 0] = pxyz[0, 1] = (0.1, 0.01, 0.02)
    pxyz[1, 65] = pxyz[1, 3] = (1.05, 0.0, 2.0)       # duplicates in different waves: the lower index wins box 0 and box 1
    pxyz[1, 69] = pxyz[1, 64] = (-1.0, 0.5, 2.125)
    a = R.loss(pxyz, pout, gxyz)
    want = R.targets(pxyz, pout, gxyz)
    got = [t.cpu().numpy() for t in PS.proposal_targets(dict(proposals_xyz=T(pxyz, dev), proposals_output=T(pout, dev)),
                                                         dict(bboxes_xyz=T(gxyz, dev)))]
    for g_, w_ in zip(got, want):
        assert np.array_equal(g_, w_)
    label, near, dual, real = got
    assert real.tolist() == [4, 3] and dual.tolist() == [[0, 0, 0, 0], [3, 3, 64, -1]]
    assert near[0, :2].tolist() == [1, 1] and near[1, [3, 65, 64, 69]].tolist() == [0, 0, 2, 2]  # of two equal boxes, the first
    r = run_loss(dev, pxyz, pout, gxyz, R.fake_losses(1))
    assert r["guards"] and r["counts"] == [a["Np"], a["Nn"], a["G"]] == [6, 2 * p - 6, 7]
    assert np.array_equal(r["d_out"][..., 2:5].view(np.int32), a["d_ctr"].view(np.int32))
    assert np.array_equal(r["d_xyz"].view(np.int32), a["d_ctr"].view(np.int32))
    # proposal (0, 0) carries its own term and four dual terms, added in ascending j; its duplicate only its own
    inv_p, inv_g = F(1) / (F(6) + F(1e-6)), F(1) / (F(7) + F(1e-6))
    c = pxyz[0, 0]
    own = (F(2) * (c - gxyz[0, 1])) * inv_p
    acc = own
    for j in range(4):
        acc = acc + (F(2) * (c - gxyz[0, j])) * inv_g
    assert np.array_equal(r["d_xyz"][0, 0].view(np.int32), acc.view(np.int32)) and np.array_equal(r["d_xyz"][0, 1].view(np.int32), own.view(np.int32))
    ref = R.loss64(pxyz, pout, gxyz)
    assert close(r["losses"][2], ref["obj"]) and close(r["losses"][3], ref["center"])


def test_a_scene_without_positives_one_without_negatives_and_an_all_grey_batch(hiplib, dev):
    b, p = 3, 40
    pxyz, pout, gxyz = R.random_case(23, b, p, 4, 8)
    rng = np.random.default_rng(6)
    pxyz[0] = (gxyz[0, rng.integers(0, 4, p)] + np.array([0, 5.0, 0]) + rng.normal(0, 0.3, (p, 3))).astype(F)   # far above: all negative
    pxyz[1] = (gxyz[1, rng.integers(0, 4, p)] + rng.normal(0, 0.05, (p, 3))).astype(F)                          # next to a centre: all positive
    a, ref = R.loss(pxyz, pout, gxyz), R.loss64(pxyz, pout, gxyz)
    assert ref["margin_thr"] > 1e-4 and a["scenes"][0]["neg"].all() and a["scenes"][1]["pos"].all() and 0 < a["scenes"][2]["pos"].sum() < p
    l0 = R.fake_losses(2)
    r = run_loss(dev, pxyz, pout, gxyz, l0)
    assert r["guards"] and r["counts"] == [a["Np"], a["Nn"], a["G"]]
    assert np.array_equal(r["d_out"][..., 2:5].view(np.int32), a["d_ctr"].view(np.int32))
    assert np.array_equal(r["d_xyz"].view(np.int32), a["d_ctr"].view(np.int32))
    assert close(r["d_out"][..., :2], ref["d_out"][..., :2], 1e-3) and close(r["losses"][2], ref["obj"]) and close(r["losses"][3], ref["center"])
    # all grey: 0.45 from the first centre, the other boxes far away.  M = 0 and Np = 0 give zeros, not the reference's NaN
    grey = (gxyz[:, :1] + np.array([0.45, 0, 0], F)) + np.zeros((b, p, 3), F)
    gfar = gxyz.copy()
    gfar[:, 1:] += F(50.0)
    a, ref = R.loss(grey, pout, gfar), R.loss64(grey, pout, gfar)
    r = run_loss(dev, grey, pout, gfar, l0)
    l = r["losses"]
    assert r["guards"] and r["counts"] == [0, 0, a["G"]] and l[2] == 0.0 and np.isfinite(l).all()
    assert not r["d_out"][..., :2].view(np.int32).any()
    assert np.array_equal(r["d_xyz"].view(np.int32), a["d_ctr"].view(np.int32)) and np.isfinite(r["d_xyz"]).all()
    assert close(l[3], ref["center"]) and np.array_equal(l.view(np.int32), R.reform(l0, l[2], l[3]).view(np.int32))


@pytest.mark.parametrize("first", [False, True], ids=["inside-the-scene", "at-proposal-0"])
def test_nan_and_inf_in_a_position_and_in_an_offset(hiplib, dev, first):
    """Non-finite values go where the rule sends them and nowhere else: equal to the restatement (NaN where it is NaN), guards intact.
    A NaN at proposal 0 is the first candidate of every box's minimum and sticks."""
    from votenet_amd import proposal_supervision as PS
    b, p = 2, 70
    pxyz, pout, gxyz = R.random_case(29, b, p, 5, 8)
    pos = [np.nonzero(s["pos"])[0] for s in R.loss(pxyz, pout, gxyz)["scenes"]]
    pxyz, pout = pxyz.copy(), pout.copy()
    pxyz[0, 0 if first else 5, 1] = np.nan            # a NaN position: grey, its centre wins no box -- unless it is the first candidate
    pxyz[0, 66] = np.inf                              # an infinite position: negative, infinitely far from every box
    pout[1, 0 if first else int(pos[1][-1]), 3] = np.nan   # a NaN offset (at a positive proposal when not first)
    pout[1, int(pos[1][1]), 2] = np.inf               # an infinite offset at a positive proposal
    a = R.loss(pxyz, pout, gxyz)
    want = R.targets(pxyz, pout, gxyz)
    got = [t.cpu().numpy() for t in PS.proposal_targets(dict(proposals_xyz=T(pxyz, dev), proposals_output=T(pout, dev)),
                                                         dict(bboxes_xyz=T(gxyz, dev)))]
    for g_, w_ in zip(got, want):
        assert np.array_equal(g_, w_)
    assert (got[2][0, :5] == 0).all() == first and got[0][0, 66] == 0 and got[0][0, 0 if first else 5] == -1
    l0 = R.fake_losses(4)
    r = run_loss(dev, pxyz, pout, gxyz, l0)
    assert r["guards"] and r["counts"] == [a["Np"], a["Nn"], a["G"]]
    assert np.array_equal(r["d_out"][..., 2:5], a["d_ctr"], equal_nan=True) and np.array_equal(r["d_xyz"], a["d_ctr"], equal_nan=True)
    assert np.array_equal(r["d_xyz"].view(np.int32), r["d_out"][..., 2:5].view(np.int32))
    assert not np.isfinite(a["d_ctr"]).all() and np.isfinite(a["d_ctr"]).sum() >= a["d_ctr"].size - 12
    assert np.allclose(r["d_out"][..., :2], a["d_obj"], rtol=1e-5, atol=1e-8) and (r["d_out"][..., 5:] == PATTERN).all()
    l = r["losses"]
    print("first", first, "obj", l[2], a["obj"], "center", l[3], a["center"])
    assert same(l[2], a["obj"]) and same(l[3], a["center"]) and not np.isfinite(l[3]) and np.isfinite(l[2])
    assert np.array_equal(l[KEEP].view(np.int32), l0[KEEP].view(np.int32))


def test_shapes_past_the_limits_are_refused_and_nothing_is_launched(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import proposal_supervision as PS
    for p, bb, text in ((1025, 4, "1 to 1024 proposals per scene, got p = 1025"), (16, 257, "1 to 256 boxes per scene, got bb = 257")):
        out = dict(proposals_xyz=torch.zeros((1, p, 3), device=dev), proposals_output=torch.zeros((1, p, W), device=dev))
        g = dict(bboxes_xyz=torch.zeros((1, bb, 3), device=dev))
        l0 = R.fake_losses(1)
        losses, d_xyz = T(l0, dev), torch.full((1, p, 3), PATTERN, device=dev)
        with pytest.raises(L.InvalidArgumentError, match=text):
            PS.paper_proposal_loss(out, g, losses, d_xyz=d_xyz)
        with pytest.raises(L.InvalidArgumentError, match=text):
            PS.proposal_targets(out, g)
        torch.cuda.synchronize()
        assert (d_xyz == PATTERN).all() and torch.equal(bits(losses), bits(l0))


# ------------------------------------------------------------------ the train step
def _batch(dev, seed):
    from votenet_amd import loss as VL
    from votenet_amd import synth
    gt_np = synth.room_gt(B, NPTS, seed)
    return torch.from_numpy(synth.room_batch(B, NPTS, seed)).to(dev), VL.gt_to_device(gt_np, dev), gt_np


def _net(dev, seed):
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL)
    net.init_optimizer(1e-3)
    return net


OUT_KEYS = ("seeds_xyz", "votes_xyz", "proposals_xyz", "proposals_output")


def _recomputed(out, gt, votes=False, proposals=True):
    """votenet_loss and the modes' launches again on a step's own forward results -> (the reference's 12 floats, the modes', the
    reference's cotangents, the modes' cotangents)."""
    from votenet_amd import loss as VL
    from votenet_amd import proposal_supervision as PS
    from votenet_amd import vote_supervision as VS
    ref, cot = VL.votenet_loss(out, gt)
    ref_cot = {k: v.clone() for k, v in cot.items()}
    paper = ref.clone()
    if votes:
        VS.paper_vote_loss(out, gt, paper, d_votes=cot["votes_xyz"])
    if proposals:
        PS.paper_proposal_loss(out, gt, paper, d_xyz=cot["proposals_xyz"], d_out=cot["proposals_output"])
    return ref.cpu().numpy(), paper.cpu().numpy(), ref_cot, cot


def test_plain_path_a_paper_step_changes_the_two_terms_and_nothing_else(hiplib, dev):
    """The bit-reproducible mode (mlp.set_deterministic).  Two networks from one seed, one step on one batch, one with the mode on (and
    the monitors, whose ring must record the re-formed total): the forward results and the eight other loss values are the same bits;
    last_losses[0, 2, 3, 9] of the paper step are paper_proposal_loss's on its own forward results; relative to the default loss only
    those four values and the two proposal cotangents differ; and its gradient bucket is, bit for bit, the bucket of a hand-assembled
    pass on a third network -- forward, votenet_loss, the launch into its cotangents, backward."""
    from votenet_amd import loss as VL
    from votenet_amd import mlp as M
    from votenet_amd import proposal_supervision as PS
    x, gt, gt_np = _batch(dev, 440)
    keys = OUT_KEYS + ("seeds_points", "votes_points")
    prev = M.set_deterministic(True)
    try:
        off, on, hand = _net(dev, 9), _net(dev, 9), _net(dev, 9)
        on.enable_proposal_supervision("paper")
        mon = on.enable_monitors(window=4)
        out_off = {k: v.clone() for k, v in off.train_step(x, gt=gt).items() if k in keys}
        out_on = {k: v.clone() for k, v in on.train_step(x, gt=gt).items() if k in keys}
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(bits(out_off[k]), bits(out_on[k])), k
        l_off, l_on = off.last_losses.cpu().numpy(), on.last_losses.cpu().numpy()
        assert np.array_equal(l_off[KEEP].view(np.int32), l_on[KEEP].view(np.int32))
        ref, paper, ref_cot, cot = _recomputed(out_on, gt)
        assert np.array_equal(ref.view(np.int32), l_off.view(np.int32)) and np.array_equal(paper.view(np.int32), l_on.view(np.int32))
        a = R.loss(out_on["proposals_xyz"].cpu().numpy(), out_on["proposals_output"].cpu().numpy(), gt_np["bboxes_xyz"], losses=l_off)
        print("Np Nn G", a["Np"], a["Nn"], a["G"], "obj reference", l_off[2], "paper", l_on[2], a["obj"], "center", l_off[3], l_on[3],
              a["center"], "total", l_off[0], l_on[0])
        assert a["Np"] == l_off[10] and a["Nn"] == l_off[11] > 0
        assert close(l_on[2], a["obj"]) and close(l_on[3], a["center"]) and np.array_equal(l_on, R.reform(l_off, l_on[2], l_on[3]), equal_nan=True)
        assert all(l_on[k] != l_off[k] for k in (0, 2, 3, 9))
        assert torch.equal(bits(cot["votes_xyz"]), bits(ref_cot["votes_xyz"]))
        assert torch.equal(bits(cot["proposals_output"][..., 5:]), bits(ref_cot["proposals_output"][..., 5:]))
        assert torch.equal(bits(cot["proposals_xyz"]), bits(a["d_ctr"])) and torch.equal(bits(cot["proposals_output"][..., 2:5]), bits(a["d_ctr"]))
        assert not torch.equal(bits(cot["proposals_xyz"]), bits(ref_cot["proposals_xyz"]))
        assert not torch.equal(bits(cot["proposals_output"][..., :2]), bits(ref_cot["proposals_output"][..., :2]))
        assert np.float32(mon.read()["last"]["total_cost"]).view(np.int32) == l_on[:1].view(np.int32)[0]
        # the hand-assembled pass: first with votenet_loss's own cotangents (the control: it must be the reference step's bucket)
        for launch, step in ((False, off), (True, on)):
            hand.store.grad.zero_()
            hand.store.refresh_transposes()
            tape = []
            out_h = hand.forward(x, tape)
            assert torch.equal(bits(out_h["proposals_output"]), bits(out_on["proposals_output"]))
            losses_h, cot_h = VL.votenet_loss(out_h, gt)
            if launch:
                PS.paper_proposal_loss(out_h, gt, losses_h, d_xyz=cot_h["proposals_xyz"], d_out=cot_h["proposals_output"])
            hand.backward(tape, cot_h)
            torch.cuda.synchronize()
            assert torch.equal(bits(hand.store.grad), bits(step.store.grad)), \
                "the %s step's gradient is not the hand-assembled one" % ("paper" if launch else "reference")
        assert not torch.equal(bits(off.store.grad), bits(on.store.grad))
    finally:
        M.set_deterministic(prev)
    assert off.proposal_supervision is None and not hasattr(off, "_loss_tail_work")


def test_graph_path_every_replayed_step_carries_the_paper_terms(hiplib, dev):
    """The default mode (atomics: not repeatable even against itself, so no second network to compare bits with), the stretch replayed
    from its captured graphs with the launch between two segments: what is exact there.  Every step: the loss vector is votenet_loss's
    on THAT step's forward results with the modes' launches behind it, bit for bit -- with the paper's vote supervision on as well,
    losses[0] is the total of both --, the buffers the next segment read hold the paper's cotangents, and the monitors' ring holds the
    re-formed total.  Switching the mode captures no graph again."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    batches = [_batch(dev, s) for s in (450, 452, 454, 456, 458, 460)]
    net = _net(dev, 10)
    mon = net.enable_monitors(window=16)
    modes = [(False, True), (False, True), (False, True), (False, False), (True, True), (False, True)]  # (votes, proposals) per step
    ngraphs = []
    for (x, gt, gt_np), (votes, props) in zip(batches, modes):
        net.enable_vote_supervision("paper") if votes else net.disable_vote_supervision()
        net.enable_proposal_supervision("paper") if props else net.disable_proposal_supervision()
        out = net.train_step(x, gt=gt)
        step_out = {k: out[k].clone() for k in OUT_KEYS}
        got = net.last_losses.cpu().numpy()
        graphs = net.__dict__.get("_stretch_graphs", {})
        ngraphs.append(len(graphs))
        ref, paper, ref_cot, cot = _recomputed(step_out, gt, votes=votes, proposals=props)
        print("votes", votes, "proposals", props, "obj", got[2], "reference", ref[2], "center", got[3], ref[3], "total", got[0], ref[0])
        assert np.array_equal(got.view(np.int32), paper.view(np.int32))
        assert np.array_equal(got[[4, 5, 6, 7, 8, 10, 11]].view(np.int32), ref[[4, 5, 6, 7, 8, 10, 11]].view(np.int32))
        assert (not props and np.array_equal(got.view(np.int32), ref.view(np.int32))) or all(got[k] != ref[k] for k in (0, 2, 3, 9))
        assert votes == (got[1] != ref[1])
        assert np.float32(mon.read()["last"]["total_cost"]).view(np.int32) == got[:1].view(np.int32)[0]
        if props:
            a = R.loss(step_out["proposals_xyz"].cpu().numpy(), step_out["proposals_output"].cpu().numpy(), gt_np["bboxes_xyz"], losses=ref)
            assert close(got[2], a["obj"]) and close(got[3], a["center"]) and torch.equal(bits(cot["proposals_xyz"]), bits(a["d_ctr"]))
        if graphs and props:  # the cotangents the first backward segment read
            sg, = graphs.values()
            nv, npx, npo = cot["votes_xyz"].numel(), cot["proposals_xyz"].numel(), cot["proposals_output"].numel()
            flat = sg.loss_bufs[1]
            assert torch.equal(bits(flat[nv:nv + npx]), bits(cot["proposals_xyz"]).reshape(-1))
            assert torch.equal(bits(flat[nv + npx:nv + npx + npo].view(-1, W)[:, :5]), bits(cot["proposals_output"]).view(-1, W)[:, :5])
            assert torch.equal(bits(flat[:nv]), bits(cot["votes_xyz"]).reshape(-1))
    graphs = net.__dict__.get("_stretch_graphs", {})
    assert ngraphs[1:] == [1, 1, 1, 1, 1] and sum(g.replays for g in graphs.values()) >= 4, "the steps did not go through StretchGraph.replay"


FRESH = """
import sys
sys.path.insert(0, %r)
import torch
from votenet_amd import _lib, loss, synth
from votenet_amd.model import VoteNetHotPath
dev = torch.device("cuda:0")
net = VoteNetHotPath(dev, seed=0, npoints=(512, 256, 128, 64))
net.init_optimizer(1e-3)
x = torch.from_numpy(synth.room_batch(2, 4096, 7)).to(dev)
gt = loss.gt_to_device(synth.room_gt(2, 4096, 7), dev)
for _ in range(3):
    net.train_step(x, gt=gt)
torch.cuda.synchronize()
maps = open("/proc/self/maps").read()
assert "libvotenet_hip.so" in maps and net.proposal_supervision is None
assert not _lib.side_loaded("propsup") and "libvotenet_propsup" not in maps and "votenet_amd.proposal_supervision" not in sys.modules
net.enable_proposal_supervision("paper")
net.train_step(x, gt=gt)
torch.cuda.synchronize()
assert _lib.side_loaded("propsup") and "libvotenet_propsup.so" in open("/proc/self/maps").read()
assert not _lib.side_loaded("votesup")
print("fresh ok")
"""


def test_a_fresh_process_default_train_step_does_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr
