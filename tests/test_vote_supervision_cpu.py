"""CPU: the paper's vote supervision without a device -- the numpy float32 restatement of include/votenet_vote_supervision.h
(tests/vote_supervision_ref.py) against an independent float64 form (half-spaces of evaluator.box_corners, plain minimum over the
containing set, torch double autograd), the slot rule on nested boxes, its invariance under the edge padding of the ground truth, its
relation to the reference's vote loss where the two rules must agree, and the interface: the header's entries, the switch of
VoteNetHotPath, the library's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402
import vote_supervision_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402
from votenet_amd import synth  # noqa: E402

F = np.float32
NAMES = ["votenet_paper_vote_loss", "votenet_vote_targets", "votenet_votesup_last_error", "votenet_votesup_workspace_bytes"]
NPTS = 20480


def room(seed, n=1024):
    """n random points of the synthetic room `seed` as seeds (the seeds of the network ARE cloud points), and its ground truth."""
    cloud = synth.room_batch(1, NPTS, seed)
    pick = np.random.default_rng(seed).choice(NPTS, n, replace=False)
    return cloud[:, pick], synth.room_gt(1, NPTS, seed)


# ------------------------------------------------------------------ float32 rule against the float64 form
def test_float32_membership_equals_the_float64_half_spaces_outside_the_margin():
    """Pairs closer than 1e-5 m to a face plane (float32 rounds coordinates of a few metres to 2.4e-7 m, and the rotation adds a few of
    those) are left out -- at most 1 % of all pairs; every other pair agrees."""
    pairs = left_out = wrong = inside = multi = seeds_n = 0
    for seed in range(1000, 1008):
        seeds, gt = room(seed)
        a = (seeds[0], gt["bboxes_xyz"][0], gt["bboxes_lwh"][0], gt["bboxes_roty"][0])
        got, want, near = R.inside(*a), R.inside64(*a), R.near_face64(*a)
        pairs += got.size
        left_out += int(near.sum())
        wrong += int(((got != want) & ~near).sum())
        inside += int(want.any(1).sum())
        multi += int((want.sum(1) >= 2).sum())
        seeds_n += got.shape[0]
    print("%d pairs, %d left out (%.3f %%), %d disagree; %.1f %% of the seeds in a box, %.1f %% in two or more"
          % (pairs, left_out, 100.0 * left_out / pairs, wrong, 100.0 * inside / seeds_n, 100.0 * multi / seeds_n))
    assert wrong == 0
    assert left_out <= 0.01 * pairs
    assert inside >= 0.1 * seeds_n and multi > 0


# ------------------------------------------------------------------ the slot rule
def test_slots_for_zero_to_five_containing_boxes():
    """Five nested boxes, box j with half height (j + 1) / 4: a seed at height r lies in the boxes j >= 4 r - 1.  Slot 0 the first, slot 1
    the second, slot 2 the LAST (from the fourth box on the third is passed over); fewer: the first again; none: -1."""
    xyz, lwh, roty = R.nested_boxes(5)
    gt = dict(bboxes_xyz=xyz[None], bboxes_lwh=lwh[None], bboxes_roty=roty[None])
    heights = [1.5, 1.25, 1.0, 0.75, 0.5, 0.25, 1.0 + 1 / 64, -0.25, -1.25]
    seeds = np.array([[[0.0, h, 0.0] for h in heights]], F)
    slots, count = R.targets(seeds, gt)
    assert count[0].tolist() == [0, 1, 2, 3, 4, 5, 1, 5, 1]  # closed: a seed ON the face of box j (height (j + 1) / 4) is inside it
    assert slots[0].tolist() == [[-1, -1, -1], [4, 4, 4], [3, 4, 3], [2, 3, 4], [1, 2, 4], [0, 1, 4], [4, 4, 4], [0, 1, 4], [4, 4, 4]]
    # the charged target is the closest of the three slots, the first of equals
    votes = seeds.copy()
    votes[0, 5] = xyz[4] + F(0.125)           # next to the last box's centre: slot 2
    votes[0, 7] = xyz[2]                      # on the centre of a box that is in the set but in no slot: slot 1, box 2's nearer neighbour
    votes[0, 3, 0] = (xyz[2, 0] + xyz[3, 0]) / 2  # midway between slots 0 and 1 along x: the first
    out = R.loss(seeds, votes, gt)
    assert out["pick"][0].tolist() == [-1, 4, 3, 2, 1, 4, 4, 1, 4]
    assert out["P"] == 8 and not out["d_votes"][0, 0].any() and np.signbit(out["d_votes"][0, 0]).sum() == 0


def test_nonfinite_seeds_are_in_no_box_and_a_zero_size_box_holds_its_centre():
    xyz, lwh, roty = R.nested_boxes(2)
    lwh[1] = 0.0
    seeds = np.array([[np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 0, 0], [0, 0, np.nan], xyz[1], xyz[1] + F(2.0 ** -20)], F)
    ins = R.inside(seeds, xyz, lwh, roty)
    assert ins.tolist() == [[False, False]] * 4 + [[True, True], [True, False]]
    lwh[0, 1] = np.nan  # a NaN extent: that box holds nothing
    assert not R.inside(seeds, xyz, lwh, roty)[:, 0].any()


# ------------------------------------------------------------------ padding
def test_edge_padding_changes_neither_the_target_centres_nor_the_loss():
    rng = np.random.default_rng(5)
    for seed in (1000, 1003):
        seeds, gt = room(seed, 512)
        # the last box gets company: seeds inside it, and a second box around it, so that padding copies of it enter sets of 1, 2 and 3
        gt["bboxes_xyz"][0, -2], gt["bboxes_lwh"][0, -2] = gt["bboxes_xyz"][0, -1] + F(0.0625), gt["bboxes_lwh"][0, -1] * F(1.5)
        gt["bboxes_roty"][0, -2] = gt["bboxes_roty"][0, -1]
        seeds[0, :64] = gt["bboxes_xyz"][0, -1] + (rng.random((64, 3)) - 0.5).astype(F) * gt["bboxes_lwh"][0, -1][[0, 2, 1]] * F(0.5)
        votes = (seeds + rng.normal(0, 0.3, seeds.shape)).astype(F)
        padded = R.edge_pad(gt, 3)
        assert padded["bboxes_xyz"].shape[1] == gt["bboxes_xyz"].shape[1] + 3
        a, b = R.loss(seeds, votes, gt), R.loss(seeds, votes, padded)
        assert (b["count"] > a["count"]).any() and ((a["count"] > 0) == (b["count"] > 0)).all()
        ca, cb = gt["bboxes_xyz"][0][a["slots"][0]], padded["bboxes_xyz"][0][b["slots"][0]]  # (n, 3 slots, 3)
        for i in np.nonzero(a["count"][0])[0]:
            assert {tuple(c) for c in ca[i]} == {tuple(c) for c in cb[i]}, i
        assert a["P"] == b["P"] and a["L"].view(np.int32) == b["L"].view(np.int32)
        assert np.array_equal(a["d_votes"].view(np.int32), b["d_votes"].view(np.int32))


# ------------------------------------------------------------------ the gradient
def overlapping_case(seed, b=2, n=256, bb=5):
    """Random rotated boxes that overlap, seeds around them; moved away from every decision float32 and float64 could take differently:
    no seed within 1e-4 m of a face, in more than three boxes (the float64 form takes the minimum over ALL containing boxes), with a
    component of v - t within 1e-4 of zero for a slot's t, or with two slot distances within 1e-4.  Offenders are moved out of every box."""
    seeds, votes, _, _, gt = loss_ref.random_case(seed, b=b, n=n, p=8, bb=bb)
    gt["bboxes_lwh"] *= F(2.5)
    far = np.array([50.0, 50.0, 50.0], F)
    for sc in range(b):
        a = (seeds[sc], gt["bboxes_xyz"][sc], gt["bboxes_lwh"][sc], gt["bboxes_roty"][sc])
        ins = R.inside64(*a)
        d = np.abs(votes[sc].astype(np.float64)[:, None] - gt["bboxes_xyz"][sc].astype(np.float64)[None])     # (n,bb,3)
        dist = np.where(ins, d.sum(-1), np.inf)
        srt = np.sort(dist, 1)
        with np.errstate(invalid="ignore"):
            close = (np.diff(srt[:, :4], axis=1) < 1e-4) & np.isfinite(srt[:, 1:4])
        bad = R.near_face64(*a, margin=1e-4).any(1) | (ins.sum(1) > 3) | ((d < 1e-4).any(-1) & ins).any(1) | close.any(1)
        seeds[sc, bad] = far
    return seeds, votes, gt


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_loss_and_gradient_equal_float64_autograd(seed):
    seeds, votes, gt = overlapping_case(seed)
    got = R.loss(seeds, votes, gt)
    L, v, P, ins = R.loss64(seeds, votes, gt)
    L.backward()
    assert got["P"] == P and np.array_equal(got["count"], ins.sum(-1))
    assert (got["count"] == 2).sum() >= 10 and (got["count"] == 3).sum() >= 3 and (got["count"] == 0).sum() >= 10
    assert got["gap"] >= 1e-4 * 0.99
    print("P", P, "L", got["L"], float(L.detach()), "sets of 1/2/3:", [(got["count"] == k).sum() for k in (1, 2, 3)])
    assert abs(float(got["L"]) - float(L.detach())) <= 1e-5 * max(1.0, abs(float(L.detach())))
    g = v.grad.numpy()
    assert np.abs(got["d_votes"] - g).max() <= 1e-5 * max(1e-3, np.abs(g).max())
    assert not got["d_votes"][got["count"] == 0].any()


# ------------------------------------------------------------------ relation to the reference's loss
def test_on_far_apart_cubes_the_sum_is_the_references_sum():
    seeds, votes, prop, out, gt = R.cube_case(7)
    T = lambda a: torch.from_numpy(np.asarray(a)).double() if np.asarray(a).dtype == F else torch.from_numpy(np.asarray(a))
    ref = loss_ref.votenet_loss(T(seeds), T(votes), T(prop), T(out), {k: T(v) for k, v in gt.items()})
    got = R.loss(seeds, votes, gt)
    b, n = seeds.shape[:2]
    assert got["P"] == int(ref["surface_ind"].sum()) and 0.05 * b * n < got["P"] < 0.5 * b * n
    assert np.array_equal(got["pick"][got["count"] > 0], ref["votes_assignment"].numpy()[got["count"] > 0])
    lhs, rhs = float(got["L"]) * (got["P"] + 1e-6), float(ref["vote_reg_loss"]) * b * n
    print("P", got["P"], "L (P + 1e-6)", lhs, "reference vote_reg_loss B n", rhs)
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(rhs))


# ------------------------------------------------------------------ the interface
def test_header_declares_the_four_entries_and_the_binding_follows_it(hiplib):
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, L.SIDE_LIBS["votesup"])) as f:
        protos = L.parse_header(f.read(), {})
    I, V = ctypes.c_int, ctypes.c_void_p
    assert sorted(protos) == NAMES
    assert protos["votenet_votesup_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_votesup_workspace_bytes"] == (ctypes.c_size_t, [I])
    assert protos["votenet_vote_targets"] == (I, [I, I, I] + [V] * 7)
    assert protos["votenet_paper_vote_loss"] == (I, [I, I, I] + [V] * 10)
    lib = L.side_lib("votesup")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == protos[name]


def test_the_mode_is_off_by_default_and_an_unknown_mode_is_refused():
    from votenet_amd import vote_supervision as VS
    from votenet_amd.model import VoteNetHotPath
    assert VS.MODES == ("reference", "paper")
    assert VoteNetHotPath.vote_supervision is None
    net = object.__new__(VoteNetHotPath)  # the switch needs no device
    assert net.vote_supervision is None
    with pytest.raises(L.InvalidArgumentError, match="nonsense"):
        net.enable_vote_supervision("nonsense")
    assert net.vote_supervision is None
    net.enable_vote_supervision()
    assert net.vote_supervision == "paper"
    net.enable_vote_supervision("reference")
    assert net.vote_supervision == "reference"
    net.disable_vote_supervision()
    assert net.vote_supervision is None


def test_the_library_checks_its_arguments_before_anything_is_launched(hiplib):
    """Every invalid-argument case returns 1 with the limit in the text: no device is needed."""
    lib = L.side_lib("votesup")
    buf = np.zeros(4096, F)
    p = buf.ctypes.data
    err = lambda: lib.votenet_votesup_last_error().decode()

    def tg(b=2, n=16, bb=4, seeds=p, xyz=p, lwh=p, roty=p, slots=p, count=p):
        return lib.votenet_vote_targets(b, n, bb, seeds, xyz, lwh, roty, slots, count, None)

    def pl(b=2, n=16, bb=4, seeds=p, votes=p, xyz=p, lwh=p, roty=p, losses=p, d_votes=p + 8192, sup=None, ws=p):
        return lib.votenet_paper_vote_loss(b, n, bb, seeds, votes, xyz, lwh, roty, losses, d_votes, sup, ws, None)
    for fn in (tg, pl):
        for kw, text in ((dict(bb=257), "1 to 256 boxes per scene, got bb = 257"), (dict(bb=0), "1 to 256 boxes"), (dict(b=0), "1 to 65535 scenes"),
                         (dict(b=65536), "got b = 65536"), (dict(n=0), "n >= 1"), (dict(b=60000, n=60000), "2^31"),
                         (dict(seeds=None), "null"), (dict(xyz=None), "null"), (dict(lwh=None), "null"), (dict(roty=None), "null")):
            assert fn(**kw) == 1, kw
            assert text in err(), (kw, err())
    for kw in (dict(slots=None), dict(count=None)):
        assert tg(**kw) == 1 and "null" in err()
    for kw, text in ((dict(votes=None), "null"), (dict(losses=None), "null"), (dict(d_votes=None), "null"), (dict(ws=None), "null"),
                     (dict(d_votes=p), "may not overlap"), (dict(d_votes=p + 2 * 16 * 12 - 4), "may not overlap"), (dict(ws=p + 2), "4-byte aligned")):
        assert pl(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert lib.votenet_votesup_workspace_bytes(8) == 16 + 8 * 4 and lib.votenet_votesup_workspace_bytes(-3) == 16
    with pytest.raises(L.InvalidArgumentError, match=r"1 to 256 boxes per scene, got bb = 257"):
        L.check(tg(bb=257), side="votesup")
