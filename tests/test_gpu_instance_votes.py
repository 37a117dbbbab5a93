"""GPU: vote supervision from instance labels on the device -- votenet_seed_points and votenet_instance_vote_loss
(csrc/instvote/instance_votes.hip) against the float32 restatement tests/instance_votes_ref.py, bit for bit in every pick, count and
cotangent, and against its float64 form in the loss values; indices out of range; the relation to the merged paper mode where the two
rules must agree, and the case in which they must not; and VoteNetHotPath.enable_instance_votes: the seeds are the cloud points the
tape's indices name, a step with the mode on is the step whose vote term was replaced by hand, on the launch path and through the
replayed graphs with prefetched geometry; a step with the mode off never loads the library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_votes_ref as R  # noqa: E402
import vote_supervision_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
# b x n x bb: a lone seed, under / at a wave, a lane tail, the real seed count (one pass of a workgroup), more than one pass; one box,
# a few, LOSS_MAXBOX.  n1 = 2 n, n0 = 4 n + 5 (instance_votes_ref.levels_case)
SHAPES = [(b, n, bb) for b in (1, 3) for n in (1, 63, 64, 257, 1024, 1500) for bb in (1, 7, 256)]
IDS = lambda s: "b%d-n%d-bb%d" % s
B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the train-step shapes of tests/test_gpu_vote_supervision.py
CANARY, GUARD = 0x5A5AA5A5, 64  # an int32 word no result is (1.5e16 as a float), 64 of them on either side of every output


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    t = t.detach().contiguous().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def close(got, want):
    """the project's tolerance on loss values: 1e-5 relative, floor 1.0 (tests/test_gpu_loss.py); a non-finite value must be the same"""
    got, want = float(got), float(want)
    if not np.isfinite(want):
        return (np.isnan(want) and np.isnan(got)) or got == want
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def guarded(dev, shape, dtype, init=None):
    """-> (a contiguous tensor of `shape` inside a larger buffer with GUARD canary words before and behind it, the buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device=dev)
    view = buf[GUARD:GUARD + n].view(dtype).view(shape)
    if init is not None:
        view.copy_(init) if isinstance(init, torch.Tensor) else view.fill_(init)
    return view, buf


def intact(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


def fake_losses(seed=3):
    """12 floats as votenet_loss leaves them: every component its own value, the total composed from them."""
    l = np.random.default_rng(seed).random(12).astype(F) + F(0.25)
    l[0] = R.total(l, l[1])
    return l


def device_run(dev, idx1, idx2, point_box, votes, xyz, l0):
    """Both entries on guarded outputs; the loss twice over ONE workspace.  -> dict of host results.  Asserted here: every canary word
    is intact, the workspace is zero after each call, the two calls wrote the same bytes."""
    from votenet_amd import instance_votes as IV
    b, n = idx2.shape
    d1, d2, pb = T(idx1, dev), T(idx2, dev), T(point_box, dev)
    out, gt = dict(votes_xyz=T(votes, dev)), dict(bboxes_xyz=T(xyz, dev), point_box=pb)
    sp = IV.seed_points(d1, d2, point_box.shape[1])
    assert sp.dtype == torch.int32 and tuple(sp.shape) == (b, n)
    lib_out, lib_buf = guarded(dev, (b, n), torch.int32)  # the entry itself, on a guarded buffer
    from votenet_amd import _lib as L
    L.check(L.side_lib("instvote").votenet_seed_points(b, point_box.shape[1], idx1.shape[1], n, L.ptr(d1), L.ptr(d2), L.ptr(lib_out),
                                                       L.stream_ptr()), side="instvote")
    work, work_buf = guarded(dev, tuple(IV.workspace(b, dev).shape), torch.int32, init=0)
    runs = []
    for _ in range(2):
        losses, losses_buf = guarded(dev, (12,), torch.float32, init=T(l0, dev))
        d_votes, dv_buf = guarded(dev, (b, n, 3), torch.float32, init=-7.0)
        counts, counts_buf = guarded(dev, (2,), torch.int32)
        dv, c = IV.instance_vote_loss(out, gt, losses, (d1, d2), d_votes=d_votes, counts=counts, work=work)
        assert dv is d_votes and c.data_ptr() == counts.data_ptr()
        assert not work.any(), "the workspace is not left zero"
        assert all(intact(x) for x in (losses_buf, dv_buf, counts_buf, work_buf, lib_buf)), "a canary word round an output was written"
        runs.append((bits(losses), bits(d_votes), counts.cpu().tolist()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2], "two calls differ"
    assert torch.equal(sp, lib_out)
    return dict(seed_point=sp.cpu().numpy(), losses=losses.cpu().numpy(), d_votes=d_votes.cpu().numpy(), P=runs[0][2][0], Q=runs[0][2][1])


def check(got, want, l0, w64=None, what=""):
    """Device results against the float32 restatement (exact) and, in the loss values, the float64 form (the project's tolerance)."""
    assert np.array_equal(got["seed_point"], want["seed_point"]), what
    assert (got["P"], got["Q"]) == (want["P"], want["Q"]), (what, got["P"], got["Q"], want["P"], want["Q"])
    assert np.array_equal(got["d_votes"].view(np.int32), want["d_votes"].view(np.int32)), what
    l = got["losses"]
    L64 = float(w64) if w64 is not None else float(want["L"])
    print(what, "P", got["P"], "Q", got["Q"], "L", l[1], "float32 form", want["L"], "float64 form", L64, "total", l[0], R.total(l0, L64))
    assert close(l[1], L64) and close(l[0], R.total(l0, L64)), what
    assert l[1].view(np.int32) == F(want["L"]).view(np.int32) or (np.isnan(l[1]) and np.isnan(want["L"])), what  # the device's order of the sum
    assert l[0].view(np.int32) == R.total(l0, l[1]).view(np.int32) or np.isnan(l[0]), what  # re-formed from the stored components
    assert np.array_equal(l[2:].view(np.int32), l0[2:].view(np.int32)), what


_cases = {}


def base_case(shape, repeated=False):
    """The inputs of a shape (random labels, every row in range) and their restated results, computed once and shared."""
    key = (shape, repeated)
    if key not in _cases:
        b, n, bb = shape
        idx1, idx2, n0 = R.levels_case(b, n, 100 + n, repeated)
        point_box, xyz = R.labels_case(b, n0, bb, 200 + n + bb)
        votes = R.votes_case(b, n, 300 + n)
        want = R.loss(idx1, idx2, point_box, votes, xyz)
        L64 = float(R.loss64(idx1, idx2, point_box, votes, xyz)[0].detach())
        _cases[key] = (idx1, idx2, point_box, votes, xyz, want, L64)
    return _cases[key]


# ------------------------------------------------------------------ both entries against the restatement
@pytest.mark.parametrize("repeated", [False, True], ids=["picks", "repeated"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_labels_equal_the_restatement(hiplib, dev, shape, repeated):
    idx1, idx2, point_box, votes, xyz, want, L64 = base_case(shape, repeated)
    l0 = fake_losses()
    check(device_run(dev, idx1, idx2, point_box, votes, xyz, l0), want, l0, L64, "random")
    assert want["Q"] == 0 and (want["P"] > 0 or shape[1] < 63)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_special_labels_and_votes(hiplib, dev, shape):
    """All seeds unlabelled; all seeds supervised by one box; votes equal to their targets; NaN and Inf votes."""
    b, n, bb = shape
    idx1, idx2, point_box, votes, xyz, base, _ = base_case(shape)
    l0 = fake_losses(5)
    # no supervised seed: zero loss, an all-zero cotangent (the workspace left zero: device_run)
    none = np.full_like(point_box, -1)
    got = device_run(dev, idx1, idx2, none, votes, xyz, l0)
    check(got, R.loss(idx1, idx2, none, votes, xyz), l0, 0.0, "unlabelled")
    assert got["P"] == 0 and got["Q"] == 0 and got["losses"][1] == 0.0 and not got["d_votes"].view(np.int32).any()
    # one box takes every seed
    one = np.full_like(point_box, bb - 1)
    got = device_run(dev, idx1, idx2, one, votes, xyz, l0)
    check(got, R.loss(idx1, idx2, one, votes, xyz), l0, float(R.loss64(idx1, idx2, one, votes, xyz)[0].detach()), "one box")
    assert got["P"] == b * n
    # votes ON their targets: distance 0, cotangent +0.0 (sgn(0) = 0), still supervised
    on = votes.copy()
    sup = base["supervised"]
    hit = sup & (np.arange(n)[None] % 2 == 0)
    on[hit] = np.take_along_axis(xyz, np.where(sup, base["row"], 0)[..., None].astype(np.int64), 1)[hit]
    want = R.loss(idx1, idx2, point_box, on, xyz)
    got = device_run(dev, idx1, idx2, point_box, on, xyz, l0)
    check(got, want, l0, float(R.loss64(idx1, idx2, point_box, on, xyz)[0].detach()), "vote = target")
    assert got["P"] == base["P"] and not got["d_votes"][hit].view(np.int32).any() and not want["dist"][hit].any()
    # NaN and Inf votes: at an unsupervised seed nothing of them arrives; at a supervised one the loss is NaN / Inf, the cotangent finite
    for value in (np.nan, np.inf, -np.inf):
        bad = votes.copy()
        bad[~sup] = value
        want = R.loss(idx1, idx2, point_box, bad, xyz)
        assert want["L"].view(np.int32) == base["L"].view(np.int32)
        check(device_run(dev, idx1, idx2, point_box, bad, xyz, l0), want, l0, None, "%r at the unsupervised seeds" % value)
        if base["P"]:
            s, j = (int(a[0]) for a in np.nonzero(sup))
            bad = votes.copy()
            bad[s, j, 1] = value
            want = R.loss(idx1, idx2, point_box, bad, xyz)
            got = device_run(dev, idx1, idx2, point_box, bad, xyz, l0)
            check(got, want, l0, None, "%r at a supervised seed" % value)
            assert not np.isfinite(got["losses"][1]) and np.isfinite(got["d_votes"]).all()
            assert got["d_votes"][s, j, 1] == (0.0 if np.isnan(value) else np.sign(value) * want["inv"])


# ------------------------------------------------------------------ indices out of range
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_poisoned_indices(hiplib, dev, shape):
    """-1, n1, n0, bb, INT_MIN, INT_MAX written into idx2, idx1 and point_box at every fifth seed's link of the chain (the picks are
    permutation prefixes: a link belongs to one seed).  A value outside its tensor's bound leaves those seeds unsupervised, counted in
    Q (a negative box row is not); one inside it is just another index.  Every other seed keeps its point and its target.  (No index
    addresses anything unchecked: device_run's canary words, and the run itself.)"""
    b, n, bb = shape
    idx1, idx2, point_box, votes, xyz, base, _ = base_case(shape)
    n1, n0 = idx1.shape[1], point_box.shape[1]
    l0 = fake_losses(7)
    J = np.arange(0, n, 5)
    hit = np.zeros((b, n), bool)
    hit[:, J] = True
    for which, bound in (("idx2", n1), ("idx1", n0), ("point_box", bb)):
        for value in (-1, n1, n0, bb, R.INT_MIN, R.INT_MAX):
            p1, p2, pb = idx1.copy(), idx2.copy(), point_box.copy()
            for s in range(b):
                if which == "idx2":
                    p2[s, J] = value
                elif which == "idx1":
                    p1[s, idx2[s, J]] = value
                else:
                    pb[s, base["seed_point"][s, J]] = value
            want = R.loss(p1, p2, pb, votes, xyz)
            got = device_run(dev, p1, p2, pb, votes, xyz, l0)
            what = "%s <- %d" % (which, value)
            check(got, want, l0, None, what)
            out_of_range = value < 0 or value >= bound
            if out_of_range:
                assert not got["d_votes"][hit].view(np.int32).any(), what
                assert got["Q"] == (0 if which == "point_box" and value < 0 else hit.sum()), what
                assert got["P"] == int((base["supervised"] & ~hit).sum()), what
                assert which == "point_box" or (got["seed_point"][hit] == -1).all(), what
            else:
                assert got["Q"] == 0, what
            # every other seed: the same point, the same target (the sign pattern; the scale follows P)
            assert np.array_equal(got["seed_point"][~hit], base["seed_point"][~hit]), what
            assert np.array_equal(np.sign(got["d_votes"][~hit]), np.sign(base["d_votes"][~hit])), what


# ------------------------------------------------------------------ the relation to the merged paper mode
def _cubes(b, bb):
    """bb unit cubes three apart along x per scene, heading 0: disjoint, so a point lies in at most one."""
    xyz = np.zeros((b, bb, 3), F)
    for s in range(b):
        for j in range(bb):
            xyz[s, j] = (3.0 * j - 4.0, 0.25 * s, 2.0 + 3.0 * s)
    return dict(bboxes_xyz=xyz, bboxes_lwh=np.ones((b, bb, 3), F), bboxes_roty=np.zeros((b, bb), F))


@pytest.mark.parametrize("shape", [(1, 64, 1), (3, 257, 7), (3, 1500, 7)], ids=IDS)
def test_on_disjoint_boxes_it_is_the_paper_mode_bit_for_bit(hiplib, dev, shape):
    """No numpy reference: the seeds are cloud points, point_box is the one box vote_supervision.vote_targets finds the POINT in, so
    both rules supervise the same seeds towards the same centres: losses[0], losses[1], the cotangent and P are the same bits."""
    from votenet_amd import instance_votes as IV
    from votenet_amd import vote_supervision as VS
    b, n, bb = shape
    rng = np.random.default_rng(n)
    idx1, idx2, n0 = R.levels_case(b, n, 40 + n)
    gt_np = _cubes(b, bb)
    cloud = (gt_np["bboxes_xyz"][np.arange(b)[:, None], rng.integers(0, bb, (b, n0))] + rng.uniform(-0.9, 0.9, (b, n0, 3))).astype(F)
    gt = {k: T(v, dev) for k, v in gt_np.items()}
    x, d1, d2 = T(cloud, dev), T(idx1, dev), T(idx2, dev)
    slots, count = VS.vote_targets(x, gt)
    assert int(count.max()) == 1 and 0.05 < float(count.float().mean()) < 0.6
    gt["point_box"] = torch.where(count == 1, slots[..., 0], torch.full_like(count, -1)).contiguous()
    sp = IV.seed_points(d1, d2, n0)
    seeds = torch.gather(x, 1, sp.long()[..., None].expand(b, n, 3)).contiguous()
    out = dict(seeds_xyz=seeds, votes_xyz=T((seeds.cpu().numpy() + rng.normal(0, 0.3, (b, n, 3))).astype(F), dev))
    l0 = fake_losses(9)
    la, lb = T(l0, dev), T(l0, dev)
    dv_paper, sup = VS.paper_vote_loss(out, gt, la)
    dv_inst, counts = IV.instance_vote_loss(out, gt, lb, (d1, d2))
    print(shape, "P", int(sup), counts.tolist(), "L", float(la[1]), float(lb[1]))
    assert int(sup) == int(counts[0]) and int(counts[1]) == 0 and (int(sup) > 0 or n < 63)
    assert torch.equal(bits(la), bits(lb)) and torch.equal(bits(dv_paper), bits(dv_inst))


def test_nested_instances_and_unlabelled_points_in_a_hull(hiplib, dev):
    """What the mode is for.  A chair (box 1) stands inside the table's hull (box 0), and floor points lie inside that hull too.  Every
    cloud point is a seed.  The in-box rule (paper_vote_loss) pulls the floor points to the table's centre and charges a chair point the
    nearer of the two centres; the instance rule leaves the floor points alone (+0.0f) and sends every chair point to the chair's centre.
    Each equals its restatement bit for bit, and they differ where and how the restatements say."""
    from votenet_amd import instance_votes as IV
    from votenet_amd import vote_supervision as VS
    rng = np.random.default_rng(12)
    table_c, chair_c = np.array([0.0, 0.0, 2.0], F), np.array([0.5, -0.5, 2.0], F)
    gt_np = dict(bboxes_xyz=np.array([[table_c, chair_c]], F), bboxes_lwh=np.array([[[2, 2, 2], [0.5, 0.5, 0.5]]], F),
                 bboxes_roty=np.zeros((1, 2), F))

    def in_hull_not_chair(k):
        p = rng.uniform(-0.95, 0.95, (4 * k, 3))
        p = p[(np.abs(p - (chair_c - table_c)) > 0.3).any(1)][:k]
        assert len(p) == k
        return (p + table_c).astype(F)
    table, floor = in_hull_not_chair(40), in_hull_not_chair(50)
    chair = (chair_c + rng.uniform(-0.2, 0.2, (30, 3))).astype(F)
    away = (table_c + np.array([5.0, 0, 0]) + rng.uniform(-0.5, 0.5, (20, 3))).astype(F)
    cloud = np.concatenate([table, chair, floor, away])[None]
    point_box = np.concatenate([np.zeros(40), np.ones(30), -np.ones(70)]).astype(np.int32)[None]
    n = cloud.shape[1]
    is_table, is_chair, is_floor = (np.arange(n) < 40), (np.arange(n) >= 40) & (np.arange(n) < 70), (np.arange(n) >= 70) & (np.arange(n) < 120)
    ident = np.arange(n, dtype=np.int32)[None]
    votes = cloud + rng.normal(0, 0.05, cloud.shape).astype(F)
    votes[0, 40:55] = table_c + rng.normal(0, 0.05, (15, 3)).astype(F)  # half of the chair's votes sit at the TABLE's centre
    want_i = R.loss(ident, ident, point_box, votes, gt_np["bboxes_xyz"])
    want_p = VR.loss(cloud, votes, gt_np)
    gt = {k: T(v, dev) for k, v in gt_np.items()}
    gt["point_box"] = T(point_box, dev)
    out = dict(seeds_xyz=T(cloud, dev), votes_xyz=T(votes, dev))
    l0 = fake_losses(11)
    la, lb = T(l0, dev), T(l0, dev)
    dv_p, sup = VS.paper_vote_loss(out, gt, la)
    dv_i, counts = IV.instance_vote_loss(out, gt, lb, (T(ident, dev), T(ident, dev)))
    dp, di = dv_p.cpu().numpy(), dv_i.cpu().numpy()
    assert np.array_equal(dp.view(np.int32), want_p["d_votes"].view(np.int32)) and int(sup) == want_p["P"] == 120
    assert np.array_equal(di.view(np.int32), want_i["d_votes"].view(np.int32)) and counts.tolist() == [want_i["P"], 0] and want_i["P"] == 70
    assert close(lb[1], want_i["L"]) and close(la[1], want_p["L"]) and float(la[1]) != float(lb[1])
    # the in-box rule: chair points are ambiguous, floor points are supervised
    assert (want_p["count"][0][is_chair] == 2).all() and (want_p["count"][0][is_floor] == 1).all() and (want_p["count"][0][is_table] == 1).all()
    assert (want_p["pick"][0, 40:55] == 0).all() and (want_p["pick"][0, 55:70] == 1).all()  # charged the nearer centre: the table's for half
    assert (np.abs(dp[0][is_floor]).sum(1) > 0).all()                                  # pulled towards the table
    # the instance rule: the floor gets +0.0f, every chair point goes to the chair's centre, the table's points to the table's
    assert not di[0][is_floor].view(np.int32).any() and not di[0, 120:].view(np.int32).any()
    inv = want_i["inv"]
    assert np.array_equal(di[0][is_chair], np.sign(votes[0][is_chair] - chair_c) * inv)
    assert np.array_equal(di[0][is_table], np.sign(votes[0][is_table] - table_c) * inv)
    assert (np.sign(di[0, 40:55]) != np.sign(dp[0, 40:55])).any()                       # towards another centre than the in-box rule's


# ------------------------------------------------------------------ the model
def _label_batch(dev, seed, **kw):
    """B synthetic rooms with their labels through build_batch_from_labels: every point kept, in order, no augmentation."""
    from votenet_amd import input_pipeline as IP
    from votenet_amd import synth
    scenes, inst, sem = [], [], []
    for i in range(B):
        pts = synth.room_scene(NPTS, seed + i)[0]
        scenes.append(np.stack([pts[:, 0], pts[:, 2], -pts[:, 1]], 1))  # upright-depth rows of the camera-frame room
        a, c = synth.room_scene_labels(NPTS, seed + i)
        inst.append(a), sem.append(c)
    raw, off = IP.pack_ragged(scenes, dev)
    choice = np.tile(np.arange(NPTS, dtype=np.int32), (B, 1))
    points, gt, index = IP.build_batch_from_labels(raw, off, np.concatenate(inst), np.concatenate(sem), np.arange(10, dtype=np.int32), choice,
                                                   n_out=NPTS, **kw)
    assert index.tolist() == list(range(B))
    return points, gt, np.stack(inst)


_batches = {}


def batch(dev, seed):
    if seed not in _batches:
        _batches[seed] = _label_batch(dev, seed, point_box=True)
    return _batches[seed]


def _net(dev, seed):
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL)
    net.init_optimizer(1e-3)
    return net


def test_build_batch_from_labels_returns_the_box_row_of_every_point(hiplib, dev):
    from votenet_amd import input_pipeline as IP
    x, gt, inst = batch(dev, 600)
    x0, gt0, _ = _label_batch(dev, 600)
    assert "point_box" not in gt0 and sorted(gt0) == sorted(k for k, _, _ in IP.GT_FIELDS) and sorted(gt) == sorted(list(gt0) + ["point_box"])
    assert torch.equal(bits(x), bits(x0)) and all(torch.equal(gt[k], gt0[k]) for k in gt0)
    pb = gt["point_box"]
    assert pb.dtype == torch.int32 and tuple(pb.shape) == (B, NPTS) and pb.is_contiguous() and pb.device == x.device
    pb = pb.cpu().numpy()
    assert ((pb >= 0) == (inst >= 0)).all() and pb.max() < gt["bboxes_xyz"].shape[1]
    lo = gt["bboxes_xyz"] - 0.5 * gt["bboxes_lwh"]  # (instance_boxes: size = hi - lo per axis, in the axes' order)
    hi = gt["bboxes_xyz"] + 0.5 * gt["bboxes_lwh"]
    for s in range(B):
        own = torch.from_numpy(np.maximum(pb[s], 0)).long().to(dev)
        inside = ((x[s] >= lo[s][own] - 1e-5) & (x[s] <= hi[s][own] + 1e-5)).all(1).cpu().numpy()
        assert inside[pb[s] >= 0].all()  # every labelled point lies in the box its row names (the hull of its instance)
        ids = [np.unique(inst[s][pb[s] == r]) for r in range(pb[s].max() + 1)]
        assert all(len(u) == 1 for u in ids) and len({int(u[0]) for u in ids}) == len(ids)  # a row is one instance


def test_the_seeds_are_the_cloud_points_the_tape_names(hiplib, dev):
    """The invariant the feature rests on: out["seeds_xyz"][s][j] has the bits of x[s][seed_points(sa1's fps_idx, sa2's fps_idx)[s][j]]."""
    from votenet_amd import instance_votes as IV
    x, gt, _ = batch(dev, 600)
    net = _net(dev, 3)
    tape = []
    out = net.forward(x, tape)
    idx1, idx2 = tape[0]["fps_idx"], tape[1]["fps_idx"]
    assert tuple(idx1.shape) == (B, SMALL[0]) and tuple(idx2.shape) == (B, SMALL[1]) and idx1.dtype == idx2.dtype == torch.int32
    sp = IV.seed_points(idx1, idx2, NPTS)
    assert int(sp.min()) >= 0 and int(sp.max()) < NPTS
    picked = torch.gather(x, 1, sp.long()[..., None].expand(B, SMALL[1], 3))
    assert torch.equal(bits(out["seeds_xyz"]), bits(picked))
    assert np.array_equal(sp.cpu().numpy(), R.seed_points(idx1.cpu().numpy(), idx2.cpu().numpy(), NPTS))


def _by_hand(net, record):
    """Make `net` a network whose vote term is replaced BY HAND: its _after_loss calls instance_vote_loss on the fps_idx of the tape's
    own first two records (caught where the tape is made), nothing of enable_instance_votes is involved."""
    from votenet_amd import instance_votes as IV
    inner_forward, inner_levels = net.forward, net.backbone_levels

    def forward(x, tape=None, **kw):
        out = inner_forward(x, tape, **kw)
        if tape:
            record["levels"] = (tape[0]["fps_idx"], tape[1]["fps_idx"])
        return out

    def after_loss(out, gt, losses, cot):
        record["counts"] = IV.instance_vote_loss(out, gt, losses, record["levels"], d_votes=cot["votes_xyz"])[1]
    net.forward, net._after_loss = forward, after_loss
    return net


def test_launch_path_a_step_with_the_mode_on_is_the_step_replaced_by_hand(hiplib, dev):
    """The bit-reproducible mode (mlp.set_deterministic: launch by launch).  Three networks from one seed, two steps on two batches: one
    with the mode on, one whose vote term is replaced by hand, one default.  Mode on and by hand: the same bits in last_losses and in
    every parameter after each update; the default step differs from both in the vote term and agrees in last_losses[2:12] of the
    first step."""
    from votenet_amd import mlp as M
    prev = M.set_deterministic(True)
    try:
        on, off, record = _net(dev, 9), _net(dev, 9), {}
        hand = _by_hand(_net(dev, 9), record)
        on.enable_instance_votes()
        for step, seed in enumerate((600, 602)):
            x, gt, _ = batch(dev, seed)
            for net in (on, hand, off):
                net.train_step(x, gt=gt)
            torch.cuda.synchronize()
            l_on, l_hand, l_off = (n.last_losses.cpu().numpy() for n in (on, hand, off))
            P, Q = on._loss_tail_work[sys.modules["votenet_amd.instance_votes"], B][1].tolist()
            print("step", step, "P", P, "Q", Q, "vote_reg_loss instance", l_on[1], "reference", l_off[1], "total", l_on[0], l_off[0])
            assert np.array_equal(l_on.view(np.int32), l_hand.view(np.int32))
            assert torch.equal(bits(on.store.flat), bits(hand.store.flat)), "a parameter differs after the update of step %d" % step
            assert [P, Q] == record["counts"].tolist() and 0 < P < B * SMALL[1] and Q == 0
            assert l_on[1] != l_off[1] and not torch.equal(bits(on.store.flat), bits(off.store.flat))
            if step == 0:
                assert np.array_equal(l_on[2:].view(np.int32), l_off[2:].view(np.int32))
        assert off.instance_votes is None and not hasattr(off, "_loss_tail_work") and not hasattr(off, "_seed_levels")
    finally:
        M.set_deterministic(prev)


def test_graph_path_with_prefetch_every_step_carries_the_instance_term(hiplib, dev):
    """The default mode (atomics: two networks never agree bit for bit, so what is exact is checked on ONE network): the stretch
    replayed from its captured graphs, the geometry of the next batch prefetched (next_x) into the ring of three geometry graphs, which
    wraps within the eight steps with the mode on.  Every step: the seeds are the cloud points this step's own indices name; the indices
    the launch read (net._seed_levels) still hold this step's values after the step; last_losses is, bit for bit, votenet_loss on the
    step's forward results with its vote term replaced by hand (instance_vote_loss on the tape's own indices, copied where the tape is
    made), and the buffer the first backward segment read holds that cotangent.  Then the mode goes off: the step is the default step
    again (votenet_loss's own bits in last_losses and in the cotangent buffer), and no graph was captured again."""
    from votenet_amd import instance_votes as IV
    from votenet_amd import loss as VL
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH and VM.GEOMETRY_RING == 3
    batches = [batch(dev, s) for s in (600, 602, 604)]
    net = _net(dev, 10)
    mine = {}
    inner = net.backbone_levels

    def levels(x, tape=None, *a, **kw):
        res = inner(x, tape, *a, **kw)
        mine["levels"] = (tape[0]["fps_idx"].clone(), tape[1]["fps_idx"].clone())  # (in stream order: this step's values)
        return res
    net.backbone_levels = levels
    net.enable_instance_votes()
    keys = ("seeds_xyz", "votes_xyz", "proposals_xyz", "proposals_output")
    ngraphs, generations = [], set()
    for i in range(10):
        if i == 8:
            net.disable_instance_votes()
        x, gt, _ = batches[i % 3]
        out = net.train_step(x, gt=gt, next_x=[batches[(i + 1) % 3][0]])
        step_out = {k: out[k].clone() for k in keys}
        got = net.last_losses.clone()
        graphs = net.__dict__.get("_stretch_graphs", {})
        ngraphs.append(len(graphs))
        idx1, idx2 = mine["levels"]
        ref, ref_cot = VL.votenet_loss(step_out, gt)
        if i < 8:
            kept1, kept2, gg, generation = net._seed_levels
            assert torch.equal(kept1, idx1) and torch.equal(kept2, idx2), "step %d: the kept indices are no longer this step's" % i
            if gg is not None:
                generations.add(id(gg))
                assert gg.generation == generation
            sp = IV.seed_points(idx1, idx2, NPTS)
            assert torch.equal(bits(step_out["seeds_xyz"]), bits(torch.gather(x, 1, sp.long()[..., None].expand(B, SMALL[1], 3))))
            hand = ref.clone()
            dv, counts = IV.instance_vote_loss(step_out, gt, hand, (idx1, idx2))
            print("step", i, "P, Q", counts.tolist(), "vote_reg_loss", float(got[1]), "reference", float(ref[1]), "graphs", len(graphs))
            assert torch.equal(bits(got), bits(hand)) and float(got[1]) != float(ref[1]), "step %d" % i
            assert torch.equal(bits(got[2:]), bits(ref[2:]))
            assert net._loss_tail_work[IV, B][1].tolist() == counts.tolist() and int(counts[0]) > 0 and int(counts[1]) == 0
        else:
            dv = ref_cot["votes_xyz"]
            assert torch.equal(bits(got), bits(ref)), "step %d: not the default step" % i
            assert not hasattr(net, "_seed_levels")
        if graphs:
            sg, = graphs.values()
            assert torch.equal(bits(sg.loss_bufs[1][:dv.numel()]), bits(dv).reshape(-1)), "step %d: the cotangent the backward read" % i
    graphs = net.__dict__.get("_stretch_graphs", {})
    assert ngraphs[1:] == [1] * 9 and sum(g.replays for g in graphs.values()) >= 8, "the steps did not go through StretchGraph.replay"
    assert len(generations) == 3, "the prefetched geometry did not go round the ring of three"


def test_a_step_without_point_box_is_refused_before_anything_runs(hiplib, dev):
    from votenet_amd import _lib as L
    x, gt, _ = batch(dev, 600)
    net = _net(dev, 4)
    net.enable_instance_votes()
    before = net.store.flat.clone()
    for bad in ({k: v for k, v in gt.items() if k != "point_box"}, dict(gt, point_box=gt["point_box"][:, :100].contiguous()),
                dict(gt, point_box=gt["point_box"].long()), dict(gt, point_box=gt["point_box"].cpu())):
        with pytest.raises(L.InvalidArgumentError, match="point_box"):
            net.train_step(x, gt=bad)
    assert torch.equal(net.store.flat, before) and net._step == 0
    with pytest.raises(L.InvalidArgumentError, match="disable_instance_votes"):
        net.enable_vote_supervision("paper")
    net.train_step(x, cot=net.make_cotangents(B))  # fixed cotangents: no loss, no launch of the mode, no point_box asked for
    assert not hasattr(net, "_loss_tail_work")


FRESH = """
import sys
sys.path.insert(0, %r)
import numpy as np
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
assert "libvotenet_hip.so" in maps and net.instance_votes is None and not hasattr(net, "_seed_levels")
assert not _lib.side_loaded("instvote") and "libvotenet_instvote" not in maps and "votenet_amd.instance_votes" not in sys.modules
gt["point_box"] = torch.from_numpy(np.stack([synth.room_scene_labels(4096, 7 + i)[0] for i in range(2)])).to(dev)  # (rows of room_gt: the generating boxes)
net.enable_instance_votes()
net.train_step(x, gt=gt)
torch.cuda.synchronize()
assert _lib.side_loaded("instvote") and "libvotenet_instvote.so" in open("/proc/self/maps").read()
assert not _lib.side_loaded("votesup")
P, Q = net._loss_tail_work[sys.modules["votenet_amd.instance_votes"], 2][1].tolist()
assert 0 < P < 2 * 256 and Q == 0, (P, Q)
print("fresh ok")
"""


def test_a_fresh_process_default_train_step_does_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr
