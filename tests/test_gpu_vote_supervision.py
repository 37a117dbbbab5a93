"""GPU: the paper's vote supervision on the device -- votenet_vote_targets and votenet_paper_vote_loss
(csrc/votesup/vote_supervision.hip) against the float32 restatement tests/vote_supervision_ref.py, bit for bit in every decision and
cotangent; the relation to votenet_loss where the two rules must agree; and VoteNetHotPath.enable_vote_supervision: a step with the
mode on changes the vote term, its cotangent and the total and nothing else, on the plain path and through the replayed graphs; a step
with the mode off never loads the library; and the network trains under it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_supervision_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(1, 1, 1), (2, 63, 2), (3, 65, 5), (2, 1000, 7), (2, 1024, 256)]  # one seed; under, over a wave; a ragged tile; the training tile, LOSS_MAXBOX
B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_monitors.py)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    t = t.detach().contiguous().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def close(got, want):
    """the project's tolerance on loss values: 1e-5 relative, floor 1.0 (tests/test_gpu_loss.py)"""
    return abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))


_cases = {}


def case(shape):
    """The inputs of a shape and their restated results, computed once and shared."""
    if shape not in _cases:
        seeds, votes, gt = R.device_case(*shape, seed=11 + shape[1])
        _cases[shape] = (seeds, votes, gt, R.loss(seeds, votes, gt))
    return _cases[shape]


def fake_losses(dev, seed=3):
    """12 floats as votenet_loss leaves them: every component its own value, the total composed from them."""
    l = np.random.default_rng(seed).random(12).astype(F) + F(0.25)
    l[0] = R.total(l, l[1])
    return l, T(l, dev)


# ------------------------------------------------------------------ targets
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d-n%d-bb%d" % s)
def test_targets_equal_the_restatement_bit_for_bit(hiplib, dev, shape):
    from votenet_amd import vote_supervision as VS
    b, n, bb = shape
    seeds, _, gt, want = case(shape)
    slots, count = VS.vote_targets(T(seeds, dev), {k: T(v, dev) for k, v in gt.items()})
    assert slots.dtype == torch.int32 and tuple(slots.shape) == (b, n, 3) and count.dtype == torch.int32 and tuple(count.shape) == (b, n)
    s, c = slots.cpu().numpy(), count.cpu().numpy()
    print(shape, "sets of 0..5+:", np.bincount(np.minimum(want["count"].ravel(), 5), minlength=6).tolist())
    assert np.array_equal(c, want["count"]) and np.array_equal(s, want["slots"])
    assert (s[c == 0] == -1).all() and (s[c > 0] >= 0).all() and s.max() < bb
    # the case holds what it is meant to: a seed ON a face is inside (closed rule), the nest is k boxes deep, non-finite seeds are nowhere
    nest = min(5, bb)
    ins = R.inside(seeds[0], gt["bboxes_xyz"][0], gt["bboxes_lwh"][0], gt["bboxes_roty"][0])
    assert ins[0, :nest].all()                                    # seed 0: ON the +y face of the nest's smallest box
    if n > 2 * nest:                                              # seeds 2 j, 2 j + 1: on the two y faces of nest box j; then the centre
        assert ins[:2 * nest + 1, :nest].sum(1).tolist() == [nest - j // 2 for j in range(2 * nest)] + [nest]
        assert c[0, 2 * nest] >= nest >= min(bb, 5)
    bad = ~np.isfinite(seeds).all(-1)
    assert not c[bad].any() and (bad.sum() >= 4 * b or n < 20)
    if bb >= 8:
        assert (gt["bboxes_lwh"][:, 6] == 0).all() and ins[2 * nest + 1, 6]  # the zero-size box holds its own centre
        assert (c > 5).any() and (s[..., 2] == bb - 1).any()       # the edge-padded copies enter sets; the LAST one is slot 2


# ------------------------------------------------------------------ the loss
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%d-n%d-bb%d" % s)
def test_loss_cotangent_and_total_equal_the_restatement(hiplib, dev, shape):
    from votenet_amd import vote_supervision as VS
    b, n, bb = shape
    seeds, votes, gt, want = case(shape)
    out = dict(seeds_xyz=T(seeds, dev), votes_xyz=T(votes, dev))
    g = {k: T(v, dev) for k, v in gt.items()}
    l0, _ = fake_losses(dev)
    work = VS.workspace(b, dev)
    runs = []
    for _ in range(2):  # twice over one workspace: the launch leaves it zero, and the bytes are the same
        losses = T(l0, dev)
        d_votes = torch.full((b, n, 3), -7.0, device=dev)
        dv, sup = VS.paper_vote_loss(out, g, losses, d_votes=d_votes, work=work)
        assert dv is d_votes and not work.any()
        runs.append((bits(losses), bits(d_votes), int(sup)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    l = losses.cpu().numpy()
    print(shape, "P", runs[0][2], want["P"], "L", l[1], want["L"], "total", l[0], R.total(l0, want["L"]))
    assert runs[0][2] == want["P"] and want["P"] > 0
    assert close(l[1], want["L"]) and close(l[0], R.total(l0, want["L"]))
    assert l[0] == R.total(l0, l[1])                                # the total re-formed from the stored components, in loss.hip's order
    assert np.array_equal(l[2:].view(np.int32), l0[2:].view(np.int32))
    assert torch.equal(runs[0][1], bits(want["d_votes"]))           # sign * inv exactly, +0.0 on every unsupervised seed
    fresh, _ = VS.paper_vote_loss(out, g, T(l0, dev))               # for a caller of the operator layer: fresh buffers
    assert torch.equal(bits(fresh), runs[0][1])


def test_no_supervised_seed_gives_zeros(hiplib, dev):
    from votenet_amd import vote_supervision as VS
    seeds, votes, gt, _ = case((3, 65, 5))
    far = seeds + F(100.0)
    far[~np.isfinite(far)] = 100.0
    l0, losses = fake_losses(dev)
    dv, sup = VS.paper_vote_loss(dict(seeds_xyz=T(far, dev), votes_xyz=T(votes, dev)), {k: T(v, dev) for k, v in gt.items()}, losses)
    l = losses.cpu().numpy()
    assert int(sup) == 0 and l[1] == 0.0 and l[0] == R.total(l0, 0.0)
    assert not bits(dv).any()                                       # +0.0 everywhere


def test_a_nan_vote_at_a_supervised_seed(hiplib, dev):
    """L is NaN (the seed's distance is), so is the total; the cotangent stays finite everywhere: 0 in the NaN component (sgn(NaN) = 0),
    the restated values elsewhere."""
    from votenet_amd import vote_supervision as VS
    seeds, votes, gt, base = case((2, 63, 2))
    i = int(np.nonzero(base["count"][1])[0][3])
    votes = votes.copy()
    votes[1, i, 1] = np.nan
    want = R.loss(seeds, votes, gt)
    l0, losses = fake_losses(dev)
    dv, sup = VS.paper_vote_loss(dict(seeds_xyz=T(seeds, dev), votes_xyz=T(votes, dev)), {k: T(v, dev) for k, v in gt.items()}, losses)
    l, d = losses.cpu().numpy(), dv.cpu().numpy()
    assert int(sup) == want["P"] == base["P"] and np.isnan(l[1]) and np.isnan(l[0]) and np.isnan(want["L"])
    assert np.isfinite(d).all() and d[1, i, 1] == 0.0 and d[1, i, 0] != 0.0
    assert torch.equal(bits(dv), bits(want["d_votes"]))
    assert np.array_equal(l[2:].view(np.int32), l0[2:].view(np.int32))


def test_more_than_256_boxes_are_refused_and_nothing_is_launched(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import vote_supervision as VS
    seeds, votes, gt = R.device_case(1, 16, 257, seed=5)
    out, g = dict(seeds_xyz=T(seeds, dev), votes_xyz=T(votes, dev)), {k: T(v, dev) for k, v in gt.items()}
    l0, losses = fake_losses(dev)
    d_votes = torch.full((1, 16, 3), -7.0, device=dev)
    with pytest.raises(L.InvalidArgumentError, match="1 to 256 boxes per scene, got bb = 257"):
        VS.paper_vote_loss(out, g, losses, d_votes=d_votes)
    with pytest.raises(L.InvalidArgumentError, match="1 to 256 boxes per scene, got bb = 257"):
        VS.vote_targets(out["seeds_xyz"], g)
    torch.cuda.synchronize()
    assert (d_votes == -7.0).all() and torch.equal(bits(losses), bits(l0))


# ------------------------------------------------------------------ cubes: the relation to votenet_loss on the device
def test_on_far_apart_cubes_the_sum_is_votenet_loss_s_sum(hiplib, dev):
    from votenet_amd import loss as VL
    from votenet_amd import vote_supervision as VS
    seeds, votes, prop, pout, gt = R.cube_case(7)
    b, n = seeds.shape[:2]
    out = dict(seeds_xyz=T(seeds, dev), votes_xyz=T(votes, dev), proposals_xyz=T(prop, dev), proposals_output=T(pout, dev))
    g = VL.gt_to_device(gt, dev)
    losses, cot = VL.votenet_loss(out, g)
    ref = losses.cpu().numpy().copy()
    ref_cot = cot["votes_xyz"].clone()
    _, sup = VS.paper_vote_loss(out, g, losses, d_votes=cot["votes_xyz"])
    l, P = losses.cpu().numpy(), int(sup)
    lhs, rhs = float(l[1]) * (P + 1e-6), float(ref[1]) * b * n
    print("P", P, "L (P + 1e-6)", lhs, "votenet_loss vote_reg_loss B n", rhs, "totals", ref[0], l[0])
    assert 0.05 * b * n < P < 0.5 * b * n and np.isfinite(ref).all()
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(rhs))
    assert np.array_equal(l[2:].view(np.int32), ref[2:].view(np.int32)) and l[0] == R.total(ref, l[1])
    # the same seeds are supervised, towards the same centres: the cotangents differ in the divisor alone
    a, c = ref_cot.cpu().numpy().astype(np.float64) * (b * n), cot["votes_xyz"].cpu().numpy().astype(np.float64) * (P + 1e-6)
    assert np.abs(a - c).max() <= 1e-5


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


def _recomputed(out, gt, losses):
    """votenet_loss and paper_vote_loss again on a step's own forward results -> (the reference's 12 floats, the paper's, its cotangent,
    P), as numpy / device tensors."""
    from votenet_amd import loss as VL
    from votenet_amd import vote_supervision as VS
    ref, _ = VL.votenet_loss(out, gt)
    paper = ref.clone()
    dv, sup = VS.paper_vote_loss(out, gt, paper)
    return ref.cpu().numpy(), paper.cpu().numpy(), dv, int(sup)


def test_plain_path_a_paper_step_changes_the_vote_term_and_nothing_else(hiplib, dev):
    """The bit-reproducible mode (mlp.set_deterministic: launch by launch, the mode in which the suite requires run-twice identical
    gradients).  Two networks from one seed, one step on one batch, one with the mode on (and the monitors, whose ring must record the
    re-formed total): the forward results and last_losses[2:12] are the same bits; last_losses[0:2] of the paper step are
    paper_vote_loss's on its own forward results; and its gradient bucket is, bit for bit, the bucket of a hand-assembled pass on a third
    network -- forward, votenet_loss, its votes_xyz cotangent replaced by the RESTATED one (numpy), backward."""
    from votenet_amd import loss as VL
    from votenet_amd import mlp as M
    x, gt, gt_np = _batch(dev, 440)
    keys = ("seeds_xyz", "votes_xyz", "proposals_xyz", "proposals_output", "seeds_points", "votes_points")
    prev = M.set_deterministic(True)
    try:
        off, on, hand = _net(dev, 9), _net(dev, 9), _net(dev, 9)
        on.enable_vote_supervision("paper")
        mon = on.enable_monitors(window=4)
        out_off = {k: v.clone() for k, v in off.train_step(x, gt=gt).items() if k in keys}
        out_on = {k: v.clone() for k, v in on.train_step(x, gt=gt).items() if k in keys}
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(bits(out_off[k]), bits(out_on[k])), k
        l_off, l_on = off.last_losses.cpu().numpy(), on.last_losses.cpu().numpy()
        assert np.array_equal(l_off[2:].view(np.int32), l_on[2:].view(np.int32))
        ref, paper, dv, P = _recomputed(out_on, gt, on.last_losses)
        assert np.array_equal(ref.view(np.int32), l_off.view(np.int32)) and np.array_equal(paper.view(np.int32), l_on.view(np.int32))
        want = R.loss(out_on["seeds_xyz"].cpu().numpy(), out_on["votes_xyz"].cpu().numpy(), gt_np)
        print("P", P, want["P"], "vote_reg_loss reference", l_off[1], "paper", l_on[1], want["L"], "total", l_off[0], l_on[0])
        assert P == want["P"] and 0 < P < B * SMALL[1] and close(l_on[1], want["L"]) and l_on[0] == R.total(l_on, l_on[1])
        assert l_on[1] != l_off[1] and torch.equal(bits(dv), bits(want["d_votes"]))
        assert np.float32(mon.read()["last"]["total_cost"]).view(np.int32) == l_on[:1].view(np.int32)[0]
        # the hand-assembled pass: first with votenet_loss's own cotangents (the control: it must be the reference step's bucket)
        for restated, step in ((None, off), (want["d_votes"], on)):
            hand.store.grad.zero_()
            hand.store.refresh_transposes()
            tape = []
            out_h = hand.forward(x, tape)
            assert torch.equal(bits(out_h["votes_xyz"]), bits(out_on["votes_xyz"]))
            _, cot = VL.votenet_loss(out_h, gt)
            if restated is not None:
                cot = dict(cot, votes_xyz=T(restated, dev))
            hand.backward(tape, cot)
            torch.cuda.synchronize()
            assert torch.equal(bits(hand.store.grad), bits(step.store.grad)), \
                "the %s step's gradient is not the hand-assembled one" % ("reference" if restated is None else "paper")
        assert not torch.equal(bits(off.store.grad), bits(on.store.grad))
    finally:
        M.set_deterministic(prev)
    assert off.vote_supervision is None and not hasattr(off, "_loss_tail_work")


def test_graph_path_every_replayed_step_carries_the_paper_term(hiplib, dev):
    """The default mode (atomics: not repeatable even against itself, so no second network to compare bits with), the stretch replayed
    from its captured graphs with the launch between two segments: what is exact there.  Every step: last_losses[2:12] are votenet_loss's
    on THAT step's forward results bit for bit, last_losses[0:2] are paper_vote_loss's on them, the buffer the next segment read holds the
    paper's cotangent, and the monitors' ring holds the re-formed total.  Switching the mode captures no graph again."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    batches = [_batch(dev, s) for s in (450, 452, 454, 456, 458)]
    net = _net(dev, 10)
    mon = net.enable_monitors(window=16)
    modes = ["paper", "paper", "paper", None, "paper"]      # launch by launch, captured, replayed, off, on again
    ngraphs = []
    for (x, gt, gt_np), mode in zip(batches, modes):
        if mode:
            net.enable_vote_supervision(mode)
        else:
            net.disable_vote_supervision()
        out = net.train_step(x, gt=gt)
        step_out = {k: out[k].clone() for k in ("seeds_xyz", "votes_xyz", "proposals_xyz", "proposals_output")}
        got = net.last_losses.cpu().numpy()
        graphs = net.__dict__.get("_stretch_graphs", {})
        ngraphs.append(len(graphs))
        ref, paper, dv, P = _recomputed(step_out, gt, net.last_losses)
        want = paper if mode else ref
        print("mode", mode, "P", P, "vote_reg_loss", got[1], "reference", ref[1], "paper", paper[1], "total", got[0])
        assert np.array_equal(got.view(np.int32), want.view(np.int32)) and (mode is None or got[1] != ref[1])
        assert np.float32(mon.read()["last"]["total_cost"]).view(np.int32) == got[:1].view(np.int32)[0]
        if graphs and mode:  # the cotangent the first backward segment read
            sg, = graphs.values()
            assert torch.equal(bits(sg.loss_bufs[1][:dv.numel()]), bits(dv).reshape(-1))
            r = R.loss(step_out["seeds_xyz"].cpu().numpy(), step_out["votes_xyz"].cpu().numpy(), gt_np)
            assert P == r["P"] and torch.equal(bits(dv), bits(r["d_votes"]))
    graphs = net.__dict__.get("_stretch_graphs", {})
    assert ngraphs[1:] == [1, 1, 1, 1] and sum(g.replays for g in graphs.values()) >= 3, "the steps did not go through StretchGraph.replay"


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
assert "libvotenet_hip.so" in maps and net.vote_supervision is None
assert not _lib.side_loaded("votesup") and "libvotenet_votesup" not in maps and "votenet_amd.vote_supervision" not in sys.modules
net.enable_vote_supervision("paper")
net.train_step(x, gt=gt)
torch.cuda.synchronize()
assert _lib.side_loaded("votesup") and "libvotenet_votesup.so" in open("/proc/self/maps").read()
print("fresh ok")
"""


def test_a_fresh_process_default_train_step_does_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr


def test_it_trains(hiplib, dev):
    """150 steps on synthetic rooms with the mode on: the mean vote_reg_loss of the last 20 steps is below that of the first 20."""
    net = _net(dev, 11)
    net.enable_vote_supervision("paper")
    batches = [_batch(dev, 460 + 2 * i) for i in range(6)]
    votes = []
    for i in range(150):
        x, gt, _ = batches[i % len(batches)]
        net.train_step(x, gt=gt, next_x=batches[(i + 1) % len(batches)][0])
        votes.append(net.last_losses[1:2].clone())
    v = torch.cat(votes).cpu().numpy()
    first, last = float(v[:20].mean()), float(v[-20:].mean())
    print("vote_reg_loss: first 20 steps %.4f, last 20 steps %.4f" % (first, last))
    assert np.isfinite(v).all() and last < first, (first, last)
