"""GPU: proposals sampled on the votes -- votenet_cluster_votes (csrc/votesamp/vote_sampling.hip) against the float32 restatement
tests/vote_sampling_ref.py and against the composition of the shipped operators on the device (farthest_point_sample, gather_point,
query_ball_point), all four outputs bit for bit over tests/vote_sampling_cases.py; what the launch leaves alone; and
VoteNetHotPath.enable_proposal_sampling: a pass with the mode on is, bit for bit, the pass that is handed the votes' sample through
propose's prop_fps argument, on the plain path and through the replayed graphs; a pass with the mode off never loads the library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_sampling_cases as C  # noqa: E402
import vote_sampling_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
PATTERN = -7
OUTS = ("fps_idx", "new_xyz", "idx", "pts_cnt")
B, SMALL = 2, (512, 256, 128, 64)     # the suite's small training shape (test_gpu_monitors.py): 256 seeds, m == n
WIDE = (1024, 512, 256, 128)          # 512 seeds: n > m = 256


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    t = t.detach().contiguous().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def guarded(shape, dev, dtype):
    """A pattern-filled contiguous tensor of `shape` with GUARD pattern elements before and behind it -> (tensor, whole buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), PATTERN, device=dev).to(dtype)
    return whole[GUARD:GUARD + n].view(shape), whole


def launch(dev, votes, m, radius, k):
    """One launch of the C entry into guarded, pattern-filled buffers -> (status, the four tensors, their whole buffers)."""
    from votenet_amd import _lib as L
    b, n, _ = votes.shape
    outs, wholes = zip(*(guarded(shape, dev, dt) for shape, dt in (((b, m), torch.int32), ((b, m, 3), torch.float32),
                                                                  ((b, m, k), torch.int32), ((b, m), torch.int32))))
    v = votes if isinstance(votes, torch.Tensor) else T(votes, dev)
    rc = L.side_lib("votesamp").votenet_cluster_votes(b, n, m, float(radius), k, L.ptr(v), *[L.ptr(o) for o in outs], L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dict(zip(OUTS, outs)), wholes


def guards_intact(wholes):
    return all(bool((w[:GUARD] == PATTERN).all() and (w[-GUARD:] == PATTERN).all()) for w in wholes)


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_cluster_votes_equals_the_restatement_and_the_shipped_operators(hiplib, dev, case):
    from votenet_amd import tf_grouping, tf_sampling
    from votenet_amd import vote_sampling as VS
    name, votes, m, radius, k, _ = case
    n = votes.shape[1]
    want = C.results(case)
    v = T(votes, dev)
    runs = [launch(dev, v, m, radius, k) for _ in range(2)]
    for rc, got, wholes in runs:
        assert rc == 0 and guards_intact(wholes), "outputs sit between guard words that keep their pattern"
    got = runs[0][1]
    for o in OUTS:
        assert torch.equal(bits(got[o]), bits(runs[1][1][o])), o + ": two runs give the same bytes"
        assert torch.equal(bits(got[o]), bits(want[o])), o + " is not the restatement's"
    assert 0 <= int(got["fps_idx"].min()) and int(got["fps_idx"].max()) < n and 0 <= int(got["idx"].min()) and int(got["idx"].max()) < n
    # the composition of the shipped operators, on the device
    fps = tf_sampling.farthest_point_sample(m, v)
    centres = tf_sampling.gather_point(v, fps)
    idx, cnt = tf_grouping.query_ball_point(radius, k, v, centres)
    for o, t in zip(OUTS, (fps, centres, idx, cnt)):
        assert torch.equal(bits(got[o]), bits(t)), o + " is not the shipped operators'"
    # the Python entry: fresh tensors, the same bytes
    api = VS.cluster_votes(v, m, radius, k)
    for o, t, dt in zip(OUTS, api, (torch.int32, torch.float32, torch.int32, torch.int32)):
        assert t.dtype == dt and tuple(t.shape) == tuple(got[o].shape) and torch.equal(bits(t), bits(got[o])), o


def test_refused_shapes_launch_nothing_and_leave_the_outputs_pattern(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import vote_sampling as VS
    for (n, m, k, radius), text in (((2049, 16, 8, 0.3), "1 to 2048 votes per scene, got n = 2049"),
                                    ((64, 1025, 8, 0.3), "1 to 1024 clusters per scene, got m = 1025"),
                                    ((64, 16, 65, 0.3), "1 to 64 votes per cluster, got nsample = 65"),
                                    ((64, 16, 8, 0.0), "positive radius")):
        votes = torch.zeros((2, n, 3), device=dev)
        rc, got, wholes = launch(dev, votes, m, radius, k)
        assert rc == 1 and text in L.side_lib("votesamp").votenet_votesamp_last_error().decode()
        assert all(bool((w == PATTERN).all()) for w in wholes)
        with pytest.raises(L.InvalidArgumentError, match=text):
            VS.cluster_votes(votes, m, radius, k)
    rc, got, wholes = launch(dev, torch.zeros((0, 64, 3), device=dev), 16, 0.3, 8)  # no scene: ok, nothing is launched
    assert rc == 0 and all(bool((w == PATTERN).all()) for w in wholes)


# ------------------------------------------------------------------ the network
def _batch(dev, seed, npts):
    from votenet_amd import loss as VL
    from votenet_amd import synth
    return torch.from_numpy(synth.room_batch(B, npts, seed)).to(dev), VL.gt_to_device(synth.room_gt(B, npts, seed), dev)


def _net(dev, seed, npoints):
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=seed, npoints=npoints)
    net.init_optimizer(1e-3)
    return net


KEYS = ("seeds_xyz", "seeds_points", "votes_xyz", "votes_points", "proposals_xyz", "proposals_output")


def _sample_of(votes_xyz, m=256):
    from votenet_amd import tf_sampling
    return tf_sampling.gather_point(votes_xyz, tf_sampling.farthest_point_sample(m, votes_xyz))


@pytest.mark.parametrize("npoints,npts", [(WIDE, 8192), (SMALL, 4096)], ids=["512-seeds", "256-seeds-m-equals-n"])
def test_plain_path_a_vote_fps_step_is_the_step_handed_the_votes_sample(hiplib, dev, npoints, npts):
    """The bit-reproducible mode (mlp.set_deterministic).  Three networks from one seed, one step on one batch.  The network with the
    mode on and the one without agree bit for bit up to the votes and differ in the proposals; the vote_fps step's outputs, loss vector
    and whole gradient bucket are those of a hand-assembled pass -- forward, votenet_loss, backward -- on the third network, whose
    propose is handed farthest_point_sample(256, votes_xyz) through its prop_fps argument (the five-launch composition); and the step
    with the mode off is the hand-assembled pass of a network that never heard of the mode."""
    from votenet_amd import loss as VL
    from votenet_amd import mlp as M
    from votenet_amd import tf_sampling
    x, gt = _batch(dev, 470, npts)
    prev = M.set_deterministic(True)
    try:
        off, on, hand = (_net(dev, 11, npoints) for _ in range(3))
        on.enable_proposal_sampling("vote_fps")
        out_off = {k: v.clone() for k, v in off.train_step(x, gt=gt).items() if k in KEYS}
        out_on = {k: v.clone() for k, v in on.train_step(x, gt=gt).items() if k in KEYS}
        torch.cuda.synchronize()
        for k in KEYS[:4]:
            assert torch.equal(bits(out_off[k]), bits(out_on[k])), k
        assert not torch.equal(bits(out_off["proposals_xyz"]), bits(out_on["proposals_xyz"]))
        assert torch.equal(bits(out_on["proposals_xyz"]), bits(_sample_of(out_on["votes_xyz"])))
        assert torch.equal(bits(out_off["proposals_xyz"]),
                           bits(tf_sampling.gather_point(out_off["votes_xyz"], tf_sampling.farthest_point_sample(256, out_off["seeds_xyz"]))))
        assert np.isfinite(on.last_losses.cpu().numpy()).all()
        orig = hand.propose
        for patched, step, out_step in ((False, off, out_off), (True, on, out_on)):
            if patched:  # the control: the composition of the existing entries, through the existing argument
                hand.propose = lambda vx, vp, sx, tape=None, prop_fps=None: orig(vx, vp, sx, tape,
                                                                                 tf_sampling.farthest_point_sample(hand.proposal.npoint, vx))
            hand.store.grad.zero_()
            hand.store.refresh_transposes()
            tape = []
            out_h = hand.forward(x, tape)
            for k in KEYS:
                assert torch.equal(bits(out_h[k]), bits(out_step[k])), (patched, k)
            losses_h, cot_h = VL.votenet_loss(out_h, gt)
            assert torch.equal(bits(losses_h), bits(step.last_losses)), patched
            hand.backward(tape, cot_h)
            torch.cuda.synchronize()
            assert torch.equal(bits(hand.store.grad), bits(step.store.grad)), \
                "the %s step's gradient is not the hand-assembled one" % ("vote_fps" if patched else "default")
        assert not torch.equal(bits(off.store.grad), bits(on.store.grad))
    finally:
        M.set_deterministic(prev)
    assert off.proposal_sampling is None and hand.proposal_sampling is None


def test_graph_path_each_mode_keeps_its_own_capture(hiplib, dev):
    """The default mode, the stretch replayed from its captured graphs: six steps with the mode switched on, on, off, on, off, on.
    Every step's proposals_xyz is the gather of ITS votes at the farthest-point sample of its votes (mode on) or of its seeds (mode
    off), bit for bit; two stretch graphs exist at the end, and the steps went through their replays; predict follows the mode too."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    from votenet_amd import tf_sampling
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    batches = [_batch(dev, s, 4096) for s in (480, 482, 484, 486, 488, 490)]
    net = _net(dev, 12, SMALL)
    for (x, gt), mode_on in zip(batches, (True, True, False, True, False, True)):
        net.enable_proposal_sampling("vote_fps") if mode_on else net.disable_proposal_sampling()
        out = net.train_step(x, gt=gt)
        out = {k: out[k].clone() for k in ("seeds_xyz", "votes_xyz", "proposals_xyz")}
        losses = net.last_losses.cpu().numpy()
        if mode_on:
            assert torch.equal(bits(out["proposals_xyz"]), bits(_sample_of(out["votes_xyz"])))
            assert np.isfinite(losses).all(), losses
        else:
            fps = tf_sampling.farthest_point_sample(256, out["seeds_xyz"])
            assert torch.equal(bits(out["proposals_xyz"]), bits(tf_sampling.gather_point(out["votes_xyz"], fps)))
    graphs = net.__dict__.get("_stretch_graphs", {})
    print("stretch graphs", len(graphs), "replays", [g.replays for g in graphs.values()])
    assert 1 <= len(graphs) <= 2 and sum(g.replays for g in graphs.values()) >= 3, "the steps did not go through StretchGraph.replay"
    x = batches[0][0]
    pred = net.predict(x)  # the mode is on: the boxes' centres derive from the vote-sampled proposals
    assert torch.equal(bits(pred["proposals_xyz"]), bits(_sample_of(pred["votes_xyz"])))
    assert pred["bboxes"].shape[:2] == pred["proposals_xyz"].shape[:2]
    net.disable_proposal_sampling()
    pred = net.predict(x)
    fps = tf_sampling.farthest_point_sample(256, pred["seeds_xyz"])
    assert torch.equal(bits(pred["proposals_xyz"]), bits(tf_sampling.gather_point(pred["votes_xyz"], fps)))


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
net.predict(x)
torch.cuda.synchronize()
maps = open("/proc/self/maps").read()
assert "libvotenet_hip.so" in maps and net.proposal_sampling is None
assert not _lib.side_loaded("votesamp") and "libvotenet_votesamp" not in maps and "votenet_amd.vote_sampling" not in sys.modules
before = {name for name in _lib.SIDE_LIBS if _lib.side_loaded(name)}
net.enable_proposal_sampling("vote_fps")
net.train_step(x, gt=gt)
torch.cuda.synchronize()
assert _lib.side_loaded("votesamp") and "libvotenet_votesamp.so" in open("/proc/self/maps").read()
assert {name for name in _lib.SIDE_LIBS if _lib.side_loaded(name)} == before | {"votesamp"}
print("fresh ok")
"""


def test_a_fresh_process_default_passes_do_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr
