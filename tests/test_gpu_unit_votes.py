"""GPU: unit-length vote features -- votenet_unit_votes / votenet_unit_votes_backward (csrc/unitvote/unit_votes.hip) against the float32
restatement tests/unit_votes_ref.py, every output bit for bit over row counts, channel counts, pitches, widths and the zero /
overflowing / denormal / NaN rows; what the launches leave alone; and VoteNetHotPath.enable_vote_features("unit"): the plain path in
the bit-reproducible mode, the whole backward pass against float64 autograd with the normalisation in its graph, the replayed stretch
graphs, and a fresh process whose default passes never load the library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_votes_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
PATTERN = -7.0
B, SMALL = 2, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_vote_sampling.py)


def bits(t):
    t = t.detach().contiguous().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, F))
    return t.view(torch.int32)


def same(got, want):
    """Equal by bit pattern, NaNs by isnan.  got: a device tensor; want: a numpy float32 array."""
    g, w = got.detach().cpu().contiguous().numpy(), np.ascontiguousarray(want, F)
    if g.shape != w.shape:
        return False
    return bool(((g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w))).all())


def pitched(a, pitch, dev):
    """a (rows, w) numpy -> its device copy as a (rows, w) view at row pitch `pitch` inside a pattern-filled buffer."""
    rows, w = a.shape
    whole = torch.full((rows + 1, pitch), PATTERN, dtype=torch.float32, device=dev)
    whole[:rows, :w] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return whole[:rows, :w]


def out_rows(rows, w, pitch, dev):
    """A pattern-filled (rows, w) output view at row pitch `pitch` with one guard row behind it -> (view, whole buffer)."""
    whole = torch.full((rows + 1, pitch), PATTERN, dtype=torch.float32, device=dev)
    return whole[:rows, :w], whole


def untouched(whole, rows, w):
    """The pitch gap of every row and the guard row behind the last keep their pattern."""
    return bool((whole[:rows, w:] == PATTERN).all() and (whole[rows:] == PATTERN).all())


def run_forward(dev, x, off, c):
    from votenet_amd import _lib as L
    rows = x.shape[0]
    (vx, wx), (vp, wp), (nr, wn) = out_rows(rows, 3, 3, dev), out_rows(rows, c, c, dev), out_rows(rows, 1, 1, dev)
    rc = L.side_lib("unitvote").votenet_unit_votes(rows, c, L.ptr(x), x.stride(0), L.ptr(off), off.stride(0), L.ptr(vx), L.ptr(vp), L.ptr(nr),
                                                   L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.side_lib("unitvote").votenet_unitvote_last_error()
    assert untouched(wx, rows, 3) and untouched(wp, rows, c) and untouched(wn, rows, 1), "a guard row behind an output lost its pattern"
    return vx, vp, nr.view(rows)


def run_backward(dev, dx, cot, g, y, norm, c, d_width, d_pitch):
    from votenet_amd import _lib as L
    rows = g.shape[0]
    d, whole = out_rows(rows, d_width, d_pitch, dev)
    rc = L.side_lib("unitvote").votenet_unit_votes_backward(rows, c, L.ptr(dx), L.ptr(cot), L.ptr(g), L.ptr(y), L.ptr(norm), L.ptr(d), d_pitch,
                                                            d_width, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.side_lib("unitvote").votenet_unitvote_last_error()
    assert untouched(whole, rows, d_width), "the pitch gap or the guard row of d_votes lost its pattern"
    return d


def both_ways(dev, x, off, c, pitches, widths, seed):
    """Forward at every operand pitch and backward at every (d_width, d_pitch), without and with cot_xyz, twice each: every output is
    the restatement's by bit pattern, and two calls write the same bytes."""
    rows = x.shape[0]
    rng = np.random.default_rng(seed)
    g, dx, cot = (rng.standard_normal((rows, w)).astype(F) for w in (c, 3, 3))
    dx[0, 0] = F(-0.0)  # without a cotangent d_xyz passes through as it is: -0 stays -0
    want_xyz, want_y, want_norm = R.forward(x, off)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for pitch in pitches:
        xd, od = pitched(x, pitch, dev), pitched(off, pitch + (0 if pitch == 3 + c else 5), dev)
        runs = [run_forward(dev, xd, od, c) for _ in range(2)]
        for got, want, name in zip(runs[0], (want_xyz, want_y, want_norm), ("votes_xyz", "votes_points", "norm")):
            assert same(got, want), "%s is not the restatement's at pitch %d" % (name, pitch)
        for a, b2 in zip(*runs):
            assert torch.equal(bits(a), bits(b2)), "two calls write different bytes"
    vy, vn = T(want_y), T(want_norm)
    for d_width, d_pitch in widths:
        for cv in (None, cot):
            want = R.backward(dx, cv, g, want_y, want_norm, d_width)
            runs = [run_backward(dev, T(dx), T(cv) if cv is not None else None, T(g), vy, vn, c, d_width, d_pitch) for _ in range(2)]
            assert same(runs[0], want), "d_votes is not the restatement's at d_width %d, d_pitch %d, cot %s" % (d_width, d_pitch, cv is not None)
            assert torch.equal(bits(runs[0]), bits(runs[1])), "two calls write different bytes"
            assert not bool(runs[0][:, 3 + c:].any())


# ------------------------------------------------------------------ the kernels against the restatement
@pytest.mark.parametrize("c", [64, 256, 512])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
def test_kernels_equal_the_restatement_bit_for_bit(hiplib, dev, rows, c):
    x, off = R.random_rows(rows, c, 1000 * rows + c)
    padded = 288 if c == 256 else 3 + c + 29
    both_ways(dev, x, off, c, pitches=(3 + c, padded), widths=((3 + c, 3 + c), (3 + c, padded), (padded, padded + 7), (3 + c + 93, 3 + c + 100)),
              seed=rows + c)


@pytest.mark.parametrize("c", [64, 256, 512])
def test_zero_overflowing_denormal_and_nan_rows_are_the_restatements(hiplib, dev, c):
    x, off = R.special_rows(c)
    _, y, norm = R.forward(x, off)
    kinds = list(R.SPECIAL)
    assert np.isnan(y[kinds.index("zero")]).all() and np.isposinf(norm[kinds.index("overflow")]) and np.isnan(norm[kinds.index("nan")])
    assert np.isinf(y[kinds.index("denormal")]).any() and np.isfinite(y[[0, -1]]).all()
    both_ways(dev, x, off, c, pitches=(3 + c, 3 + c + 29), widths=((3 + c, 3 + c), (3 + c + 29, 3 + c + 30)), seed=c)


def test_python_entries_write_the_same_bytes_and_refused_shapes_launch_nothing(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import unit_votes as UV
    rows, c = 37, 256
    x, off = R.random_rows(rows, c, 77)
    xd, od = pitched(x, 259, dev), pitched(off, 288, dev)
    vx, vp, norm = UV.unit_votes(xd, od)
    want = R.forward(x, off)
    assert vx.shape == (rows, 3) and vp.shape == (rows, c) and norm.shape == (rows,)
    assert all(same(a, b2) for a, b2 in zip((vx, vp, norm), want))
    g = torch.randn(rows, c, device=dev)
    dx, cot = torch.randn(rows, 3, device=dev), torch.randn(rows, 3, device=dev)
    for cv in (None, cot):
        d, whole = out_rows(rows, 288, 300, dev)
        assert UV.unit_votes_backward(dx.view(1, rows, 3), cv, g.view(1, rows, c), vp, norm, d) is d
        torch.cuda.synchronize()
        assert same(d, R.backward(dx.cpu().numpy(), cv.cpu().numpy() if cv is not None else None, g.cpu().numpy(), want[1], want[2], 288))
        assert untouched(whole, rows, 288)
    # refused: nothing is written
    d, whole = out_rows(rows, 288, 300, dev)
    with pytest.raises(L.InvalidArgumentError, match="multiples of 64 expected, got c = 93"):
        UV.unit_votes(xd[:, :96], od[:, :96])
    with pytest.raises(L.InvalidArgumentError, match="d_width of at least 3 \\+ c = 259 columns expected, got d_width = 200"):
        UV.unit_votes_backward(dx, None, g, vp, norm, d[:, :200])
    torch.cuda.synchronize()
    assert bool((whole == PATTERN).all())
    e = torch.empty((0, 259), device=dev)
    assert [tuple(t.shape) for t in UV.unit_votes(e, e)] == [(0, 3), (0, 256), (0,)]  # no row: ok, nothing is launched


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


def _row_norms(votes_points):
    v = votes_points.detach().double()
    return v.reshape(-1, v.shape[-1]).norm(dim=1)


def test_plain_path_the_unit_step_normalises_the_default_steps_vote_features(hiplib, dev):
    """The bit-reproducible mode (mlp.set_deterministic).  Two networks from one seed, one step on one batch: seeds and votes_xyz
    agree bit for bit, the unit step's votes_points are the restatement applied to the default step's (the same sum u), the proposals
    differ, the losses are finite."""
    from votenet_amd import mlp as M
    x, gt = _batch(dev, 470, 4096)
    prev = M.set_deterministic(True)
    try:
        off, on = (_net(dev, 11, SMALL) for _ in range(2))
        on.enable_vote_features("unit")
        out_off = {k: v.clone() for k, v in off.train_step(x, gt=gt).items() if k in KEYS}
        out_on = {k: v.clone() for k, v in on.train_step(x, gt=gt).items() if k in KEYS}
        torch.cuda.synchronize()
        for k in ("seeds_xyz", "seeds_points", "votes_xyz"):
            assert torch.equal(bits(out_off[k]), bits(out_on[k])), k
        u = out_off["votes_points"].cpu().numpy().reshape(-1, 256)
        y, _ = R.normalise(u)
        assert out_on["votes_points"].shape == out_off["votes_points"].shape
        assert same(out_on["votes_points"].reshape(-1, 256), y), "votes_points is not the restatement of the default step's"
        assert not torch.equal(bits(out_off["proposals_output"]), bits(out_on["proposals_output"]))
        assert np.isfinite(on.last_losses.cpu().numpy()).all() and np.isfinite(off.last_losses.cpu().numpy()).all()
        assert not torch.equal(bits(off.store.grad), bits(on.store.grad)) and bool(torch.isfinite(on.store.grad).all())
    finally:
        M.set_deterministic(prev)
    assert off.vote_features is None and on.vote_features == "unit"


def test_full_backward_vs_autograd_with_the_normalisation_in_the_graph(hiplib, dev):
    """test_gpu_backward.py's whole-pass check -- the default mode against float64 autograd over the device's own indices and active
    sets, at that file's own bars -- with enable_vote_features("unit") and vp / |vp| in the float64 head.  Every gradient in front of
    the votes (voting, fp, sa) reaches its tensor through the projection; without it the voting weights' are off by far more."""
    from test_gpu_backward import perturb, ref_chain, ref_fp, ref_sa, relerr
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    from votenet_amd import pointnet2 as P
    from votenet_amd import synth
    assert P.HALF_GROUPS and P.ASSEMBLE_FIRST and P.NARROW_FIRST and P.POOL_GRAM_BACKWARD and not M.DETERMINISTIC
    x = torch.from_numpy(synth.room_batch(2, 2048, 5)).to(dev)
    net = VM.VoteNetHotPath(dev, seed=2, npoints=SMALL)
    net.enable_vote_features("unit")
    perturb(net, dev)
    cot = {k: v * 100 for k, v in net.make_cotangents(2, seed=0).items()}
    net.store.grad.zero_()
    tape = []
    out = net.forward(x, tape)
    net.backward(tape, cot)
    assert float((_row_norms(out["votes_points"]) - 1).abs().max()) <= 1e-6

    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in net.store.views.items()}
    xd = x.double()
    sa1, sa2, sa3, sa4, fp1, fp2, vote, prop = tape
    assert vote["unit"]["y"].data_ptr() == out["votes_points"].data_ptr() and vote["unit"]["norm"].shape == (2 * 256,)
    l1x, l1p = ref_sa(net.sa1, params, xd, xd, sa1)
    l2x, l2p = ref_sa(net.sa2, params, l1x, l1p, sa2)
    l3x, l3p = ref_sa(net.sa3, params, l2x, l2p, sa3)
    l4x, l4p = ref_sa(net.sa4, params, l3x, l3p, sa4)
    l3p2 = ref_fp(net.fp1, params, l3p, l4p, fp1)
    seeds = ref_fp(net.fp2, params, l2p, l3p2, fp2)
    xx = torch.cat([l2x, seeds], 2).view(-1, 259)
    votes = (xx + ref_chain(xx, net.voting, params, vote["recs"])).view(2, -1, 259)
    vx, vp = votes[..., :3], votes[..., 3:]
    vp = vp / vp.norm(dim=-1, keepdim=True)
    _, pout = ref_sa(net.proposal, params, vx, vp, prop)
    err_out = relerr(out["proposals_output"].double(), pout.detach())
    print("proposals_output vs float64: %.3g (bar 5e-5); votes_points %.3g" % (err_out, relerr(out["votes_points"].double(), vp.detach())))
    assert err_out < 5e-5
    loss = (pout * cot["proposals_output"].double()).sum() + (vx * cot["votes_xyz"].double()).sum()
    loss.backward()
    worst = {}
    for name in net.store.views:
        ref = params[name].grad
        got = net.store.g(name).double()
        if name.endswith("/b") and not (name.endswith("fc2/b") or name.endswith("conv_post_2/b")):
            assert float(got.abs().max()) == 0.0  # bias of a BatchNorm'ed layer: exactly zero here
            continue
        worst[name] = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-8)
    print("WORST", sorted(((round(v, 6), k) for k, v in worst.items()), reverse=True)[:12])
    bad = {k: round(v, 6) for k, v in worst.items() if v > 1e-4}
    assert not bad, bad
    assert np.median(list(worst.values())) < 2e-5
    assert len(worst) > 60 and any(k.startswith("voting") for k in worst)


def test_graph_path_each_mode_keeps_its_own_capture(hiplib, dev):
    """The default mode, the stretch replayed from its captured graphs: six steps with the mode switched on, on, off, on, off, on.
    Every row of votes_points has unit norm when the mode is on and none has when it is off; one or two stretch graphs exist at the
    end and the steps went through their replays; predict follows the mode; a step with the paper's other rules beside it is finite."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    batches = [_batch(dev, s, 4096) for s in (480, 482, 484, 486, 488, 490, 492)]
    net = _net(dev, 12, SMALL)
    for (x, gt), mode_on in zip(batches, (True, True, False, True, False, True)):
        net.enable_vote_features("unit") if mode_on else net.disable_vote_features()
        out = net.train_step(x, gt=gt)
        off_one = (_row_norms(out["votes_points"]) - 1).abs()
        losses = net.last_losses.cpu().numpy()
        assert np.isfinite(losses).all(), losses
        if mode_on:
            assert float(off_one.max()) <= 1e-6, float(off_one.max())
        else:
            assert float(off_one.min()) > 1e-6, float(off_one.min())
    graphs = net.__dict__.get("_stretch_graphs", {})
    print("stretch graphs", len(graphs), "replays", [g.replays for g in graphs.values()])
    assert 1 <= len(graphs) <= 2 and sum(g.replays for g in graphs.values()) >= 3, "the steps did not go through StretchGraph.replay"
    x = batches[0][0]
    pred = net.predict(x)  # the mode is on
    assert float((_row_norms(pred["votes_points"]) - 1).abs().max()) <= 1e-6
    net.disable_vote_features()
    pred = net.predict(x)
    assert float((_row_norms(pred["votes_points"]) - 1).abs().min()) > 1e-6
    # the paper's rule in full: votes sampled by FPS, paper vote supervision, paper objectness and centre, unit vote features
    net.enable_vote_features("unit")
    net.enable_proposal_sampling("vote_fps")
    net.enable_vote_supervision("paper")
    net.enable_proposal_supervision("paper")
    x, gt = batches[6]
    out = net.train_step(x, gt=gt)
    assert np.isfinite(net.last_losses.cpu().numpy()).all() and float((_row_norms(out["votes_points"]) - 1).abs().max()) <= 1e-6
    assert bool(torch.isfinite(net.store.grad).all())


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
assert "libvotenet_hip.so" in maps and net.vote_features is None
assert not _lib.side_loaded("unitvote") and "libvotenet_unitvote" not in maps and "votenet_amd.unit_votes" not in sys.modules
before = {name for name in _lib.SIDE_LIBS if _lib.side_loaded(name)}
net.enable_vote_features("unit")
net.train_step(x, gt=gt)
torch.cuda.synchronize()
assert _lib.side_loaded("unitvote") and "libvotenet_unitvote.so" in open("/proc/self/maps").read()
assert {name for name in _lib.SIDE_LIBS if _lib.side_loaded(name)} == before | {"unitvote"}
print("fresh ok")
"""


def test_a_fresh_process_default_passes_do_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr
