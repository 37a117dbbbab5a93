"""GPU: the training summaries on the device -- votenet_accuracies and votenet_tensor_stats (csrc/monitors/monitors.hip) against
the float64 restatement tests/monitors_ref.py, and VoteNetHotPath.enable_monitors: a monitored step trains exactly as an unmonitored
one, read() reports the step that ran, and an unmonitored step never reaches the new entries."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402
import monitors_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_checkpoint.py)


def _pad_boxes(gt, bb):
    """Ragged scenes padded to bb boxes by repeating one (run.py:14-24)."""
    return {k: np.concatenate([v, np.repeat(v[:, :1], bb - v.shape[1], axis=1)], axis=1) for k, v in gt.items()}


# The random cases, fixed after computing monitors_ref on them on the CPU.  Every case has positives and negatives, and right AND wrong
# answers of both kinds (an all-correct kernel gives obj = n_pos + n_neg, sem = n_pos); the smallest distance of a min_dist from a
# threshold is 1.6e-4 and the smallest gap between a nearest and a second nearest distinct box 4.1e-4, a thousand times fp32's error
# on distances of this size.  name -> (seed, random_case arguments, boxes after padding, pitch of proposals_output, expected counts
# n_obj_correct, n_sem_correct, n_pos, n_neg) -- the expected counts are the provenance record of that CPU run; the test compares
# against monitors_ref computed afresh.
RANDOM_CASES = {
    "seed0": (0, {}, 0, 79, (60, 3, 58, 64)),
    "seed1": (1, {}, 0, 79, (57, 4, 64, 55)),
    "one_box": (3, dict(b=1, n=100, p=33, bb=1), 0, 79, (22, 0, 16, 16)),
    "p300_two_rounds": (4, dict(b=3, n=64, p=300, bb=16), 0, 79, (410, 41, 459, 357)),
    "real_shape_seed11": (11, dict(b=8, n=1024, p=256, bb=9), 64, 128, (949, 87, 1018, 902)),
    "real_shape_seed12": (12, dict(b=8, n=1024, p=256, bb=9), 64, 128, (932, 107, 1045, 858)),
}


def _device_case(dev, seeds, votes, prop, out, gt, pitch=79):
    from votenet_amd import loss as VL
    pout = torch.from_numpy(out).to(dev)
    if pitch != out.shape[2]:  # the first 79 columns of a wider row-major tensor, as the proposal module's last GEMM leaves them
        wide = torch.full((out.shape[0], out.shape[1], pitch), 1e30, device=dev)
        wide[:, :, :out.shape[2]] = pout
        pout = wide[:, :, :out.shape[2]]
        assert not pout.is_contiguous()
    o = dict(seeds_xyz=torch.from_numpy(seeds).to(dev), votes_xyz=torch.from_numpy(votes).to(dev),
             proposals_xyz=torch.from_numpy(prop).to(dev), proposals_output=pout)
    return o, VL.gt_to_device(gt, dev)


def _check_against_reference(acc, counts, want):
    from votenet_amd import loss as VL
    c = dict(zip(VL.ACCURACY_COUNTS, counts.cpu().tolist()))
    a = acc.cpu().numpy()
    print("device", c, a.tolist(), "reference", want)
    for k in VL.ACCURACY_COUNTS:
        assert c[k] == want[k], (k, c[k], want[k])
    for got, k in zip(a, ("obj_accuracy", "sem_accuracy")):
        ref = np.float32(want[k])  # a ratio of two integers below 2^24: the fp32 quotient is the rounded float64 quotient
        assert got == ref or (np.isnan(got) and np.isnan(ref)), (k, got, ref)


@pytest.mark.parametrize("name", sorted(RANDOM_CASES))
def test_accuracies_equal_the_reference_on_random_cases(hiplib, dev, name):
    from votenet_amd import loss as VL
    seed, shape, bb, pitch, recorded = RANDOM_CASES[name]
    seeds, votes, prop, out, gt = loss_ref.random_case(seed, **shape)
    if bb:
        gt = _pad_boxes(gt, bb)
    want = R.accuracies(prop, out, gt)
    assert (want["n_obj_correct"], want["n_sem_correct"], want["n_pos"], want["n_neg"]) == recorded
    assert 0 < want["n_sem_correct"] < want["n_pos"] or name == "one_box"
    assert want["n_pos"] > 0 and want["n_neg"] > 0 and 0 < want["n_obj_correct"] < want["n_pos"] + want["n_neg"]
    o, g = _device_case(dev, seeds, votes, prop, out, gt, pitch)
    losses, _ = VL.votenet_loss(o, g)
    ring = torch.full((5, VL.RING_COLS), -7.0, device=dev)
    bufs = (torch.empty(2, device=dev), torch.empty(4, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev))
    for row in (3, 1):  # twice over the same buffers: the launch leaves its workspace zero for the next one
        acc, counts = VL.votenet_accuracies(o, g, losses=losses, ring=ring, ring_row=row, buffers=bufs)
        _check_against_reference(acc, counts, want)
        assert not bufs[2].any()
    # n_pos / n_neg are votenet_loss's on the same inputs, and the ring rows hold the step: total_cost bit for bit
    l = losses.cpu().numpy()
    assert counts.cpu().tolist()[2:] == [int(l[10]), int(l[11])]
    r = ring.cpu().numpy()
    for row in (3, 1):
        assert r[row].tolist() == [acc.cpu().numpy()[0], acc.cpu().numpy()[1], l[0], l[10], l[11]]
    assert (r[[0, 2, 4]] == -7.0).all()
    # for a caller of the operator layer: fresh buffers, no ring, no losses
    acc2, counts2 = VL.votenet_accuracies(o, g)
    assert torch.equal(acc2, acc) and torch.equal(counts2, counts)


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_accuracies_on_hand_made_cases(hiplib, dev, name):
    """A tie is correct, a NaN / infinite target logit is wrong, no positive gives a NaN sem_accuracy beside a finite obj_accuracy."""
    from votenet_amd import loss as VL
    prop, out, gt, want = R.HAND_CASES[name]()
    ref = R.accuracies(prop, out, gt)
    assert {k: ref[k] for k in VL.ACCURACY_COUNTS} == {k: want[k] for k in VL.ACCURACY_COUNTS}
    seeds = np.zeros((prop.shape[0], 8, 3), np.float32)
    o, g = _device_case(dev, seeds, seeds, prop, out, gt)
    acc, counts = VL.votenet_accuracies(o, g)
    _check_against_reference(acc, counts, want)
    a = acc.cpu().numpy()
    if name == "no_positive":
        assert np.isnan(a[1]) and np.isfinite(a[0])
    losses, _ = VL.votenet_loss(o, g)
    assert counts.cpu().tolist()[2:] == [int(v) for v in losses.cpu().numpy()[10:12]]


# ---- tensor summaries -----------------------------------------------------------------------------------------------------------

def _ragged_bucket():
    """Segments of 1, 3, 64, 259 and 65 537 elements behind each other (so most of them start off a 16-byte boundary), gradient-like
    magnitudes, and in them zeros, subnormals, both infinities and a NaN."""
    rng = np.random.default_rng(42)
    lens = [1, 3, 64, 259, 65537]
    ends = np.cumsum(lens)
    segs = [(int(e - n), int(e)) for n, e in zip(lens, ends)]
    x = (rng.standard_normal(ends[-1]) * np.exp(rng.uniform(-12, 3, ends[-1]))).astype(np.float32)
    x[0] = 1e-41                                   # the one-element tensor IS a subnormal: its minimum and maximum must be it
    x[2] = 0.0
    a = segs[2][0]
    x[a + 5], x[a + 6], x[a + 7] = np.inf, -0.0, -3e-39
    a = segs[3][0]
    x[a + 100], x[a + 258] = -np.inf, 2.0 ** 24
    a = segs[4][0]
    x[a + 1], x[a + 40000], x[a + 65536], x[a + 12345] = np.nan, 1e-45, -2.0 ** -41, 0.0
    return x, segs


@pytest.mark.parametrize("scale,clip", [(1.0, 0.0), (0.125, 0.5)])
def test_tensor_stats_on_a_ragged_bucket(hiplib, dev, scale, clip):
    """Counts, extrema, the non-finite count and the histogram equal numpy exactly; sum and sum of squares against float64 within
    the error bound of an fp32 sum of n terms in ANY order, n * 2^-24 * sum |x| (n - 1 additions), resp. n * 2^-24 * sum x^2 (n - 1
    additions and the rounding of each square), plus n * 2^-149 for results below the normal range (a subnormal's square underflows).
    The kernel forms 16 ordered partials per tensor (one per wave of its workgroup).  Twice: same bits."""
    from votenet_amd import monitors as MON
    x, segs = _ragged_bucket()
    want = R.tensor_stats(x, segs, scale=scale, clip=clip)
    # 8 floats ahead of the bucket's segments: the table's offsets need not start at 0
    flat = torch.from_numpy(np.concatenate([np.full(8, np.nan, np.float32), x])).to(dev)
    seg = torch.tensor([v + 8 for s in segs for v in s], dtype=torch.int64, device=dev)
    stats, hist = MON.tensor_stats(seg, flat, scale, clip)
    stats2, hist2 = MON.tensor_stats(seg, flat, scale, clip)
    assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32)) and torch.equal(hist, hist2)
    s, h = stats.cpu().numpy(), hist.cpu().numpy()
    u = 2.0 ** -24
    for i, w in enumerate(want):
        n = w["numel"] - w["nonfinite"]
        print(i, w["numel"], "device", s[i].tolist(), "nonfinite", h[i, 0], "reference", w["sum"], w["sumsq"], w["min"], w["max"], w["clip_factor"])
        assert h[i, 0] == w["nonfinite"] and (h[i, 1:] == w["hist"]).all() and h[i, 1:].sum() == w["numel"]
        assert s[i, 2] == w["min"] and s[i, 3] == w["max"]
        assert abs(float(s[i, 0]) - w["sum"]) <= n * u * w["abs_sum"] + n * 2.0 ** -149
        assert abs(float(s[i, 1]) - w["sumsq"]) <= n * u * w["sumsq"] + n * 2.0 ** -149
        if math.isnan(w["clip_factor"]):
            assert np.isnan(s[i, 4])
        else:
            assert abs(float(s[i, 4]) - w["clip_factor"]) <= 1e-5 * w["clip_factor"]
    if scale == 1.0:
        assert want[0]["min"] == want[0]["max"] == np.float32(1e-41) and s[0, 2] == np.float32(1e-41)
    assert [w["nonfinite"] for w in want] == [0, 0, 1, 1, 1] and want[4]["hist"][0] >= 2
    t = MON.tensor_table(["t%d" % i for i in range(5)], [b - a for a, b in segs], s, h)
    assert t["t1"]["rms"] == pytest.approx(math.sqrt(want[1]["sumsq"] / 3), rel=1e-6) and t["t2"]["nonfinite"] == 1


# ---- the hooks in the train step ------------------------------------------------------------------------------------------------

def _batches(dev, seeds):
    from votenet_amd import loss as VL
    from votenet_amd import synth
    return [(torch.from_numpy(synth.room_batch(B, NPTS, s)).to(dev), VL.gt_to_device(synth.room_gt(B, NPTS, s), dev), synth.room_gt(B, NPTS, s))
            for s in seeds]


def _net(dev, seed):
    from votenet_amd import model as VM
    return VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def test_monitored_steps_train_bit_identically(hiplib, dev):
    """Two nets from one seed, three steps each in the bit-reproducible mode (mlp.set_deterministic: the mode in which the suite requires
    run-twice identical gradients), one with every monitor on: parameters, Adam moments and the losses of every step are the same bits."""
    from votenet_amd import mlp as M
    batches = _batches(dev, (400, 402, 404))
    prev = M.set_deterministic(True)
    try:
        runs = []
        for on in (False, True):
            net = _net(dev, 5)
            net.init_optimizer(1e-3)
            if on:
                net.enable_monitors(window=2, tensors_every=1)
            losses = []
            for x, gt, _ in batches:
                net.train_step(x, gt=gt)
                losses.append(_bits(net.last_losses))
            torch.cuda.synchronize()
            runs.append((_bits(net.store.flat), _bits(net._m), _bits(net._v), losses, net))
    finally:
        M.set_deterministic(prev)
    off, on = runs
    assert torch.equal(off[0], on[0]), "parameters differ"
    assert torch.equal(off[1], on[1]) and torch.equal(off[2], on[2]), "Adam moments differ"
    for a, b in zip(off[3], on[3]):
        assert torch.equal(a, b)
    assert off[4].monitors is None and off[4].last_accuracies is None
    r = on[4].monitors.read()
    assert r["steps"] == 3 and r["filled"] == 2 and r["tensors_step"] == 3 and r["tensors"] is not None
    assert np.float32(r["last"]["total_cost"]).view(np.int32) == on[3][2][0].numpy()


def test_monitors_through_the_stretch_graph_report_every_step(hiplib, dev):
    """The default mode (atomics: not repeatable even against itself), the stretch replayed from its captured graphs with the accuracy
    launch between two segments: what is exact there.  Every step: n_pos / n_neg of read() are last_losses[10:12], the accuracies are
    monitors_ref's on the proposals_xyz / proposals_output THAT step's forward pass produced, and at the end the ring holds
    last_losses[0] of every step bit for bit."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    batches = _batches(dev, (410, 412, 414, 416))
    net = _net(dev, 6)
    net.init_optimizer(1e-3)
    mon = net.enable_monitors(window=100, tensors_every=0)
    costs = []
    for x, gt, gt_np in batches:
        out = net.train_step(x, gt=gt)
        prop, pout = out["proposals_xyz"].clone(), out["proposals_output"].clone()  # this step's forward outputs, before the next replay
        losses = net.last_losses.cpu().numpy()
        acc = net.last_accuracies.cpu().numpy()
        r = mon.read()
        last = r["last"]
        assert (last["n_pos"], last["n_neg"]) == (int(losses[10]), int(losses[11]))
        want = R.accuracies(prop.cpu().numpy(), pout.cpu().numpy(), gt_np)
        print("step", r["steps"], last, "reference", want, "margin", R.decision_margin(prop.cpu().numpy(), gt_np["bboxes_xyz"]))
        for k in ("n_obj_correct", "n_sem_correct", "n_pos", "n_neg"):
            assert last[k] == want[k], k
        for k, a in (("obj_accuracy", acc[0]), ("sem_accuracy", acc[1])):
            ref = np.float32(want[k])
            assert (np.float32(last[k]) == ref and a == ref) or (np.isnan(ref) and np.isnan(last[k]) and np.isnan(a)), (k, last[k], a, ref)
        assert last["n_pos"] + last["n_neg"] > 0
        costs.append(np.float32(losses[0]))
    graphs = net.__dict__.get("_stretch_graphs", {})
    assert graphs and sum(g.replays for g in graphs.values()) >= 2, "the steps did not go through StretchGraph.replay"
    r = mon.read()
    assert r["steps"] == r["filled"] == 4 and r["tensors"] is None
    ring = mon.ring.cpu().numpy()
    assert (ring[:4, 2].view(np.int32) == np.array(costs, np.float32).view(np.int32)).all()
    assert (ring[4:] == 0).all()
    mean = np.array(costs, np.float64).mean()
    assert r["mean"]["total_cost"] == mean or (np.isnan(mean) and np.isnan(r["mean"]["total_cost"]))


def test_tensor_tables_carry_the_reference_names(hiplib, dev):
    """tensors_every: the table is keyed by the reference's variable names, in the optimizer's order; rms, extrema and the clip factor
    are those of the buckets the optimizer read and wrote."""
    from votenet_amd import monitors as MON
    (x, gt, _), = _batches(dev, (420,))
    net = _net(dev, 7)
    net.init_optimizer(1e-3)
    mon = net.enable_monitors(window=3, tensors_every=2)
    net.train_step(x, gt=gt)
    assert mon.read()["tensors"] is None           # step 1: not a multiple of 2
    net.train_step(x, gt=gt)
    r = mon.read()
    assert r["tensors_step"] == 2
    golden = [l.split()[0] for l in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "votenet_variable_names.txt"))
              if l.strip() and not l.startswith("#")]
    params = [n for n in golden if n.split("/")[-1] in ("W", "b", "gamma", "beta")]
    assert sorted(r["tensors"]) == sorted(params) and list(r["tensors"]) == MON.tensor_names(net)
    seg = net._seg.cpu().numpy().reshape(-1, 2)
    flat, grad = net.store.flat.double().cpu().numpy(), net.store.grad.double().cpu().numpy()
    for (a, b), name in zip(seg, MON.tensor_names(net)):
        t = r["tensors"][name]
        for key, v in (("param", flat[a:b]), ("grad", grad[a:b])):
            assert t[key]["numel"] == b - a and t[key]["nonfinite"] == 0 and t[key]["hist"].sum() == b - a
            assert t[key]["rms"] == pytest.approx(math.sqrt((v * v).mean()), rel=1e-5, abs=1e-30)
            assert t[key]["min"] == v.min() and t[key]["max"] == v.max()
        ss = float((grad[a:b] ** 2).sum())
        assert t["grad"]["clip_factor"] == pytest.approx(0.5 / max(math.sqrt(ss) / (b - a), 0.5), rel=1e-5)
        assert t["param"]["clip_factor"] == 1.0


def test_an_unmonitored_step_never_reaches_the_new_entries(hiplib, dev, monkeypatch):
    from votenet_amd import loss as VL
    from votenet_amd import monitors as MON

    def boom(*a, **k):
        raise AssertionError("a monitor launch in an unmonitored step")
    monkeypatch.setattr(VL, "votenet_accuracies", boom)
    monkeypatch.setattr(MON, "tensor_stats", boom)
    batches = _batches(dev, (430, 432, 434))
    net = _net(dev, 8)
    net.init_optimizer(1e-3)
    for x, gt, _ in batches:        # launch by launch, then captured and replayed
        net.train_step(x, gt=gt)
    torch.cuda.synchronize()
    assert net.monitors is None and net.last_accuracies is None
    net.enable_monitors(window=4, tensors_every=1)
    net.disable_monitors()
    net.train_step(batches[0][0], gt=batches[0][1])
    torch.cuda.synchronize()
    net.enable_monitors(window=4, tensors_every=1)
    with pytest.raises(AssertionError, match="monitor launch"):   # the patch has teeth (the net is not used after this)
        net.train_step(batches[0][0], gt=batches[0][1])
    torch.cuda.synchronize()
