"""GPU: the guarded optimizer step (csrc/guard/step_guard.hip, votenet_amd/step_guard.py).  At the ABI on the synthetic bucket of
tests/step_guard_cases.py: a good step is votenet_clip_adam bit for bit, a bad one writes nothing and is counted, the moving averages
follow the snapshot rule.  In the model: guarded steps train bit-identically, a poisoned step leaves the four buffers as they were,
checkpoints refresh the snapshot, and an unguarded step never reaches the entry."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_guard_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)  # the suite's small training shape (test_gpu_monitors.py)
N_EMA = 25003                                  # the model's moving averages are ~25 k floats; odd: the 16-byte loop and its tail


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.fixture(scope="module")
def bucket(hiplib, dev):
    """The clean bucket on the device (never written: every case works on clones) and the unguarded optimizer's result for both
    (step, grad_scale) pairs, computed once."""
    from votenet_amd import mlp as M
    host, seg = C.bucket(0)
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    d["seg"] = torch.tensor([x for ab in seg for x in ab], dtype=torch.int64, device=dev)
    d["host"], d["segs"] = host, seg
    d["want"] = {}
    for step, scale in C.STEPS_SCALES:
        d["want"][(step, scale)] = _unguarded(M, d, d["g"], step, scale)
    return d


def _unguarded(M, d, g, step, scale):
    p, m, v = d["p"].clone(), d["m"].clone(), d["v"].clone()
    M.clip_adam(d["seg"], torch.zeros(M.SUMSQ_SLICES * len(d["segs"]), device=g.device), p, g, m, v, 1e-3, step, grad_scale=scale)
    return _bits(p), _bits(m), _bits(v)


def _guarded(M, d, g, step, scale, state, ema=None, snap=None):
    p, m, v = d["p"].clone(), d["m"].clone(), d["v"].clone()
    M.clip_adam_guarded(d["seg"], torch.zeros(M.SUMSQ_SLICES * len(d["segs"]), device=g.device), p, g, m, v, 1e-3, step, state,
                        ema=ema, ema_snapshot=snap, grad_scale=scale)
    return _bits(p), _bits(m), _bits(v)


def _state(dev):
    return torch.zeros(8, dtype=torch.int32, device=dev)


def _same(got, want):
    return all(torch.equal(a, b) for a, b in zip(got, want))


# ---- 1. a good step ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step,scale", C.STEPS_SCALES)
def test_a_good_step_is_clip_adam_bit_for_bit(bucket, dev, step, scale):
    from votenet_amd import mlp as M
    state = _state(dev)
    got = _guarded(M, bucket, bucket["g"], step, scale, state)
    want = bucket["want"][(step, scale)]
    assert _same(got, want), "p, m, v differ from votenet_clip_adam"
    assert not _same(got, (_bits(bucket["p"]), _bits(bucket["m"]), _bits(bucket["v"]))), "nothing was updated"
    assert state.cpu().tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    # the padding between the segments (NaN in every buffer) is neither read into the verdict nor written
    a0 = bucket["segs"][0][0]
    assert torch.equal(got[0][:a0], _bits(bucket["p"])[:a0])


def test_the_clip_is_applied_only_when_asked_for_but_the_verdict_always(bucket, dev):
    from votenet_amd import mlp as M
    d = bucket
    sumsq = torch.zeros(M.SUMSQ_SLICES * 4, device=dev)
    p, m, v = d["p"].clone(), d["m"].clone(), d["v"].clone()
    M.clip_adam(d["seg"], sumsq, p, d["g"], m, v, 1e-3, 3, clip=0.0)
    state = _state(dev)
    p2, m2, v2 = d["p"].clone(), d["m"].clone(), d["v"].clone()
    M.clip_adam_guarded(d["seg"], sumsq, p2, d["g"], m2, v2, 1e-3, 3, state, clip=0.0)
    assert _same((_bits(p2), _bits(m2), _bits(v2)), (_bits(p), _bits(m), _bits(v)))
    g = torch.from_numpy(C.poisoned(d["host"]["g"], d["segs"], "tail_region", "nan")).to(dev)
    p3, m3, v3 = d["p"].clone(), d["m"].clone(), d["v"].clone()
    M.clip_adam_guarded(d["seg"], sumsq, p3, g, m3, v3, 1e-3, 4, state, clip=0.0)
    assert _same((_bits(p3), _bits(m3), _bits(v3)), (_bits(d["p"]), _bits(d["m"]), _bits(d["v"])))
    assert state.cpu().tolist()[:6] == [1, 2, 1, 1, 4, 0]


def test_an_all_zero_gradient_is_good(bucket, dev):
    from votenet_amd import mlp as M
    g = torch.zeros_like(bucket["g"])
    state = _state(dev)
    got = _guarded(M, bucket, g, 1, 1.0, state)
    assert _same(got, _unguarded(M, bucket, g, 1, 1.0))
    assert state.cpu().tolist()[:6] == [0, 1, 0, 0, 0, 0]


# ---- 2. a bad step ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("position,value", C.BAD_CASES)
def test_a_bad_step_writes_nothing_and_is_counted(bucket, dev, position, value):
    from votenet_amd import mlp as M
    d = bucket
    step, scale = C.STEPS_SCALES[1]
    g = torch.from_numpy(C.poisoned(d["host"]["g"], d["segs"], position, value)).to(dev)
    assert C.verdict(g.cpu().numpy(), d["segs"])
    state = _state(dev)
    got = _guarded(M, d, g, step, scale, state)
    assert _same(got, (_bits(d["p"]), _bits(d["m"]), _bits(d["v"]))), "a skipped step changed a bit of p, m or v"
    assert state.cpu().tolist()[:6] == [1, 1, 1, 1, step, 0]
    # a following good step resets the run of skips and is again votenet_clip_adam
    got = _guarded(M, d, d["g"], step, scale, state)
    assert _same(got, d["want"][(step, scale)])
    assert state.cpu().tolist()[:6] == [0, 2, 1, 0, step, 0]


# ---- 3. the moving averages -------------------------------------------------------------------------------------------------------

def _ema(dev, offset=0):
    """(ema, snapshot): different finite contents; offset 1: views one float off the 16-byte grid (the scalar path)."""
    rng = np.random.default_rng(7)
    e = torch.from_numpy(rng.standard_normal(N_EMA + 1).astype(np.float32)).to(dev)[offset:offset + N_EMA]
    s = torch.from_numpy(rng.standard_normal(N_EMA + 1).astype(np.float32)).to(dev)[offset:offset + N_EMA]
    return e, s


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off_by_one_float"])
def test_ema_snapshot_rule(bucket, dev, offset):
    from votenet_amd import mlp as M
    d = bucket
    step, scale = C.STEPS_SCALES[0]
    bad_g = torch.from_numpy(C.poisoned(d["host"]["g"], d["segs"], "unrolled_third_accumulator", "+inf")).to(dev)
    untouched = (_bits(d["p"]), _bits(d["m"]), _bits(d["v"]))
    # good gradient + finite averages: the snapshot becomes the averages
    ema, snap = _ema(dev, offset)
    ema0 = _bits(ema)
    state = _state(dev)
    assert _same(_guarded(M, d, d["g"], step, scale, state, ema, snap), d["want"][(step, scale)])
    assert torch.equal(_bits(ema), ema0) and torch.equal(_bits(snap), ema0)
    assert state.cpu().tolist()[:6] == [0, 1, 0, 0, 0, 0]
    # bad gradient + finite averages: the averages become the old snapshot
    ema, snap = _ema(dev, offset)
    snap0 = _bits(snap)
    state = _state(dev)
    assert _same(_guarded(M, d, bad_g, step, scale, state, ema, snap), untouched)
    assert torch.equal(_bits(ema), snap0) and torch.equal(_bits(snap), snap0)
    assert state.cpu().tolist()[:6] == [1, 1, 1, 1, step, 1]
    # good gradient + one non-finite average (in the 16-byte loop, in its tail): restored, and the parameters still updated
    for where, val in ((5, float("nan")), (N_EMA - 1, float("inf")), (N_EMA // 2, float("-inf"))):
        ema, snap = _ema(dev, offset)
        ema[where] = val
        snap0 = _bits(snap)
        state = _state(dev)
        assert _same(_guarded(M, d, d["g"], step, scale, state, ema, snap), d["want"][(step, scale)])
        assert torch.equal(_bits(ema), snap0) and torch.equal(_bits(snap), snap0)
        assert state.cpu().tolist()[:6] == [0, 1, 0, 0, 0, 1]


def test_no_moving_averages_is_accepted(bucket, dev):
    from votenet_amd import mlp as M
    state = _state(dev)
    step, scale = C.STEPS_SCALES[0]
    assert _same(_guarded(M, bucket, bucket["g"], step, scale, state), bucket["want"][(step, scale)])
    bad_g = torch.from_numpy(C.poisoned(bucket["host"]["g"], bucket["segs"], "first_of_tensor0", "nan")).to(dev)
    _guarded(M, bucket, bad_g, step, scale, state)
    assert state.cpu().tolist()[:6] == [1, 2, 1, 1, step, 0]   # nothing to restore: nothing counted


# ---- 4. the model -----------------------------------------------------------------------------------------------------------------

def _batches(dev, seeds):
    from votenet_amd import loss as VL
    from votenet_amd import synth
    return [(torch.from_numpy(synth.room_batch(B, NPTS, s)).to(dev), VL.gt_to_device(synth.room_gt(B, NPTS, s), dev)) for s in seeds]


def _net(dev, seed, guard):
    from votenet_amd import model as VM
    net = VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL)
    net.init_optimizer(1e-3)
    if guard:
        net.enable_step_guard()
    return net


def _four(net):
    torch.cuda.synchronize()
    return _bits(net.store.flat), _bits(net._m), _bits(net._v), _bits(net._ema_flat)


def _ema_rows(net):
    """Moving mean | variance of every layer: what a checkpoint carries of _ema_flat (the blocks' two other rows are scratch that a
    restore leaves as it finds them, so two nets with different pasts differ there)."""
    return torch.cat([_bits(t[2:]).reshape(-1) for t in net._ema_state().values()])


def _finite(net):
    return bool(torch.isfinite(net.store.flat).all() and torch.isfinite(net._m).all() and torch.isfinite(net._v).all())


def test_guarded_steps_train_bit_identically_and_a_poisoned_step_does_no_harm(hiplib, dev):
    """Two nets from one seed in the bit-reproducible mode (mlp.set_deterministic: launch by launch; the default mode's atomics are not
    repeatable even against themselves, the captured stretch has the test below): three clean steps with and without the guard leave
    the same bits in store.flat, _m, _v and _ema_flat.  Then a step with one NaN among the fixed cotangents: the unguarded twin ends
    with non-finite parameters, the guarded net's four buffers keep every bit, predict() is finite and a further clean step trains.
    Then ground truth whose heading_residuals are +Inf.  The loss is Inf, but its cotangents are not: Huber's derivative saturates at
    +-1 (csrc/loss.hip, as tf.losses.huber_loss), and no entry of the ground truth reaches a cotangent any other way.  So the unguarded
    twin stays FINITE on that step -- it cannot be the poisoned case -- and the guard, whose verdict the loss value takes no part in,
    applies the step: bit-identical to the twin."""
    from votenet_amd import mlp as M
    batches = _batches(dev, (500, 502, 504, 506))
    prev = M.set_deterministic(True)
    try:
        off, on = _net(dev, 9, False), _net(dev, 9, True)
        for x, gt in batches[:3]:
            off.train_step(x, gt=gt)
            on.train_step(x, gt=gt)
        assert _same(_four(on), _four(off)), "a guarded clean step differs from an unguarded one"
        assert on.step_guard.read() == dict(seen=3, skipped=0, consecutive=0, last_skip_step=0, ema_restores=0, last_step_skipped=False)
        assert torch.equal(_bits(on.step_guard.snapshot), _bits(on._ema_flat))
        # Inf heading residuals: an Inf loss with finite gradients -- applied, identically
        x, gt = batches[3]
        gt_inf = dict(gt)
        gt_inf["heading_residuals"] = torch.full_like(gt["heading_residuals"], float("inf"))
        off.train_step(x, gt=gt_inf)
        on.train_step(x, gt=gt_inf)
        assert not torch.isfinite(on.last_losses[0]), "the Inf residual did not reach the loss"
        assert torch.isfinite(on.store.grad).all() and _finite(off)
        assert _same(_four(on), _four(off)) and on.step_guard.read()["skipped"] == 0
        # one NaN among the cotangents
        before = _four(on)
        cot = on.make_cotangents(B)
        cot["proposals_output"][1, 17, 40] = float("nan")
        off.train_step(x, cot=cot)
        torch.cuda.synchronize()
        assert not _finite(off), "the poisoned step left the unguarded twin finite: the case has no teeth"
        on.train_step(x, cot=cot)
        assert not torch.isfinite(on.store.grad).all()
        assert _same(_four(on), before), "a skipped step changed parameters, moments or moving averages"
        r = on.step_guard.read()
        assert (r["seen"], r["skipped"], r["consecutive"], r["last_skip_step"], r["ema_restores"]) == (5, 1, 1, 5, 1) and on._step == 5
    finally:
        M.set_deterministic(prev)
    out = on.predict(batches[0][0])
    assert torch.isfinite(out["bboxes"]).all() and torch.isfinite(out["scores"]).all()
    on.train_step(*batches[0][:1], gt=batches[0][1])
    after = _four(on)
    assert not torch.equal(after[0], before[0]) and _finite(on)
    assert on.step_guard.read()["consecutive"] == 0 and on.step_guard.read()["seen"] == 6


def test_a_label_outside_its_range_is_a_skipped_step(hiplib, dev):
    """Ground truth whose semantic labels are all nc (one past the last class): votenet_loss makes the class term and the class block's
    cotangents of every positive proposal NaN (include/votenet_hip.h), the gradient is not finite, and the guard skips the step: the
    four buffers keep every bit.  The nets, batches and steps are those of the test above, whose fourth step has positive proposals."""
    from votenet_amd import mlp as M
    from votenet_amd import synth
    batches = _batches(dev, (500, 502, 504, 506))
    prev = M.set_deterministic(True)
    try:
        on = _net(dev, 9, True)
        for x, gt in batches[:3]:
            on.train_step(x, gt=gt)
        before = _four(on)
        x, gt = batches[3]
        gt_bad = dict(gt)
        gt_bad["semantic_labels"] = torch.full_like(gt["semantic_labels"], synth.NC)
        on.train_step(x, gt=gt_bad)
        l = on.last_losses.cpu().numpy()
        assert l[10] > 0, "no positive proposal: the label was never used"
        assert np.isnan(l[0]) and np.isnan(l[8]) and np.isfinite(l[[1, 2, 3, 4, 5, 6, 7, 9]]).all()
        assert not torch.isfinite(on.store.grad).all()
        assert _same(_four(on), before), "a skipped step changed parameters, moments or moving averages"
        r = on.step_guard.read()
        assert (r["seen"], r["skipped"], r["consecutive"], r["last_skip_step"]) == (4, 1, 1, 4)
    finally:
        M.set_deterministic(prev)


def test_guarded_steps_through_the_captured_stretch(hiplib, dev, monkeypatch):
    """The default mode: the first step of a shape runs launch by launch, the following ones replay the captured stretch.  Two nets
    cannot be compared there (atomics), so every guarded optimizer call is checked against votenet_clip_adam on copies of exactly
    the buffers it was handed; the guard's snapshot follows the moving averages the replayed graph updated."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    assert not M.DETERMINISTIC and VM.STRETCH_GRAPH
    real, checked = M.clip_adam_guarded, []

    def checking(seg, sumsq, p, g, m, v, lr, step, state, ema=None, ema_snapshot=None, grad_scale=1.0, **kw):
        p2, m2, v2 = p.clone(), m.clone(), v.clone()
        real(seg, sumsq, p, g, m, v, lr, step, state, ema=ema, ema_snapshot=ema_snapshot, grad_scale=grad_scale, **kw)
        M.clip_adam(seg, torch.zeros_like(sumsq), p2, g, m2, v2, lr, step, grad_scale=grad_scale)
        checked.append(torch.equal(_bits(p), _bits(p2)) and torch.equal(_bits(m), _bits(m2)) and torch.equal(_bits(v), _bits(v2)))
    monkeypatch.setattr(M, "clip_adam_guarded", checking)
    net = _net(dev, 10, True)
    batches = _batches(dev, (510, 512, 514, 516))
    emas = []
    for x, gt in batches:
        net.train_step(x, gt=gt)
        emas.append(_bits(net._ema_flat))
        assert torch.equal(_bits(net.step_guard.snapshot), emas[-1])
    graphs = net.__dict__.get("_stretch_graphs", {})
    assert graphs and sum(g.replays for g in graphs.values()) >= 2, "the steps did not go through StretchGraph.replay"
    assert checked == [True] * 4 and not torch.equal(emas[-1], emas[-2])
    assert net.step_guard.read() == dict(seen=4, skipped=0, consecutive=0, last_skip_step=0, ema_restores=0, last_step_skipped=False)
    # a poisoned step while the stretch is captured (fixed cotangents run launch by launch beside it), then a replay again
    before = _four(net)
    cot = net.make_cotangents(B)
    cot["votes_xyz"][0, 3, 1] = float("nan")
    monkeypatch.setattr(M, "clip_adam_guarded", real)
    net.train_step(batches[0][0], cot=cot)
    assert _same(_four(net), before) and net.step_guard.read()["skipped"] == 1
    out = net.predict(batches[1][0])
    assert torch.isfinite(out["bboxes"]).all()
    net.train_step(batches[1][0], gt=batches[1][1])
    assert _finite(net) and not torch.equal(_four(net)[0], before[0]) and torch.isfinite(net._ema_flat).all()


# ---- 5. checkpoints ---------------------------------------------------------------------------------------------------------------

def test_a_resume_under_the_guard(hiplib, dev, tmp_path):
    from votenet_amd import mlp as M
    batches = _batches(dev, (520, 522, 524, 526))
    prev = M.set_deterministic(True)
    try:
        net = _net(dev, 11, True)
        for x, gt in batches[:2]:
            net.train_step(x, gt=gt)
        path = tmp_path / "guarded.npz"
        net.save(path)
        saved = _four(net)
        cot = net.make_cotangents(B)
        cot["proposals_output"][0, 0, 0] = float("inf")
        net.train_step(batches[2][0], cot=cot)
        assert net.step_guard.read()["skipped"] == 1 and _same(_four(net), saved) and net._step == 3
        net.load(path)
        plain = _net(dev, 12, False)
        plain.load(path)
        assert net._step == plain._step == 2
        for x, gt in batches[2:]:
            net.train_step(x, gt=gt)
            plain.train_step(x, gt=gt)
        assert _same(_four(net)[:3], _four(plain)[:3]) and torch.equal(_ema_rows(net), _ema_rows(plain)), \
            "a guarded resume differs from an unguarded one"
        # another state loaded: a bad step afterwards restores THAT state's averages, not the snapshot from before the load
        other = _net(dev, 13, False)
        other.train_step(batches[0][0], gt=batches[0][1])
        sd = other.state_dict()
        old_snapshot = _bits(net.step_guard.snapshot)
        net.load_state_dict(sd)
        loaded = _four(net)
        assert not torch.equal(loaded[3], old_snapshot) and torch.equal(_ema_rows(net), _ema_rows(other))
        net.train_step(batches[1][0], cot=cot)
        assert _same(_four(net), loaded) and net.step_guard.read()["skipped"] == 2
    finally:
        M.set_deterministic(prev)


# ---- 6. off means off -------------------------------------------------------------------------------------------------------------

def test_an_unguarded_step_never_reaches_the_new_entry(hiplib, dev, monkeypatch):
    from votenet_amd import mlp as M

    def boom(*a, **k):
        raise AssertionError("a guard launch in an unguarded step")
    monkeypatch.setattr(M, "clip_adam_guarded", boom)
    batches = _batches(dev, (530, 532, 534))
    net = _net(dev, 14, False)
    for x, gt in batches:           # launch by launch, then captured and replayed
        net.train_step(x, gt=gt)
    torch.cuda.synchronize()
    assert net.step_guard is None
    net.enable_step_guard()
    net.disable_step_guard()
    net.train_step(batches[0][0], gt=batches[0][1])
    torch.cuda.synchronize()
    net.enable_step_guard()
    with pytest.raises(AssertionError, match="guard launch"):   # the patch has teeth (the net is not used after this)
        net.train_step(batches[0][0], gt=batches[0][1])
    torch.cuda.synchronize()
