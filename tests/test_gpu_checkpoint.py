"""GPU: checkpoints of a training run (votenet_amd/checkpoint.py) on the suite's small shape (2 x 4096 points, 512/256/128/64 samples).
A resumed run equals the uninterrupted one bit for bit (deterministic mode); a loaded model serves the trained model's predictions;
a load into a model whose train step is replayed from captured HIP graphs (StretchGraph: the addresses of the parameter bucket and
of the moving averages baked in) trains on the loaded state, as a fresh model that loaded the same file does."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NPTS, SMALL = 2, 4096, (512, 256, 128, 64)


def _batches(dev, seeds):
    from votenet_amd import loss as VL
    from votenet_amd import synth
    return [(torch.from_numpy(synth.room_batch(B, NPTS, s)).to(dev), VL.gt_to_device(synth.room_gt(B, NPTS, s), dev)) for s in seeds]


def _net(dev, seed):
    from votenet_amd import model as VM
    return VM.VoteNetHotPath(dev, seed=seed, npoints=SMALL)


def _train(net, batches):
    for x, gt in batches:
        net.train_step(x, gt=gt)
    torch.cuda.synchronize()


def _predict(net, x):
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*moving averages.*")  # a loaded model's moving averages are trained ones
        r = net.predict(x, 0.25)
    torch.cuda.synchronize()
    return {k: r[k].cpu() for k in ("proposals_output", "bboxes", "nms_idx")}


def _rel(a, b):
    """max |a - b| over the largest magnitude of b (0 when both are 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = float(np.abs(a - b).max()) if a.size else 0.0
    return d / max(float(np.abs(b).max()), 1e-30) if d else 0.0


def test_a_resumed_run_equals_the_uninterrupted_run_bit_for_bit(hiplib, dev, tmp_path):
    """A: 4 steps.  B: the same first 2 steps, saved.  C (another seed) loads B's file and runs steps 3-4: C == A in every value of the
    state (parameters, moving averages, Adam moments, step, rate), and in the losses of the last step."""
    from votenet_amd import mlp as M
    batches = _batches(dev, (300, 302, 304, 306))
    path = str(tmp_path / "b.npz")
    prev = M.set_deterministic(True)
    try:
        a = _net(dev, 0)
        _train(a, batches)
        b = _net(dev, 0)
        _train(b, batches[:2])
        b.save(path)
        c = _net(dev, 9)
        c.load(path)
        _train(c, batches[2:])
    finally:
        M.set_deterministic(prev)
    sa, sc = a.state_dict(), c.state_dict()
    assert int(sc["global_step"]) == 4 and list(sa) == list(sc)
    differ = [k for k in sa if not np.array_equal(sa[k], sc[k])]
    assert not differ, "%d of %d entries differ, first: %s" % (len(differ), len(sa), differ[:5])
    assert torch.equal(a.last_losses.cpu(), c.last_losses.cpu())


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "default"])
def test_a_loaded_model_serves_the_trained_model_predictions(hiplib, dev, tmp_path, deterministic):
    """SaverRestore + OfflinePredictor (evaluator.py:239-243): a fresh model that loads a trained model's file predicts what the trained
    model predicts -- bit-equal in deterministic mode, within 1e-5 of the tensor maximum in the default mode (fp32 atomics)."""
    from votenet_amd import mlp as M
    batches = _batches(dev, (310, 312, 314))
    xv = _batches(dev, (90000,))[0][0]
    path = str(tmp_path / "t.npz")
    prev = M.set_deterministic(deterministic)
    try:
        t = _net(dev, 1)
        _train(t, batches)
        t.save(path, optimizer=False)
        s = _net(dev, 2)
        s.load(path)
        pt, ps = _predict(t, xv), _predict(s, xv)
    finally:
        M.set_deterministic(prev)
    assert torch.equal(pt["nms_idx"], ps["nms_idx"])
    for k in ("proposals_output", "bboxes"):
        if deterministic:
            assert torch.equal(pt[k], ps[k]), k
        else:
            assert _rel(ps[k], pt[k]) <= 1e-5, (k, _rel(ps[k], pt[k]))


def test_a_load_into_a_model_with_captured_graphs_trains_on_the_loaded_state(hiplib, dev, tmp_path):
    """D trains 3 steps in the default mode (eager, capture, replay: its StretchGraph holds the addresses of store.flat, bn_flat and
    _ema_flat), then loads a file written by E, trained differently.  F, fresh, loads the same file.  D's predictions equal F's, and
    after one more step on the same batch (D: a graph replay; F: eager) the losses, moving averages, gradients and parameters of the two
    agree to 1e-5 of each tensor's maximum (parameters: where the gradient is above round-off, see below).  A swapped buffer or a stale
    weight image would differ by orders of magnitude more."""
    from votenet_amd import mlp as M
    assert not M.DETERMINISTIC
    batches = _batches(dev, (320, 322, 324, 326))
    xv = _batches(dev, (90002,))[0][0]
    path = str(tmp_path / "e.npz")
    d = _net(dev, 3)
    _train(d, batches[:3])
    graphs = d.__dict__.get("_stretch_graphs") or {}
    assert len(graphs) == 1, "the default train step did not capture its stretch"
    sg = next(iter(graphs.values()))
    assert sg.replays >= 2
    e = _net(dev, 4)
    _train(e, batches[2:])
    e.save(path)
    f = _net(dev, 5)
    f.load(path)
    ptrs = (d.store.flat.data_ptr(), d.store.bn_flat.data_ptr(), d._ema_flat.data_ptr(), d._m.data_ptr(), d._v.data_ptr())
    d.load(path)
    assert (d.store.flat.data_ptr(), d.store.bn_flat.data_ptr(), d._ema_flat.data_ptr(), d._m.data_ptr(), d._v.data_ptr()) == ptrs
    sd, sf = d.state_dict(), f.state_dict()
    assert all(np.array_equal(sd[k], sf[k]) for k in sf)  # the same bits in both, whatever D held before
    pd, pf = _predict(d, xv), _predict(f, xv)
    assert torch.equal(pd["nms_idx"], pf["nms_idx"])
    for k in ("proposals_output", "bboxes"):
        assert _rel(pd[k], pf[k]) <= 1e-5, (k, _rel(pd[k], pf[k]))
    replays = sg.replays
    x, gt = batches[0]
    _train(d, [(x, gt)])
    _train(f, [(x, gt)])
    assert sg.replays == replays + 1 and d.__dict__["_stretch_graphs"].get(next(iter(graphs))) is sg  # D's step was the replay
    ld, lf = d.last_losses.cpu(), f.last_losses.cpu()
    assert torch.allclose(ld, lf, rtol=1e-5, atol=1e-7), (ld, lf)
    sd, sf = d.state_dict(), f.state_dict()
    assert int(sd["global_step"]) == int(sf["global_step"]) == 3
    worst = max((_rel(sd[k], sf[k]), k) for k in sf if k.endswith("/EMA"))
    assert worst[0] <= 1e-5, worst
    # the step's gradients (the clip / Adam kernel reads store.grad and leaves it) and the parameters.  D and F held the same bits
    # before the step, so their parameters differ by their Adam updates alone, and Adam divides every element by its own RMS: where an
    # element's gradient is round-off (voting2/b's feature columns: ~1e-8 of the tensor's largest gradient) the update is noise of up to
    # a few lr -- two fresh models that load the same file and take the step eagerly differ there just as much (2e-2 of the tensor
    # maximum, measured).  Everywhere else the parameters agree to 1e-5 of the tensor maximum.
    lr = float(sf["learning_rate"])
    for name in f.store.views:
        gd, gf = d.store.g(name).cpu().numpy(), f.store.g(name).cpu().numpy()
        assert _rel(gd, gf) <= 1e-5, (name, _rel(gd, gf))
        qd, qf = d.store[name].cpu().numpy(), f.store[name].cpu().numpy()
        dp = np.abs(qd.astype(np.float64) - qf)
        gmax = max(float(np.abs(gf).max()), 1e-30)
        signal = np.maximum(np.abs(gd), np.abs(gf)) > 1e-5 * gmax
        tol = 1e-5 * float(np.abs(qf).max())
        assert (dp[signal] <= tol).all(), (name, float(dp[signal].max()), tol)
        assert (dp <= 4 * lr + tol).all(), (name, float(dp.max()))
