"""GPU: a VoteNetHotPath built with point features (height above the floor, colour) -- sa1 takes feats (B, n, c) beside the coordinates
and still runs its narrow first layer: forward against the CPU oracle, backward against float64 autograd, the prefetched geometry
(launch by launch and through the GeometryGraph ring), train steps through the stretch graph, checkpoints, predict."""
import numpy as np
import pytest
import torch

from test_gpu_backward import perturb, ref_chain, ref_fp, ref_sa
from test_gpu_model import N, oracle_chain, oracle_fp, oracle_sa

pytestmark = pytest.mark.gpu

SMALL = (512, 256, 128, 64)


def make_feats(x, c, seed):
    """(B, n, c) = [height above the floor | c - 1 random colours in [0, 1]] from the device feature builder on the cloud's own rows."""
    from votenet_amd import input_pipeline as IP
    b, n = x.shape[:2]
    g = torch.Generator().manual_seed(seed)
    colours = torch.rand(b * n, c - 1, generator=g).to(x.device)
    raw = torch.cat([x.reshape(b * n, 3), colours], 1).contiguous()
    choice = torch.arange(n, dtype=torch.int32, device=x.device).repeat(b, 1)
    points, feats, _ = IP.subsample_augment_features(raw, np.arange(b + 1, dtype=np.int64) * n, n, choice=choice, depth_to_camera=False,
                                                     height=True, extra_cols=c - 1)
    assert torch.equal(points, x) and feats.shape == (b, n, c)
    return feats


def batch(dev, seed, c=4, b=2, n=4096):
    from votenet_amd import synth
    x = torch.from_numpy(synth.room_batch(b, n, seed)).to(dev)
    return x, make_feats(x, c, seed)


@pytest.mark.parametrize("c", [4, 1])
def test_forward_small_vs_oracle_with_point_features(hiplib, dev, O, c):
    """tests/test_gpu_model.py::test_forward_small_vs_oracle with sa1 fed [height | colours] instead of the coordinates."""
    from votenet_amd import model as VM
    xt, ft = batch(dev, 77, c)
    x, f = N(xt), N(ft)
    net = VM.VoteNetHotPath(dev, seed=3, npoints=SMALL, point_features=c)
    assert tuple(net.store.views["sa1/conv0/W"].shape) == (3 + c, 64)
    assert net.sa1.narrow(2 * SMALL[0] * 64)  # the narrow form is the one that runs
    g = torch.Generator().manual_seed(1)
    for name, v in net.store.views.items():
        if name.endswith("gamma"):
            v.copy_((1 + 0.2 * torch.randn(v.shape, generator=g)).to(dev))
        if name.endswith("beta") or name.endswith("/b"):
            v.copy_((0.1 * torch.randn(v.shape, generator=g)).to(dev))
    tape = []
    out = net.forward(xt, tape, feats=ft)
    assert tape[0]["recs"][0]["kind"] == "narrow"

    l1x, l1p = oracle_sa(O, net.sa1, x, f)
    l2x, l2p = oracle_sa(O, net.sa2, l1x, l1p)
    l3x, l3p = oracle_sa(O, net.sa3, l2x, l2p)
    l4x, l4p = oracle_sa(O, net.sa4, l3x, l3p)
    l3p2 = oracle_fp(O, net.fp1, l3x, l4x, l3p, l4p)
    seeds = oracle_fp(O, net.fp2, l2x, l3x, l2p, l3p2)
    assert (N(tape[0]["new_xyz"]) == l1x).all() and (N(out["seeds_xyz"]) == l2x).all()  # centres: bit-exact

    def relerr(a, b):
        return np.abs(a - b).max() / max(1.0, np.abs(b).max())
    from votenet_amd import mlp as M
    net.store.refresh_split()
    M.arena_begin(dev)
    try:
        sa1_out = net.sa1.forward(xt, ft)[1]
    finally:
        M.arena_end()
    assert relerr(N(sa1_out), l1p) < 2e-5
    assert relerr(N(out["seeds_points"]), seeds) < 2e-5
    xx = np.concatenate([l2x, seeds], 2).reshape(-1, 259)
    votes = (xx + oracle_chain(O, xx, net.voting)).reshape(2, -1, 259)
    assert relerr(N(out["votes_xyz"]), votes[..., :3]) < 2e-5
    assert relerr(N(out["votes_points"]), votes[..., 3:]) < 2e-5
    vx, vp = N(out["votes_xyz"]), N(out["votes_points"])
    px, pout = oracle_sa(O, net.proposal, vx, vp, sample_xyz=l2x)
    assert (N(out["proposals_xyz"]) == px).all()
    assert relerr(N(out["proposals_output"]), pout) < 2e-5
    assert out["proposals_output"].shape == (2, 256, 79)


def test_full_backward_vs_autograd_with_point_features(hiplib, dev):
    """tests/test_gpu_backward.py::test_full_backward_vs_autograd (its shape, its bars) with point_features=4: every parameter gradient,
    the seven rows of sa1/conv0/W among them, against float64 autograd over the device's own indices and active sets."""
    from votenet_amd import model as VM
    x, feats = batch(dev, 5, 4, n=2048)
    net = VM.VoteNetHotPath(dev, seed=2, npoints=SMALL, point_features=4)
    perturb(net, dev)
    cot = {k: v * 100 for k, v in net.make_cotangents(2, seed=0).items()}
    net.store.grad.zero_()
    tape = []
    out = net.forward(x, tape, feats=feats)
    net.backward(tape, cot)
    assert tape[0]["recs"][0]["kind"] == "narrow"

    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in net.store.views.items()}
    xd, fd = x.double(), feats.double()
    sa1, sa2, sa3, sa4, fp1, fp2, vote, prop = tape
    l1x, l1p = ref_sa(net.sa1, params, xd, fd, sa1)
    l2x, l2p = ref_sa(net.sa2, params, l1x, l1p, sa2)
    l3x, l3p = ref_sa(net.sa3, params, l2x, l2p, sa3)
    l4x, l4p = ref_sa(net.sa4, params, l3x, l3p, sa4)
    l3p2 = ref_fp(net.fp1, params, l3p, l4p, fp1)
    seeds = ref_fp(net.fp2, params, l2p, l3p2, fp2)
    xx = torch.cat([l2x, seeds], 2).view(-1, 259)
    votes = (xx + ref_chain(xx, net.voting, params, vote["recs"])).view(2, -1, 259)
    vx, vp = votes[..., :3], votes[..., 3:]
    _, pout = ref_sa(net.proposal, params, vx, vp, prop)
    loss = (pout * cot["proposals_output"].double()).sum() + (vx * cot["votes_xyz"].double()).sum()
    loss.backward()
    worst = {}
    for name in net.store.views:
        ref = params[name].grad
        got = net.store.g(name).double()
        if name.endswith("/b") and not (name.endswith("fc2/b") or name.endswith("conv_post_2/b")):
            assert float(got.abs().max()) == 0.0  # bias of a BatchNorm'ed layer
            continue
        worst[name] = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-8)
    print("WORST", sorted(((round(v, 6), k) for k, v in worst.items()), reverse=True)[:10])
    assert tuple(net.store.g("sa1/conv0/W").shape) == (7, 64) and "sa1/conv0/W" in worst
    assert float(params["sa1/conv0/W"].grad[3:].abs().min(1).values.max()) > 0  # (every feature row carries gradient in the reference)
    bad = {k: round(v, 6) for k, v in worst.items() if v > 1e-4}
    assert not bad, bad
    assert np.median(list(worst.values())) < 2e-5


def test_prefetched_geometry_with_features_is_the_same_computation(hiplib, dev):
    """forward() on geometry prefetched by the previous call (next_x, next_feats) -- the first prefetch of a shape enqueued launch by
    launch, the later ones replayed from the GeometryGraph ring -- equals a fresh net's un-prefetched pass (geometry_ahead) bit for bit;
    features changed in place after the prefetch mean the geometry is computed again."""
    from votenet_amd import model as VM
    data = [batch(dev, 50 + i) for i in range(4)]
    fresh = VM.VoteNetHotPath(dev, seed=6, npoints=SMALL, point_features=4)
    refs = [{k: v.clone() for k, v in fresh.forward(x, feats=f).items()} for x, f in data]
    assert not fresh.__dict__.get("_prefetched")
    net = VM.VoteNetHotPath(dev, seed=6, npoints=SMALL, point_features=4)
    net.forward(data[0][0], feats=data[0][1], next_x=data[1][0], next_feats=data[1][1])
    served = []
    for i in range(1, 9):
        x, f = data[i % 4]
        nx, nf = data[(i + 1) % 4]
        entry = net._prefetched[id(x)]
        assert entry.x is x and entry.feats is f
        served.append(entry.graph is not None)
        got = net.forward(x, feats=f, next_x=[nx], next_feats=[nf])
        for k in refs[0]:
            assert torch.equal(got[k], refs[i % 4][k]), (i, k)
    assert served[0] is False and served[-1] is True  # launch by launch first, then graphs
    ring = next(iter(net._geometry.rings.values()))
    assert len(ring["graphs"]) == VM.GEOMETRY_RING and all(g.feats is not None for g in ring["graphs"])
    # stale features: changed in place after the prefetch
    x, f = data[1]
    net.prefetch_geometry(x, f)
    assert net._prefetched[id(x)].graph is not None
    f.add_(1)
    want = fresh.forward(x, feats=f)
    got = net.forward(x, feats=f)
    assert not net._prefetched
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["proposals_output"], refs[1]["proposals_output"])
    # ... and another feature tensor of the same values is not the prefetched one either, with the same result
    net.prefetch_geometry(x, f)
    f2 = f.clone()
    got = net.forward(x, feats=f2)
    assert torch.equal(got["proposals_output"], want["proposals_output"])
    # the same through the launch-by-launch prefetch (graphs off)
    net.drop_graphs()
    net._geometry.graphs_off = True
    net.prefetch_geometry(x, f)
    assert net._prefetched[id(x)].graph is None
    f.add_(1)
    want = fresh.forward(x, feats=f)
    got = net.forward(x, feats=f)
    assert torch.equal(got["proposals_output"], want["proposals_output"])


def test_train_steps_with_point_features(hiplib, dev, tmp_path):
    from votenet_amd import loss as VL
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    from votenet_amd import synth
    seeds = (300, 302, 304)
    data = [batch(dev, s) for s in seeds]
    gts = [VL.gt_to_device(synth.room_gt(2, 4096, s), dev) for s in seeds]
    net = VM.VoteNetHotPath(dev, seed=0, npoints=SMALL, point_features=4)
    before = {k: v.clone() for k, v in net.store.views.items()}
    for i in range(2):
        nxt = dict(next_x=data[1][0], next_feats=data[1][1]) if i == 0 else {}  # (the second step runs on prefetched geometry)
        net.train_step(data[i][0], gt=gts[i], feats=data[i][1], **nxt)
    torch.cuda.synchronize()
    graphs = net.__dict__.get("_stretch_graphs", {})
    assert len(graphs) == 1 and next(iter(graphs.values())).replays == 1  # the second step replayed the captured stretch
    assert net._step == 2 and bool(torch.isfinite(net.last_losses).all())
    for k, v in net.store.views.items():
        assert bool(torch.isfinite(v).all()), k
        if not (k.endswith("/b") and not (k.endswith("fc2/b") or k.endswith("conv_post_2/b"))):  # (a BatchNorm'ed layer's bias has no gradient)
            assert not torch.equal(v, before[k]), k
    assert tuple(net.store.views["sa1/conv0/W"].shape) == (7, 64)
    assert float((net.store.views["sa1/conv0/W"] - before["sa1/conv0/W"]).abs().min(1).values.max()) > 0  # every input row moved
    path = str(tmp_path / "pf.npz")
    net.save(path)
    other = VM.VoteNetHotPath(dev, seed=9, npoints=SMALL, point_features=4)
    other.load(path)
    plain = VM.VoteNetHotPath(dev, seed=9, npoints=SMALL)
    with pytest.raises(ValueError, match="7 input rows.*6"):
        plain.load(path)
    prev = M.set_deterministic(True)
    try:
        for m in (net, other):
            m.train_step(data[2][0], gt=gts[2], feats=data[2][1])
        torch.cuda.synchronize()
    finally:
        M.set_deterministic(prev)
    sa, sb = net.state_dict(), other.state_dict()
    differ = [k for k in sa if not np.array_equal(sa[k], sb[k])]
    assert int(sb["global_step"]) == 3 and list(sa) == list(sb) and not differ, differ[:5]
    assert torch.equal(net.last_losses.cpu(), other.last_losses.cpu())


def test_predict_and_the_default_network(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import evaluator as E
    from votenet_amd import model as VM
    from votenet_amd import synth
    x, f = batch(dev, 90000)
    net = VM.VoteNetHotPath(dev, seed=1, npoints=SMALL, point_features=4)
    base = VM.VoteNetHotPath(dev, seed=1, npoints=SMALL)
    got = net.predict(x, feats=f, batch_statistics=True)
    want = base.predict(x, batch_statistics=True)
    assert set(got) == set(want)
    for k in want:
        if torch.is_tensor(want[k]) and k != "nms_idx":
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert bool(torch.isfinite(got["proposals_output"]).all())
    with pytest.raises(L.InvalidArgumentError, match="point_features=4"):
        net.predict(x)
    with pytest.raises(L.InvalidArgumentError, match="without point features"):
        base.predict(x, feats=f)
    with pytest.raises(L.InvalidArgumentError, match="without point features"):
        base.forward(x, feats=f)
    with pytest.raises(L.InvalidArgumentError):
        net.forward(x, feats=f[:, :, :3].contiguous())
    # the evaluator takes (x, feats) pairs
    x2, f2 = batch(dev, 90002)
    gts = [E.gt_for_eval(synth.room_gt(2, 4096, s)) for s in (90000, 90002)]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (untrained moving averages)
        res = E.evaluate(net, [(x, f), (x2, f2)], gts, (0.25,))
    assert set(res) == {0.25} and "mAP" in res[0.25]
