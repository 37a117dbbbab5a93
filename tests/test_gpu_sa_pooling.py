"""GPU: SAModule's group_all and its pooling modes (csrc/pool_modes.hip) against a float64 torch restatement of the reference's
sample_and_group_all / pointnet_sa_module (utils.py:64-158), run on the module's own idx / new_xyz; and the new ABI entries against
numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 1e-5
MODES = ["avg", "weighted_avg", "max_and_avg", "max"]


def relerr(a, b):
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def fwd_err(a, b):
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def ref_chain(x, layers, params, recs):
    """float64 BN (training mode, biased variance) + ReLU chain; the ReLU's active set is the device's wherever it stored z (a
    fp32-vs-fp64 sign flip of a near-zero pre-activation would otherwise reroute a gradient and say nothing about the kernels)."""
    for L, r in zip(layers, recs):
        z = x @ params[L.name + "/W"] + params[L.name + "/b"]
        if L.bn:
            mu = z.mean(0)
            var = z.var(0, unbiased=False)
            z = params[L.name + "/gamma"] * (z - mu) / torch.sqrt(var + EPS) + params[L.name + "/beta"]
        if L.relu:
            if r.get("z") is not None and r.get("half") is None:
                z = z * (r["z"] * r["scale"] + r["shift"] > 0).double()
            else:
                z = torch.relu(z)
        x = z
    return x


def safe_norm(v):
    """|v| whose gradient at v = 0 is 0 (the project's rule; tf.norm gives 0 * inf = NaN there)."""
    sq = (v * v).sum(-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def ref_sa(mod, params, xyz, pts, rec, centre_shift=None):
    """utils.py:64-158 in float64 on the module's grouping.  centre_shift: a constant added to the gathered centres (a test that
    moved a centre away from every point to get an empty ball)."""
    b, n = xyz.shape[:2]
    dev = xyz.device
    if mod.group_all:
        m, k = 1, n
        grouped_xyz = xyz[:, None]                                      # utils.py:82, uncentred
        rows = grouped_xyz if pts is None else torch.cat([xyz, pts], -1)[:, None]
        new_xyz = torch.zeros((b, 1, 3), dtype=xyz.dtype, device=dev)
    else:
        idx = rec["idx"].long()
        m, k = idx.shape[1:]
        bi = torch.arange(b, device=dev)[:, None, None]
        new_xyz = xyz[torch.arange(b, device=dev)[:, None], rec["fps_idx"].long()]
        if centre_shift is not None:
            new_xyz = new_xyz + centre_shift
        grouped_xyz = xyz[bi, idx] - new_xyz[:, :, None, :]             # utils.py:50-51
        rows = grouped_xyz if pts is None else torch.cat([grouped_xyz, pts[bi, idx]], -1)
    y = ref_chain(rows.reshape(b * m * k, -1), mod.mlp, params, rec["recs"]).view(b * m, k, -1)
    mean = y.mean(1)
    if mod.pooling in ("max", "max_and_avg"):
        # max through the device's arg-max, checked to be a float64 maximum up to fp32 round-off first
        with torch.no_grad():
            picked = y.gather(1, rec["argmax"].long()[:, None, :])[:, 0, :]
            top = y.max(1).values
            tol = 1e-4 * max(1.0, float(y.abs().max()))
            assert bool((picked >= top - tol).all()), "device arg-max misses the maximum by %g" % float((top - picked).max())
        mx = y.gather(1, rec["argmax"].long()[:, None, :])[:, 0, :]
        last = rec["recs"][-1]
        if last["z"] is None:  # Gram form (the default max path): the device's active set at the arg-max entries
            mx = mx * (rec["zsel"] * last["scale"] + last["shift"] > 0).double()
    if mod.pooling == "max":
        out = mx
    elif mod.pooling == "avg":
        out = mean
    elif mod.pooling == "max_and_avg":
        out = torch.cat([mean, mx], -1)                                  # utils.py:143-146
    else:
        d = safe_norm(grouped_xyz).reshape(b * m, k)                    # utils.py:135-140
        w = torch.softmax(-d * 5, dim=1)
        out = (y * w[..., None]).sum(1)
    if mod.mlp2:
        out = ref_chain(out, mod.mlp2, params, rec["recs2"])
    return new_xyz, out.view(b, m, -1)


def perturb(store):
    g = torch.Generator().manual_seed(1)
    for name, v in store.views.items():
        if name.endswith("gamma"):
            v.copy_((1 + 0.2 * torch.randn(v.shape, generator=g)).to(v.device))
        if name.endswith("beta") or name.endswith("/b"):
            v.copy_((0.1 * torch.randn(v.shape, generator=g)).to(v.device))


def build(dev, npoint, radius, nsample, cin, mlp, mlp2=None, **kw):
    from votenet_amd import pointnet2 as P
    store = P.ParamStore(dev)
    mod = P.SAModule(store, "t", npoint, radius, nsample, cin, mlp, mlp2=mlp2, **kw)
    store.materialize(4)
    perturb(store)
    return store, mod


def run(store, mod, xyz, pts, seed=3, geom=None, need_xyz=True):
    from votenet_amd import pointnet2 as P
    tape = []
    new_xyz, out, idx = mod.forward(xyz, pts, tape=tape, geom=geom)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)
    store.grad.zero_()
    d_feat, d_xyz = mod.backward(tape[0], gout, need_feat_grad=pts is not None, need_xyz_grad=need_xyz)
    P.wgrad_join()
    torch.cuda.synchronize()
    return tape[0], new_xyz, out, idx, gout, d_feat, d_xyz


def check_vs_ref(store, mod, xyz, pts, res, centre_shift=None, need_xyz=True):
    rec, new_xyz, out, idx, gout, d_feat, d_xyz = res
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in store.views.items()}
    xd = xyz.double().requires_grad_(need_xyz)
    pd = pts.double().requires_grad_(True) if pts is not None else None
    rnew, y = ref_sa(mod, params, xd, pd, rec, centre_shift)
    (y * gout.double()).sum().backward()
    assert torch.equal(new_xyz.double(), rnew.detach())
    e = fwd_err(out.double(), y.detach())
    assert e < 1e-5, "forward %g" % e
    if pd is not None:
        assert relerr(d_feat.double(), pd.grad) < 1e-4, relerr(d_feat.double(), pd.grad)
    if need_xyz:
        assert bool(torch.isfinite(d_xyz).all())
        assert relerr(d_xyz.double(), xd.grad) < 1e-4, relerr(d_xyz.double(), xd.grad)
    plain = {L.name + "/b" for L in (mod.mlp2 or []) if not L.bn}  # a BatchNorm'ed layer's bias gradient is 0 (left at 0)
    for name in store.views:
        if not name.endswith("/b") or name in plain:
            assert relerr(store.g(name).double(), params[name].grad) < 1e-4, (name, relerr(store.g(name).double(), params[name].grad))


def small_cloud(dev, b, n, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(b, n, 3, generator=g)
    xyz[:, -3:] += 3.0  # a few isolated points: their balls hold fewer hits than nsample
    pts = torch.randn(b, n, c, generator=g) if c else None
    return xyz.to(dev), (pts.to(dev) if pts is not None else None)


@pytest.mark.parametrize("pooling", MODES)
def test_small_balls_with_padding_and_an_empty_ball(hiplib, dev, pooling):
    """B = 2, n = 600, nsample 16: balls with pts_cnt < nsample (their padding rows count in the mean and the softmax) and one
    centre moved away from every point (pts_cnt 0)."""
    from votenet_amd import pointnet2 as P, tf_grouping
    store, mod = build(dev, 48, 0.15, 16, 6, [32, 64], pooling=pooling)
    xyz, pts = small_cloud(dev, 2, 600, 6)
    fps_idx, new_xyz, _, _ = P.sample_and_group(48, 0.15, 16, xyz)
    shift = torch.zeros_like(new_xyz)
    shift[1, 5] = 50.0
    moved = new_xyz + shift
    idx, cnt = tf_grouping.query_ball_point(0.15, 16, xyz, moved)
    assert int(cnt[1, 5]) == 0 and bool((cnt < 16).any())
    geom = P.SAGeometry(fps_idx, moved, P.M.attach_inverse(idx, 600), cnt)
    res = run(store, mod, xyz, pts, geom=geom)
    check_vs_ref(store, mod, xyz, pts, res, centre_shift=moved.double() - new_xyz.double())  # exact: the device's moved centres


@pytest.mark.parametrize("pooling", MODES)
def test_proposal_like_shape_with_mlp2(hiplib, dev, pooling):
    """256 centres, nsample 16, cin 128, [128, 128, 128], mlp2 behind the pool (on 2 x 128 channels after max_and_avg)."""
    store, mod = build(dev, 256, 0.3, 16, 128, [128, 128, 128], mlp2=[128, 64], pooling=pooling)
    g = torch.Generator().manual_seed(5)
    xyz = torch.rand(2, 1024, 3, generator=g).to(dev)
    pts = torch.randn(2, 1024, 128, generator=g).to(dev)
    res = run(store, mod, xyz, pts)
    check_vs_ref(store, mod, xyz, pts, res)


@pytest.mark.parametrize("n,cin,mlp", [(1000, 6, [32, 64]), (20480, 16, [64, 128, 256]), (80000, 3, [16, 32])],
                         ids=["n1000", "n20480", "n80000"])
@pytest.mark.parametrize("pooling", MODES)
def test_group_all(hiplib, dev, pooling, n, cin, mlp):
    store, mod = build(dev, 99, 0.1, 7, cin, mlp, pooling=pooling, group_all=True)
    g = torch.Generator().manual_seed(6)
    xyz = (torch.rand(2, n, 3, generator=g) * 2 - 1).to(dev)
    xyz[0, 7] = 0.0  # a point at the origin: |v| = 0 in weighted_avg's softmax
    pts = torch.randn(2, n, cin, generator=g).to(dev)
    res = run(store, mod, xyz, pts)
    rec, new_xyz, out, idx = res[:4]
    assert out.shape == (2, 1, mlp[-1] * (2 if pooling == "max_and_avg" else 1))
    assert new_xyz.shape == (2, 1, 3) and not bool(new_xyz.any())
    assert idx.dtype == torch.int32 and idx.shape == (2, 1, n) and torch.equal(idx[1, 0].long().cpu(), torch.arange(n))
    check_vs_ref(store, mod, xyz, pts, res)


def test_group_all_without_features(hiplib, dev):
    store, mod = build(dev, 1, None, None, 0, [32, 64], pooling="weighted_avg", group_all=True)
    xyz = torch.rand(2, 500, 3, generator=torch.Generator().manual_seed(8)).to(dev)
    res = run(store, mod, xyz, None)
    check_vs_ref(store, mod, xyz, None, res)


@pytest.mark.parametrize("group_all", [False, True])
@pytest.mark.parametrize("pooling", ["avg", "weighted_avg", "max_and_avg", "max"])
def test_deterministic_mode_is_bit_reproducible(hiplib, dev, pooling, group_all):
    from votenet_amd import mlp as M
    if pooling == "max" and not group_all:
        pytest.skip("the default path: tests/test_gpu_backward.py::test_training_gradients_are_bit_reproducible")
    prev = M.set_deterministic(True)
    try:
        store, mod = build(dev, 64, 0.3, 16, 16, [32, 64], pooling=pooling, group_all=group_all)
        g = torch.Generator().manual_seed(9)
        xyz = torch.rand(2, 3000, 3, generator=g).to(dev)
        pts = torch.randn(2, 3000, 16, generator=g).to(dev)
        outs = []
        for _ in range(2):
            _, _, out, _, _, d_feat, d_xyz = run(store, mod, xyz, pts)
            outs.append((out.clone(), d_feat.clone(), d_xyz.clone(), store.grad.clone()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    finally:
        M.set_deterministic(prev)


def test_default_arguments_are_the_max_path_bit_for_bit(hiplib, dev):
    """No new argument = pooling='max', group_all=False: the same fused path (deterministic mode, so that two runs can be compared
    bit for bit)."""
    from votenet_amd import mlp as M, pointnet2 as P
    xyz, pts = small_cloud(dev, 2, 2000, 16, seed=2)
    results = []
    for kw in ({}, dict(pooling="max", group_all=False)):
        store, mod = build(dev, 64, 0.2, 64, 16, [64, 128, 256], **kw)
        assert not mod.plain_pool
        prev = M.set_deterministic(True)
        try:
            _, _, out, _, _, d_feat, d_xyz = run(store, mod, xyz, pts)
        finally:
            M.set_deterministic(prev)
        results.append((out, d_feat, d_xyz, store.grad.clone()))
    for a, b in zip(*results):
        assert torch.equal(a, b)
    assert P.SAModule.__init__.__defaults__[-2:] == ("max", False)


# ---------------------------------------------------------------- kernel level
def np_pool(y, k, mode, w=None):
    g = y.reshape(-1, k, y.shape[1]).astype(np.float64)
    if mode == "avg":
        return g.mean(1)
    if mode == "weighted_avg":
        return (g * w.reshape(-1, k, 1)).sum(1)
    if mode == "max":
        return g.max(1)
    return np.concatenate([g.mean(1), g.max(1)], 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("groups,k,c", [(5, 1, 3), (7, 7, 6), (9, 16, 130), (33, 13, 128), (2, 5000, 130), (3, 20001, 64), (1, 3, 1)])
@pytest.mark.parametrize("unaligned", [False, True])
def test_bn_relu_pool_vs_numpy(hiplib, dev, mode, groups, k, c, unaligned):
    from votenet_amd import mlp as M
    rng = np.random.default_rng(groups * 1000 + k + c)
    zn = rng.normal(size=(groups * k, c)).astype(np.float32)
    sc = rng.normal(size=c).astype(np.float32)
    sh = (0.3 * rng.normal(size=c)).astype(np.float32)
    wn = rng.random(groups * k).astype(np.float32)
    buf = torch.empty(groups * k * c + 1, dtype=torch.float32, device=dev)
    z = buf[1:].view(groups * k, c) if unaligned else buf[:-1].view(groups * k, c)
    z.copy_(torch.from_numpy(zn))
    T = lambda a: torch.from_numpy(a).to(dev)
    out, arg = M.bn_relu_pool(z, k, T(sc), T(sh), True, mode, w=T(wn), want_argmax=True)
    y = np.maximum(zn * sc + sh, 0)
    exp = np_pool(y, k, mode, wn)
    assert np.abs(out.cpu().numpy() - exp).max() / max(1.0, np.abs(exp).max()) < 1e-5
    if mode in ("max", "max_and_avg"):
        yk = y.reshape(groups, k, c)
        assert (arg.cpu().numpy() == yk.argmax(1)).all()  # the first maximum in row order
    else:
        assert arg is None
    # the gradient reaching y, against numpy
    gout = rng.normal(size=out.shape).astype(np.float32)
    da = M.sa_pool_grad(T(gout), k, c, mode, w=T(wn), argmax=arg).cpu().numpy().reshape(groups, k, c)
    e = np.zeros((groups, k, c))
    if mode in ("avg", "max_and_avg"):
        e += gout[:, None, :c] / k
    if mode == "weighted_avg":
        e += wn.reshape(groups, k, 1) * gout[:, None, :]
    if mode in ("max", "max_and_avg"):
        a = arg.cpu().numpy()
        gm = gout[:, c:] if mode == "max_and_avg" else gout
        for gg in range(groups):
            e[gg, a[gg], np.arange(c)] += gm[gg]
    assert np.abs(da - e).max() <= 1e-6 * max(1.0, np.abs(e).max())


def test_pool_entries_handle_zero_groups_and_reject_a_bad_mode(hiplib, dev):
    from votenet_amd import _lib as L, mlp as M
    z = torch.empty((0, 8), device=dev)
    s = torch.ones(8, device=dev)
    out, arg = M.bn_relu_pool(z, 4, s, s, True, "max_and_avg", want_argmax=True)
    assert out.shape == (0, 16) and arg.shape == (0, 8)
    assert M.sa_pool_grad(torch.empty((0, 8), device=dev), 4, 8, "avg").shape == (0, 8)
    z = torch.ones((8, 8), device=dev)
    o = torch.empty((2, 8), device=dev)
    with pytest.raises(L.InvalidArgumentError):
        L.check(L.lib().votenet_bn_relu_pool(2, 4, 8, z.data_ptr(), s.data_ptr(), s.data_ptr(), 1, 4, None, o.data_ptr(), None, None,
                                             L.stream_ptr()))
    with pytest.raises(L.InvalidArgumentError):
        L.check(L.lib().votenet_sa_pool_grad(2, 4, 8, 9, o.data_ptr(), None, None, z.data_ptr(), L.stream_ptr()))
    with pytest.raises(L.InvalidArgumentError):  # weighted_avg without its weights
        M.bn_relu_pool(z, 4, s, s, True, "weighted_avg")


@pytest.mark.parametrize("m,k", [(1, 1), (3, 7), (16, 64), (1, 5000)])
def test_sa_pool_weights_vs_numpy(hiplib, dev, m, k):
    from votenet_amd import mlp as M
    rng = np.random.default_rng(m + k)
    b, n = 2, max(k, 50)
    xyz = rng.random((b, n, 3)).astype(np.float32)
    X = torch.from_numpy(xyz).to(dev)
    if m == 1 and k == n:  # group_all: the raw coordinates
        w = M.sa_pool_weights(X).cpu().numpy().reshape(b, 1, k)
        v = xyz[:, None].astype(np.float64)
    else:
        idx = rng.integers(0, n, size=(b, m, k)).astype(np.int32)
        cen = rng.random((b, m, 3)).astype(np.float32)
        w = M.sa_pool_weights(X, torch.from_numpy(cen).to(dev), torch.from_numpy(idx).to(dev)).cpu().numpy().reshape(b, m, k)
        v = xyz[np.arange(b)[:, None, None], idx].astype(np.float64) - cen[:, :, None].astype(np.float64)
    s = -5 * np.sqrt((v * v).sum(-1))
    e = np.exp(s - s.max(-1, keepdims=True))
    e /= e.sum(-1, keepdims=True)
    assert np.abs(w - e).max() < 1e-6
