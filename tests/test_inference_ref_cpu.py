"""CPU: tests/inference_ref.py (the float64 restatement the GPU inference tests compare with) held to two independent statements of
the same arithmetic at small shapes -- torch.nn.functional.batch_norm in float64, layer by layer, and the CPU oracle composed as
tests/test_gpu_model.py:oracle_chain composes it (fp32 storage: 1e-5 of max(1, max |ref|)).  Both routes run every chain form: negative
and exactly-zero gamma channels, BatchNorm layers without ReLU, a plain last layer without BatchNorm."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inference_ref as R  # noqa: E402

B, N, M_, K = 2, 40, 6, 8            # grouped rows: 2 x 6 x 8 = 96
CIN, WIDTHS = 3, (6, 16, 32)          # grouped width 3 + 3 = 6
L = R.Layer
CHAINS = {  # (bn, relu) per layer
    "bn_relu": [(True, True)] * 3,
    "relu_false_inside": [(True, True), (True, False), (True, True)],
    "relu_false_last": [(True, True), (True, True), (True, False)],
    "plain_last": [(True, True), (True, True), (False, False)],
}
MODES = ("moving", "batch")


def make_chain(scope, cin, widths, form, seed):
    """Layers + parameters + moving statistics; gamma = 0.2 + 0.3 randn (signed) with every 7th channel exactly 0."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    layers, params, stats = [], {}, {}
    for i, (co, (bn, relu)) in enumerate(zip(widths, form)):
        name = "%s/conv%d" % (scope, i)
        layers.append(L(name, bn, relu))
        params[name + "/W"] = (rnd(cin, co) * (2.0 / cin) ** 0.5).float().numpy()
        params[name + "/b"] = (rnd(co) * 0.1).float().numpy()
        if bn:
            gamma = 0.2 + 0.3 * rnd(co)
            gamma[::7] = 0.0
            gamma[1] = -gamma[1].abs() - 0.05  # (a narrow layer may draw no negative channel)
            assert bool((gamma < 0).any()) and bool((gamma == 0).any()) and bool((gamma > 0).any())
            params[name + "/gamma"] = gamma.float().numpy()
            params[name + "/beta"] = (rnd(co) * 0.1).float().numpy()
            stats[name] = ((rnd(co) * 0.5).float().numpy(), (0.5 + 1.5 * torch.rand(co, generator=g, dtype=torch.float64)).float().numpy())
        cin = co
    return layers, params, stats


def cloud(seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, N, 3, generator=g).numpy()
    pts = torch.randn(B, N, CIN, generator=g).numpy()
    fps_idx = torch.stack([torch.randperm(N, generator=g)[:M_] for _ in range(B)]).numpy().astype(np.int32)
    idx = torch.randint(0, N, (B, M_, K), generator=g).numpy().astype(np.int32)
    idx[:, :, 5:] = idx[:, :, :1]  # a ball query's padding: the first hit repeated
    return xyz, pts, fps_idx, idx


def torch_chain(x, layers, params, stats, mode):
    """Route 1: torch's own batch_norm in float64."""
    F = torch.nn.functional
    for Lr in layers:
        z = x @ R.f64(params[Lr.name + "/W"]) + R.f64(params[Lr.name + "/b"])
        if Lr.bn:
            if mode == "moving":
                z = F.batch_norm(z, R.f64(stats[Lr.name][0]), R.f64(stats[Lr.name][1]), R.f64(params[Lr.name + "/gamma"]),
                                 R.f64(params[Lr.name + "/beta"]), training=False, eps=1e-5)
            else:
                z = F.batch_norm(z, None, None, R.f64(params[Lr.name + "/gamma"]), R.f64(params[Lr.name + "/beta"]), training=True, eps=1e-5)
        x = F.relu(z) if Lr.relu else z
    return x


def oracle_chain(O, x, layers, params, stats, mode, k=None):
    """Route 2: tests/test_gpu_model.py:oracle_chain with the GIVEN mean / var in moving mode."""
    for Lr in layers:
        z = O.linear(x, params[Lr.name + "/W"], params[Lr.name + "/b"])
        if Lr.bn:
            mean, var = stats[Lr.name] if mode == "moving" else O.bn_stats(z)
            x = O.bn_relu(z, mean, var, params[Lr.name + "/gamma"], params[Lr.name + "/beta"], relu=Lr.relu)
        else:
            x = z
    return O.max_over_k(x, k) if k else x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", sorted(CHAINS))
def test_chain_layer_by_layer_vs_torch_batch_norm(form, mode):
    """Every prefix of the chain (so a failure names the layer), on the grouped rows of a small cloud, to float64 round-off; and the
    statistics chain_ref reports are torch's mean / unbiased variance of that layer's z."""
    layers, params, stats = make_chain("t", 3 + CIN, WIDTHS, CHAINS[form], 11)
    xyz, pts, fps_idx, idx = cloud(5)
    _, rows = R.group_rows(R.f64(xyz), R.f64(pts), R.i64(fps_idx), R.i64(idx))
    x = rows.reshape(B * M_ * K, -1)
    assert x.shape == (96, 6)
    for n in range(1, len(layers) + 1):
        bn = {}
        got = R.chain_ref(x, layers[:n], params, stats, mode, bn)
        want = torch_chain(x, layers[:n], params, stats, mode)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (form, mode, n)
        if layers[n - 1].bn:
            zin = torch_chain(x, layers[:n - 1], params, stats, mode) if n > 1 else x
            z = zin @ R.f64(params[layers[n - 1].name + "/W"]) + R.f64(params[layers[n - 1].name + "/b"])
            rec = bn[layers[n - 1].name]
            assert rec["rows"] == 96
            assert torch.allclose(rec["mean"], z.mean(0), rtol=1e-12, atol=1e-14)
            assert torch.allclose(rec["var_unbiased"], z.var(0, unbiased=True), rtol=1e-12, atol=1e-14)
            assert torch.allclose(rec["var"], z.var(0, unbiased=False), rtol=1e-12, atol=1e-14)
            assert torch.allclose(rec["zmin"], z.amin(0), rtol=1e-12, atol=1e-14) and torch.allclose(rec["zmax"], z.amax(0), rtol=1e-12, atol=1e-14)
    # the two modes are different functions of these inputs (a reference that ignored `mode` would pass both routes)
    a, b = (R.chain_ref(x, layers, params, stats, m) for m in MODES)
    assert float((a - b).abs().max()) > 1e-2


def test_zero_and_negative_gamma_channels_by_hand():
    """gamma = 0: the channel is beta whatever z is; gamma < 0: the normalised z mirrored about beta."""
    name = "t/conv0"
    x = torch.randn(96, 6, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    W = torch.randn(6, 4, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    W[:, 2] = W[:, 1]  # channels 1 and 2: the same z, gamma -1 and +1
    params = {name + "/W": W.numpy(), name + "/b": np.zeros(4), name + "/gamma": np.array([0.0, -1.0, 1.0, -0.5]),
              name + "/beta": np.array([0.3, 0.0, 0.0, -0.2])}
    stats = {name: (np.array([0.1, 0.2, 0.2, 0.0]), np.array([1.0, 2.0, 2.0, 0.5]))}
    y = R.chain_ref(x, [L(name, True, False)], params, stats, "moving")
    assert bool((y[:, 0] == 0.3).all())
    assert torch.allclose(y[:, 1], -y[:, 2], rtol=0, atol=1e-15)
    z3 = (x @ W)[:, 3]
    assert torch.allclose(y[:, 3], -0.5 * z3 / np.sqrt(0.5 + 1e-5) - 0.2, rtol=1e-14, atol=1e-15)
    with pytest.raises(ValueError):
        R.chain_ref(x, [L(name, True, False)], params, stats, "frozen")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", sorted(CHAINS))
def test_sa_and_fp_modules_vs_the_oracle(O, form, mode):
    """sa_ref (with and without mlp2 behind the pool) and fp_ref against O.group_concat / O.linear / O.bn_relu / O.max_over_k /
    O.three_interpolate at the oracle's fp32 storage class: 1e-5 of max(1, max |ref|)."""
    xyz, pts, fps_idx, idx = cloud(6)
    layers, params, stats = make_chain("sa", 3 + CIN, WIDTHS, CHAINS[form], 12)
    post, p2, s2 = make_chain("post", WIDTHS[-1], (16, 6), [(True, True), (False, False)], 13)
    params.update(p2), stats.update(s2)
    new_xyz = O.gather_point(xyz, fps_idx)
    g = O.group_concat(xyz, new_xyz, pts, idx).reshape(-1, 3 + CIN)
    pooled = oracle_chain(O, g, layers, params, stats, mode, K)
    for pst, want in ((None, pooled), (post, oracle_chain(O, pooled, post, params, stats, mode))):
        rx, got = R.sa_ref(layers, params, stats, mode, R.f64(xyz), R.f64(pts), R.i64(fps_idx), R.i64(idx), post=pst)
        assert np.array_equal(rx.numpy(), new_xyz.astype(np.float64))
        e = R.relerr(got.reshape(B * M_, -1), want)
        assert e < 1e-5, (form, mode, pst is not None, e)
    # feature propagation: three taps x weights of a coarser level, concat with the finer level's own features
    gq = torch.Generator().manual_seed(7)
    p2f = torch.randn(B, 9, 5, generator=gq).numpy()
    tap = torch.randint(0, 9, (B, N, 3), generator=gq).numpy().astype(np.int32)
    w = torch.rand(B, N, 3, generator=gq)
    w = (w / w.sum(2, keepdim=True)).numpy()
    fl, fpar, fst = make_chain("fp", 5 + CIN, (16, 32), CHAINS[form][1:], 14)
    x = np.concatenate([O.three_interpolate(p2f, tap, w), pts], 2).reshape(B * N, -1)
    want = oracle_chain(O, x, fl, fpar, fst, mode)
    got = R.fp_ref(fl, fpar, fst, mode, R.f64(pts), R.f64(p2f), R.i64(tap), R.f64(w))
    e = R.relerr(got.reshape(B * N, -1), want)
    assert e < 1e-5, (form, mode, e)


def test_forward_ref_wires_the_stack_as_the_oracle_composition(O):
    """forward_ref on a miniature stack (the module order, fp1 <- (l3, l4), fp2 <- (l2, fp1), seeds = l2, the voting residual, the
    proposal module on the votes with mlp2) against the same modules composed by hand on the oracle, moving mode, signed gammas."""
    g = torch.Generator().manual_seed(21)
    n, ms, k, c = 64, (32, 16, 8, 4), 4, 8
    x = torch.rand(B, n, 3, generator=g).numpy()
    stack, params, stats, geo = {}, {}, {}, {}
    cin, npts = 3, n
    for i, m in enumerate(ms, 1):
        name = "sa%d" % i
        stack[name], p, s = make_chain(name, 3 + cin, (8, 8, c), CHAINS["bn_relu"], 30 + i)
        params.update(p), stats.update(s)
        geo[name] = dict(fps_idx=torch.stack([torch.randperm(npts, generator=g)[:m] for _ in range(B)]).numpy(),
                         idx=torch.randint(0, npts, (B, m, k), generator=g).numpy())
        cin, npts = c, m
    for name, n1, n2 in (("fp1", ms[2], ms[3]), ("fp2", ms[1], ms[2])):
        stack[name], p, s = make_chain(name, 2 * c, (8, c), CHAINS["bn_relu"][:2], 40 + n1)
        params.update(p), stats.update(s)
        w = torch.rand(B, n1, 3, generator=g)
        geo[name] = dict(idx=torch.randint(0, n2, (B, n1, 3), generator=g).numpy(), weight=(w / w.sum(2, keepdim=True)).numpy())
    stack["voting"], p, s = make_chain("voting", 3 + c, (8, 8, 3 + c), CHAINS["plain_last"], 50)
    params.update(p), stats.update(s)
    stack["proposal"], p, s = make_chain("proposal", 3 + c, (8, 8, 8), CHAINS["bn_relu"], 51)
    params.update(p), stats.update(s)
    stack["proposal_post"], p, s = make_chain("proposal_post", 8, (8, 8, 5), CHAINS["plain_last"], 52)
    params.update(p), stats.update(s)
    seen = []

    def proposal_geometry(votes_xyz):
        seen.append(tuple(votes_xyz.shape))
        return dict(fps_idx=np.tile(np.arange(4), (B, 1)), idx=geo["sa4"]["idx"] % ms[1])
    geo["proposal"] = proposal_geometry
    out, bn = R.forward_ref(params, stats, geo, x, "moving", stack=stack)
    assert seen == [(B, ms[1], 3)] and len(bn) == 4 * 3 + 2 * 2 + 2 + 3 + 2

    def o_sa(name, xyz, pts, gm, post=None):
        new_xyz = O.gather_point(xyz, gm["fps_idx"].astype(np.int32))
        rows = O.group_concat(xyz, new_xyz, pts, gm["idx"].astype(np.int32))
        y = oracle_chain(O, rows.reshape(-1, rows.shape[-1]), stack[name], params, stats, "moving", gm["idx"].shape[2])
        if post:
            y = oracle_chain(O, y, stack[post], params, stats, "moving")
        return new_xyz, y.reshape(B, gm["idx"].shape[1], -1)

    def o_fp(name, p1, p2):
        itp = O.three_interpolate(p2, geo[name]["idx"].astype(np.int32), geo[name]["weight"])
        xx = np.concatenate([itp, p1], 2)
        return oracle_chain(O, xx.reshape(-1, xx.shape[2]), stack[name], params, stats, "moving").reshape(B, p1.shape[1], -1)
    r = {}
    xyz, pts = x, x
    for i in range(1, 5):
        xyz, pts = o_sa("sa%d" % i, xyz, pts, geo["sa%d" % i])
        r["l%d_xyz" % i], r["l%d_p" % i] = xyz, pts
    r["l3_p2"] = o_fp("fp1", r["l3_p"], r["l4_p"])
    r["seeds_points"] = o_fp("fp2", r["l2_p"], r["l3_p2"])
    xx = np.concatenate([r["l2_xyz"], r["seeds_points"]], 2).reshape(-1, 3 + c)
    votes = (xx + oracle_chain(O, xx, stack["voting"], params, stats, "moving")).reshape(B, ms[1], -1)
    r["votes_xyz"], r["votes_points"] = votes[..., :3], votes[..., 3:]
    r["proposals_xyz"], r["proposals_output"] = o_sa("proposal", np.ascontiguousarray(r["votes_xyz"]), np.ascontiguousarray(r["votes_points"]),
                                                     proposal_geometry(torch.zeros(B, ms[1], 3)), post="proposal_post")
    assert torch.equal(out["seeds_xyz"], out["l2_xyz"])
    for key, want in r.items():
        e = R.relerr(out[key], want)
        assert e < 1e-5, (key, e)


def test_the_stack_names_the_23_batchnorm_layers():
    names = R.bn_layer_names()
    assert len(names) == 23 and len(set(names)) == 23
    assert names[:3] == ["sa1/conv0", "sa1/conv1", "sa1/conv2"] and "fp1/conv_1" in names and "voting/fc1" in names
    assert "voting/fc2" not in names and "proposal/conv_post_2" not in names and names[-1] == "proposal/conv_post_1"


def test_moving_error_is_the_bar_shape_on_the_normalised_output():
    """moving_error against the normalised outputs written out row by row."""
    g = torch.Generator().manual_seed(4)
    z = torch.randn(200, 5, generator=g, dtype=torch.float64) * 3 + 1
    gamma, beta = torch.tensor([0.0, -0.7, 1.2, 0.3, -0.1], dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
    want = (torch.randn(5, generator=g, dtype=torch.float64), torch.rand(5, generator=g, dtype=torch.float64) + 0.5)
    got = (want[0] + 1e-3, want[1] * 1.01)
    a = lambda s: gamma * (z - s[0]) / torch.sqrt(s[1] + R.BN_EPS) + beta
    rec = dict(zmin=z.amin(0), zmax=z.amax(0))
    e = float((a(got) - a(want)).abs().max()) / max(1.0, float(a(want).abs().max()))
    assert abs(R.moving_error(rec, gamma, beta, got, want) - e) < 1e-14
    assert R.moving_error(rec, gamma, beta, want, want) == 0.0
