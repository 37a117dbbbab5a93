"""GPU: the BatchNorm batch statistics of every producer against float64, at |mean| / std ratios r the other tests never reach.

Every producer of the raw sums (sum z, sum z^2) is launched through its Python entry of votenet_amd/mlp.py on the inputs of
tests/bn_stats_ref.py (CASES: columns of r = 0 ... 300 mixed in one launch, a constant channel, channels of magnitude 1e-3 and 30), the
sums are finalized on the device, and the recorded fp32 scale / shift are held to the float64 BatchNorm of the same z:

    e = max |z scale + shift - (gamma (z - mean) / sqrt(var + eps) + beta)| / max(1, max |a_ref|)          (bn_stats_ref.metric)

The reference is taken from the device's STORED z wherever the producer stores it (the GEMM's own rounding stays out); from a float64
recomputation from the inputs where it does not -- linear_dense_pool(keep_z=False) and the never-stored first layers (assembled,
narrow): the printed line of a case says which.  Tier A columns: e <= 1e-5, the project's bar.  Tier B columns (input-sourced r of 30
and 100; every r in the one launch whose single workgroup walks 32 tiles): e <= the smaller of the bar and 4 x the maximum the
unpivoted emulation of bn_stats_ref gives over its eight seeds at the same (rows, r, L); at the shapes here that is the bar.  The
fast-path producers run with one tile per workgroup and WALKED under a workgroup cap (the `walk` fixture of
tests/test_gpu_tile_walk.py); L in a test's id is the longest fp32 run of a lane.  Input-sourced r also runs beside a small random
bias (small_bias: the packed epilogues carry the pivot in the bias).  Every case is launched twice and its sums compared bit for bit.
Not reached here: a workgroup of csrc/mlp.hip that walks more than one tile (it takes more than 1024 / ny tiles, 131072 rows), and
more than 16 rows per thread of group_linear (4096 workgroups' worth): their pivot is set once per lane / thread, as in the fast path,
whose walks are run.  Run with -s for the measured e of every case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_stats_ref as B  # noqa: E402
from test_gpu_tile_walk import images, walk  # noqa: E402,F401  (the fixture, by import)

pytestmark = pytest.mark.gpu

_inputs = {}


def inputs(case, source):
    """Host inputs once per (case, source); nothing writes them."""
    key = (case, source)
    if key not in _inputs:
        _inputs[key] = B.host_inputs(case, source)
    return _inputs[key]


def ids_of(cases):
    return [B.case_id(c, s, B.lane_run(c)[0]) for c, s in cases]


FAST = [(c, s) for c in B.CASES if c.producer in B.FAST_PRODUCERS for s in B.sources_of(c)]
OTHER = [(c, s) for c in B.CASES if c.producer not in B.FAST_PRODUCERS for s in B.sources_of(c)]


def pending_input_bn(M, d, rows, dev):
    """The BatchNorm folded into the load as a PendingBN: raw sums (0, rows) are mean 0 and variance 1 -> scale = gamma0 / sqrt(1 + eps),
    shift = beta0.  -> (PendingBN or None, check()): check() holds the consumer-side finalize (csrc/common.h) to bn_finalize."""
    if "gamma0" not in d:
        return None, lambda: None
    cin = d["gamma0"].shape[0]
    st0 = torch.cat([torch.zeros(cin, dtype=torch.float64), torch.full((cin,), float(rows), dtype=torch.float64)]).to(dev)
    g0, b0 = d["gamma0"].to(dev), d["beta0"].to(dev)
    pend = M.PendingBN(st0, g0, b0, rows)

    def check():
        assert pend.done
        for got, exp in zip(pend.out, M.bn_finalize(rows, st0, g0, b0)):
            assert torch.equal(got, exp)
    return pend, check


def launch(M, dev, case, d, gemm_form):
    """-> (z the reference is taken from (numpy float64), which reference, stats, n, recorded (scale, shift, mean, var) or None)."""
    rows, cin, cout = case.rows, case.cin, case.cout
    T = lambda t: None if t is None else t.to(dev)
    w, bias, gamma, beta = T(d["w"]), T(d["bias"]), T(d["gamma"]), T(d["beta"])
    p = case.producer
    if p in ("dense_fp32", "dense", "pool", "pieces"):
        x = T(d["x"])
        in_bn, check_in = pending_input_bn(M, d, rows, dev)
        img = images(M, [w], gemm_form, True) if gemm_form is not None else None
        prev = M.set_deterministic(True) if B.opt(case, "deterministic") else None
        try:
            if p == "pool":
                z, st, _ = M.linear_dense_pool(x, w, 64, bias, in_bn=in_bn, keep_z=B.opt(case, "keep_z"))
            elif p == "pieces":
                cnt = torch.from_numpy(d["cnt"]).to(dev).view(1, -1)
                half = M.half_groups(cnt, device_count=d["device_count"]).resolve()
                assert half.true_count() == d["pieces"] and half.rows == rows
                wts = torch.ones(d["valid"], device=dev)
                wts[::16] = half.wh[:d["pieces"]]
                assert np.array_equal(wts.cpu().numpy(), d["weights"])  # the layout restated on the host is the device's
                z, st, _ = M.linear_dense_pool(x, w, 64, bias, in_bn=in_bn, keep_z=True, half=half, gamma=gamma)
                assert bool(torch.isnan(z[d["valid"]:]).all())  # rows past the count are nobody's to write
            else:
                assert M.split_eligible(cin, cout) and rows % 128 == 0 if p == "dense" else not (rows % 128 == 0 and cout % 64 == 0)
                z, st = M.linear_dense(x, w, bias, in_bn=in_bn)
        finally:
            if prev is not None:
                M.set_deterministic(prev)
            if img is not None:
                img.close()
        check_in()
        if z is None:
            return d["z64"], "inputs", st, d["n"], None
        return z[:d["valid"]].double().cpu().numpy(), "stored z", st, d["n"], None
    xyz, new_xyz, idx, feat = T(d["xyz"]), T(d["new_xyz"]), T(d["idx"]), T(d["feat"])
    b, n, m, k = B.opt(case, "geom")
    if p == "gather":
        z, st = M.linear_gather(xyz, new_xyz, feat, idx, w, bias)
        return z.double().cpu().numpy(), "stored z", st, rows, None
    if p == "group_linear":
        P = (d["feat"].double().reshape(b * n, cin - 3) @ d["w"][3:].double()).float().reshape(b, n, cout).to(dev)
        z, st = M.group_linear(xyz, new_xyz, idx, P, w[:3].contiguous(), bias)
        return z.double().cpu().numpy(), "stored z", st, rows, None
    # the never-stored first layers: statistics in double from moments, finalized in the prologue of the second layer's fused GEMM
    g1 = torch.Generator().manual_seed(rows + cout)
    w1 = (torch.randn(cout, B.C1, generator=g1) * 0.2).to(dev)
    img = images(M, [w1], gemm_form, True)
    try:
        if p == "assembled":
            assert M.assembled_supported(rows, cout, B.C1)
            P, _ = M.linear_dense(feat.reshape(b * n, cin - 3), w[3:].contiguous(), bias, want_stats=False)  # the per-point table, bias inside
            wx = w[:3].contiguous()
            geo, cntv, mom = M.assemble_rows(xyz, new_xyz, idx)
            st = M.assemble_stats(P, cntv, wx, mom)
            bn0 = M.PendingBN(st, gamma, beta, rows)
            M.assembled_linear(geo, P, wx, w1, None, bn0)
            dx = geo[:, :3].double()
            z0 = P[T(d["prow"])].double() + dx @ wx.double()
        else:
            assert M.narrow_supported(rows, cin, cout, B.C1)
            b0 = bias if bias is not None else torch.zeros(cout, device=dev)
            u8, mom = M.narrow_rows(xyz, new_xyz, feat, idx)
            st = M.narrow_stats(rows, mom, w, b0)
            bn0 = M.PendingBN(st, gamma, beta, rows)
            M.narrow_linear(u8, w, b0, w1, None, bn0)
            z0 = u8[:, :cin].double() @ w.double() + b0.double()
    finally:
        img.close()
    assert bn0.done
    return z0.cpu().numpy(), "inputs", st, rows, tuple(t.clone() for t in bn0.out)


def check(M, dev, case, source, L, d, zref, which, st, n, recorded, gemm_form):
    gamma, beta = d["gamma"].to(dev), d["beta"].to(dev)
    cols = d["cols"]
    cout = case.cout
    sc, sh, mean, var = M.bn_finalize(n, st, gamma, beta)
    if recorded is not None:  # what the consumer's prologue recorded is what the stand-alone kernel gives
        for got, exp in zip(recorded, (sc, sh, mean, var)):
            assert torch.equal(got, exp)
    # a second consumer-side finalize of the SAME sums: the activation pass
    pend = M.PendingBN(st, gamma, beta, n)
    M.bn_relu(torch.zeros(8, cout, device=dev), None, None, True, bn=pend)
    for got, exp in zip(pend.out, (sc, sh, mean, var)):
        assert torch.equal(got, exp)
    sc, sh, mean, var = (t.cpu() for t in (sc, sh, mean, var))
    g32, b32 = d["gamma"], d["beta"]
    for t in (sc, sh, mean, var):
        assert bool(torch.isfinite(t).all())
    assert bool((var >= 0).all())
    # the recorded mean and variance are what scale and shift were derived from: scale exactly; shift = beta - mean scale was formed
    # from the double mean and rounded once, so it sits within half an ulp of itself plus |scale| times half an ulp of the fp32 mean
    eps32 = torch.tensor(B.BN_EPS, dtype=torch.float32)
    want_sc = (g32 / torch.sqrt(var + eps32)).numpy()  # (the device's fp32 square root and division: within an ulp or two of the host's)
    assert np.all(np.abs(sc.numpy() - want_sc) <= 2 * np.spacing(np.abs(want_sc)))
    slack = 0.5 * np.spacing(np.abs(sh.numpy())).astype(np.float64) + np.abs(sc.numpy()).astype(np.float64) * 0.5 * np.spacing(np.abs(mean.numpy())).astype(np.float64)
    assert np.all(np.abs(sh.numpy().astype(np.float64) - (b32.numpy().astype(np.float64) - mean.numpy().astype(np.float64) * sc.numpy().astype(np.float64))) <= slack)
    m = B.metric(zref, sc.numpy(), sh.numpy(), g32.numpy(), b32.numpy(), d["weights"])
    var_rel, mstd = B.recorded_errors(mean.numpy(), var.numpy(), zref, d["weights"])
    worst = {}
    for j, col in enumerate(cols):
        tier = B.tier_of(case, source, col, L)
        if tier == "exact":  # a constant channel that eight bits hold (every channel of a one-row launch: var is zeroed there)
            assert float(var[j]) == 0.0, (j, float(var[j]))  # (scale = gamma / sqrt(eps) then follows from the line above)
            continue
        if tier == "near":  # a constant the pivot does not hold: the fp32 partials carry n (z - c) and its ROUNDED squares, and the
            # workgroup's sums are cut to 36 bits, so the double subtraction leaves up to 2^-36-odd of mean^2 (or clamps): exact zero is
            # not attainable; 1e-9 mean^2 is 2^-30, and at eps = 1e-5 it moves scale by less than an fp32 ulp for |z| < 30
            assert 0.0 <= float(var[j]) <= 1e-9 * float(mean[j]) ** 2, (j, float(var[j]), float(mean[j]))
            continue
        key = (tier, col.r, col.sigma)
        worst[key] = max(worst.get(key, (0.0, 0.0, 0.0)), (float(m["e"][j]), float(var_rel[j]), float(mstd[j])))
        if tier == "A":
            assert m["e"][j] <= B.BAR, (j, col, float(m["e"][j]))
        elif tier == "B":
            bar = min(B.BAR, 4.0 * B.table_e(d["valid"], col.r, L))
            assert m["e"][j] <= bar, (j, col, float(m["e"][j]), bar)
    print("\nBNSTAT %s form=%s ref=%s |" % (B.case_id(case, source, L), {None: "-", 0: "fp32", 1: "bf16x3", 2: "fp16x2"}[gemm_form],
                                         which), "  ".join("%s r=%g s=%g e=%.1e var=%.1e m/s=%.1e" % (k + v) for k, v in sorted(worst.items(), key=str)), end="")


def launch_twice(M, dev, case, d, gemm_form):
    """Two launches of the case: the raw sums must come out bit for bit the same (what a workgroup hands to the double atomics is a
    short number, csrc/mlp_types.h stat_cut, so the sums do not depend on the order of arrival), at every r of the matrix.  What this
    does not reach is stated in DESIGN 9: a workgroup of near-constant rows far smaller in magnitude than the column's other rows."""
    first = launch(M, dev, case, d, gemm_form)
    again = launch(M, dev, case, d, gemm_form)
    if case.producer != "assembled":  # (assemble_stats adds full doubles per point with atomics, csrc/assemble.hip: not an epilogue)
        assert torch.equal(first[2], again[2])
    return first


@pytest.mark.parametrize("case,source", FAST, ids=ids_of(FAST))
def test_fast_path_producers(walk, dev, gemm_form, case, source):
    M = walk.M
    L, variant, caps = B.lane_run(case)
    d = inputs(case, source)
    walk.caps(caps[0], caps[1], 1)
    try:
        zref, which, st, n, recorded = launch_twice(M, dev, case, d, gemm_form)
    finally:
        walk.caps()
    check(M, dev, case, source, L, d, zref, which, st, n, recorded, gemm_form)


@pytest.mark.parametrize("case,source", OTHER, ids=ids_of(OTHER))
def test_producers_off_the_fast_path(walk, dev, case, source):
    """linear_dense on the fp32 MFMA kernel of csrc/mlp.hip (rows no multiple of 128, cout 7 and 79; one row), linear_gather, group_linear."""
    M = walk.M
    L = B.lane_run(case)[0]
    d = inputs(case, source)
    zref, which, st, n, recorded = launch_twice(M, dev, case, d, None)
    check(M, dev, case, source, L, d, zref, which, st, n, recorded, None)


def test_a_negative_difference_is_clamped(hiplib, dev):
    """sum z^2 / n - mean^2 below zero by rounding (a constant channel whose sums were formed in another order): var = 0 is recorded and
    scale = gamma / sqrt(eps), never a NaN -- by bn_finalize and by the consumer-side copy of csrc/common.h."""
    from votenet_amd import mlp as M
    n, c = 1000, 4
    mu = torch.tensor([300.0, -7.25, 1e-3, 0.0], dtype=torch.float64)
    s2 = n * mu * mu * torch.tensor([1 - 1e-13, 1 - 1e-15, 1 - 1e-12, 1.0], dtype=torch.float64)
    assert bool((s2 / n - mu * mu <= 0).all()) and bool((s2 / n - mu * mu < 0).any())
    st = torch.cat([n * mu, s2]).to(dev)
    gamma, beta = torch.tensor([1.5, -0.5, 1.0, 2.0], device=dev), torch.tensor([0.1, 0.2, -0.3, 0.0], device=dev)
    sc, sh, mean, var = M.bn_finalize(n, st, gamma, beta)
    pend = M.PendingBN(st, gamma, beta, n)
    M.bn_relu(torch.zeros(8, c, device=dev), None, None, True, bn=pend)
    for got, exp in zip(pend.out, (sc, sh, mean, var)):
        assert torch.equal(got, exp)
    assert bool((var == 0).all()) and bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all())
    want = (gamma.cpu() / torch.sqrt(torch.tensor(B.BN_EPS, dtype=torch.float32))).numpy()
    assert np.all(np.abs(sc.cpu().numpy() - want) <= 2 * np.spacing(np.abs(want)))  # (the device's fp32 sqrt and division)
    assert torch.equal(mean.cpu(), mu.float())
