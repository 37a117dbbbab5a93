"""CPU: tests/bn_stats_ref.py checks itself -- the float64 reference against numpy and the oracle, the weighted form against repeated
rows, the emulation against a plain loop -- and checks, on the very inputs tests/test_gpu_bn_stats.py launches, what its bars rest on:
every builder reaches the |mean| / std it claims inside the fp16 x 2 operand range, and the model of the epilogues' accumulation stays
a factor of four under the bar wherever the bar is asserted of an input-sourced case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_stats_ref as B  # noqa: E402

_inputs = {}


def inputs(case, source):
    key = (case, source)
    if key not in _inputs:
        _inputs[key] = B.host_inputs(case, source)
    return _inputs[key]


def test_reference_against_numpy_and_the_oracle(O):
    rng = np.random.default_rng(0)
    z = (rng.normal(size=(777, 13)) * rng.uniform(0.1, 30, 13) + rng.normal(size=13) * 50).astype(np.float32)
    mean, var, n = B.reference(z)
    assert n == 777
    assert np.allclose(mean, z.astype(np.float64).mean(0), rtol=1e-14, atol=0) and np.allclose(var, np.var(z.astype(np.float64), axis=0), rtol=1e-12)
    omean, ovar = O.bn_stats(z)
    assert np.allclose(omean, mean, rtol=1e-6, atol=1e-6) and np.allclose(ovar, var, rtol=1e-5, atol=1e-6)  # fp32 results of the oracle


def test_weighted_reference_equals_repeated_rows():
    rng = np.random.default_rng(1)
    z = rng.normal(3.0, 2.0, (96, 5))
    w = np.ones(96)
    w[::16] = 1 + 16 * rng.integers(0, 4, 6)
    rep = np.repeat(z, w.astype(int), 0)
    m1, v1, n1 = B.reference(z, w)
    m2, v2, n2 = B.reference(rep)
    assert n1 == n2 == rep.shape[0] and np.allclose(m1, m2, rtol=1e-13) and np.allclose(v1, v2, rtol=1e-12)
    # ... and the restated piece weights: one piece of 4 kept -> its head stands for 49 rows; all kept -> every row for itself
    assert B.piece_weights(np.array([5, 64], np.int32)).tolist() == [49.0] + [1.0] * 15 + [1.0] * 16 + [1.0] * 48
    for kind, rows in (("mixed", 384), ("full", 512), ("one", 256), ("device", 2048), ("mixed", 2048)):
        cnt, pieces, _ = B.piece_layout(kind, rows)
        assert int((-(-cnt // 16)).sum()) == pieces and pieces % 8 == 0 and len(cnt) % 8 == 0
        assert B.piece_weights(cnt).sum() == 64 * len(cnt)


@pytest.mark.parametrize("pivot", [False, True])
def test_emulation_equals_a_plain_loop(pivot):
    rng = np.random.default_rng(2)
    z = rng.normal(7.0, 1.0, (41, 2)).astype(np.float32)  # 41 rows: the last lane runs short, the last wave group is not full
    z[:16] = rng.normal(7.0, 0.3, (16, 2)).astype(np.float32)  # (the first group of four lanes: |mean| above 8 std)
    L, waves = 4, 4
    s1, s2 = B.emulate(z, L, waves, pivot)
    for ch in range(2):
        lanes = []
        for lo in range(0, 41, L):
            run = z[lo:lo + L, ch]
            c = np.array([run[0]]).view(np.uint32) & np.uint32(0xffff0000)
            c = c.view(np.float32)[0] if pivot else np.float32(0)
            a1 = a2 = np.float32(0)
            for v in run:
                d = np.float32(v - c)
                a1 = np.float32(a1 + d)
                a2 = np.float32(a2 + np.float32(d * d))
            lanes.append((a1, a2, float(c), len(run)))
        if pivot:  # four lanes are added in double; their two sums are cut to 36 bits where the |mean| of their rows is 8 std or more,
            #         else to 24 (z is built so that both happen)
            def cut(t, long_):
                return t * 131073.0 - (t * 131073.0 - t) if long_ else float(np.float32(t))
            e1 = e2 = 0.0
            rule = []
            for g in range(0, len(lanes), waves):
                t1 = sum(float(a1) + n * c for a1, a2, c, n in lanes[g:g + waves])
                t2 = sum(float(a2) + 2.0 * c * float(a1) + n * c * c for a1, a2, c, n in lanes[g:g + waves])
                n = sum(n for _, _, _, n in lanes[g:g + waves])
                rule.append(t1 * t1 >= 64.0 * (n * t2 - t1 * t1))
                e1, e2 = e1 + cut(t1, rule[-1]), e2 + cut(t2, rule[-1])
            assert any(rule) and not all(rule)
        else:
            e1 = e2 = 0.0
            for g in range(0, len(lanes), waves):
                w1 = w2 = np.float32(0)
                for a1, a2, _, _ in lanes[g:g + waves]:
                    w1, w2 = np.float32(w1 + a1), np.float32(w2 + a2)
                e1, e2 = e1 + float(w1), e2 + float(w2)
        assert np.isclose(s1[ch], e1, rtol=1e-15, atol=0) and np.isclose(s2[ch], e2, rtol=1e-15, atol=0)
    # the model is a model of fp32: it differs from the float64 sums, by fp32 rounding
    z64 = z.astype(np.float64)
    assert 0 < np.abs(s2 / (z64 * z64).sum(0) - 1).max() < 1e-5 or pivot


def test_finalize_model_clamps_and_rounds_once():
    sc, sh, mean, var = B.finalize(np.array([300.0, 3.0]), np.array([900.0 * (1 - 1e-13), 0.09]), 100,  # a negative difference, a zero one
                                   np.ones(2, np.float32),
                                   np.zeros(2, np.float32))
    assert var[0] == 0 and var[1] == 0 and np.all(sc == np.float32(1) / np.sqrt(np.float32(B.BN_EPS))) and np.all(np.isfinite(sh))


def test_the_unpivoted_table_has_the_shape_the_design_section_prints():
    """Without a pivot the error grows with r (as 1 + r^2 in the variance) and with L; with it, it does not."""
    rows = 4096
    e32 = [B.table_e(rows, r, 32) for r in (3, 10, 30)]
    assert e32[0] < e32[1] < e32[2] and B.table_e(rows, 30, 1024) > e32[2]
    z = np.stack([np.random.default_rng(1000 + s).normal(30.0, 1.0, rows) for s in range(B.SEEDS)], 1)
    assert B.emulated_e(z, 1024, pivot=True).max() < B.CONDITION < B.table_e(rows, 30, 1024)


CASE_SOURCES = [(c, s) for c in B.CASES for s in B.sources_of(c)]


@pytest.mark.parametrize("case,source", CASE_SOURCES, ids=[B.case_id(c, s, B.lane_run(c)[0]) for c, s in CASE_SOURCES])
def test_builders_reach_their_r_inside_the_operand_range(case, source):
    d = inputs(case, source)
    assert float(d["act"].abs().max()) < B.ACT_LIMIT and float(d["w"].abs().max()) < B.W_LIMIT
    if d["valid"] == 1:
        return
    got, want = B.measured_r(d["z64"], d["cols"], d["weights"])
    assert len(got) and np.all(np.abs(got - want) <= 0.1 * np.maximum(want, 1.0)), (got, want)  # r = 0: |r| <= 0.1
    sd = np.sqrt(B.reference(d["z64"], d["weights"])[1])
    for j, col in enumerate(d["cols"]):
        if col.kind in B.CONST_VALUE:
            assert sd[j] == 0
        else:
            assert abs(sd[j] / col.sigma - 1) < 5e-2  # (over a grouping the three offset rows add a little)
    if source == "input":  # one sign per column -- but the r = 0 column and, over a grouping, the three offset rows
        w = d["w"].numpy()[3:] if B.opt(case, "geom") else d["w"].numpy()
        for j, col in enumerate(d["cols"]):
            if col.kind == "r" and col.r > 0:
                assert (w[:, j] >= 0).all() or (w[:, j] <= 0).all()
    kinds = set((c.kind, c.r, c.sigma) for c in d["cols"])
    assert ("r", 3, 1e-3) in kinds and (("r", 3, 30) in kinds or case.cout < 8)  # (5 x 3 x 7: seven columns)
    assert ("const", 0, 0) in kinds or B.opt(case, "small_bias")
    assert ("constg", 0, 0) in kinds or case.cout < 9 or (source == "input" and not B.opt(case, "small_bias"))


@pytest.mark.parametrize("case", B.CASES, ids=[B.case_id(c, "input", B.lane_run(c)[0]) for c in B.CASES])
def test_conditions_of_the_tier_a_bars(case, capsys):
    """Every input-sourced column the GPU test holds to the bar: the model of the accumulation (fp32 lane runs about a pivot, double
    from there on; four waves) on the case's own z, at the case's L, gives e <= 2.5e-6."""
    d = inputs(case, "input")
    if d["valid"] == 1:
        return
    L = B.lane_run(case)[0]
    z = d["z64"].astype(np.float32)
    if d["weights"] is not None:
        z = np.repeat(z, d["weights"].astype(int), 0)
    g, be = d["gamma"].numpy(), d["beta"].numpy()
    if case.producer in B.DOUBLE_PRODUCERS:  # their sums are formed in double from moments: exact sums stand for them
        z64 = z.astype(np.float64)
        sums = z64.sum(0), (z64 * z64).sum(0)
    else:
        sums = B.emulate(z, L, 4, True)
    sc, sh, _, _ = B.finalize(*sums, z.shape[0], g, be)
    e = B.metric(z, sc, sh, g, be)["e"]
    held = [j for j, col in enumerate(d["cols"]) if B.tier_of(case, "input", col, L) == "A"]
    with capsys.disabled():
        worst = {}
        for j in held:
            worst[d["cols"][j].r] = max(worst.get(d["cols"][j].r, 0.0), float(e[j]))
        print("\n  emulated e, %s: %s" % (B.case_id(case, "input", L), "  ".join("r=%g %.1e" % kv for kv in sorted(worst.items()))), end="")
    assert held or L > 256
    # r = 300 (the double-precision producers alone are held to the bar there): shift ~ -300 gamma is an fp32 number, and half an ulp
    # of it -- 1.5e-5 over max |a| ~ 6 -- is 2.5e-6 by itself, whatever the sums are.  That share is allowed beside the condition.
    mean, var, _ = B.reference(z)
    den = max(1.0, float(np.abs(g * (z - mean) / np.sqrt(var + B.BN_EPS) + be).max()))
    bound = [B.CONDITION + (0.5 * float(np.spacing(np.abs(sh[j]))) / den if d["cols"][j].r > 100 else 0.0) for j in range(len(e))]
    assert all(e[j] <= bound[j] for j in held), [(d["cols"][j].r, float(e[j])) for j in held if e[j] > bound[j]]


def test_every_producer_keeps_a_walked_and_an_unwalked_case():
    for producer in B.FAST_PRODUCERS:
        assert any(c.producer == producer and c.gx is None for c in B.CASES) and any(c.producer == producer and c.gx is not None for c in B.CASES)
    walks = {B.case_id(c, "", 0): B.lane_run(c) for c in B.CASES}
    assert sorted(set(v[1] for v in walks.values())) == ["2x2", "4x1", "few", "fp32", "rows"]
    assert max(v[0] for v in walks.values()) == 1024 and sum(v[0] == 1024 for v in walks.values()) == 1  # the one Tier B walk of 32 tiles
    assert all(v[0] <= 256 for k, v in walks.items() if v[0] != 1024)
