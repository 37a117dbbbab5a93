"""CPU: the cases of the loss kernel's GPU tests (tests/loss_ref.py: shape_case at SHAPES, HAND_CASES) are sound before any device sees
them -- the float32 and the float64 run of the reference restatement take the same decisions, so a kernel that computes in float32 can
be held to the float64 result at the bar of test_gpu_loss.py, and the hand cases decide what their docstrings say."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref  # noqa: E402
from loss_cases import NAMES, SHAPES, case_ids, load_case, reference  # noqa: E402

DECISIONS = ("votes_assignment", "surface_ind", "bboxes_assignment", "positive", "negative", "dual_assignment")


def test_argmin_returns_the_first_minimum():
    """The reference restatement leans on torch.argmin for tf.argmin's first minimum, along the last axis and along axis 1."""
    for dt in (torch.float32, torch.float64):
        t = torch.tensor([[3.0, 1.0, 2.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5, 0.5]], dtype=dt)
        assert t.argmin(-1).tolist() == [1, 0]
        wide = torch.full((2, 130, 3), 7.0, dtype=dt)
        wide[0, 66, 0] = wide[0, 10, 0] = wide[1, 129, 2] = wide[1, 65, 2] = 0.25
        assert wide.argmin(1).tolist() == [[10, 0, 0], [0, 0, 65]]


@pytest.mark.parametrize("cid", case_ids())
def test_case_is_decided_alike_in_float32_and_float64(cid):
    seeds, votes, prop, out, gt, kw = load_case(cid)
    r64, g64 = reference(cid)
    T = lambda a: torch.from_numpy(a.copy())
    v, p, w = T(votes).requires_grad_(True), T(prop).requires_grad_(True), T(out).requires_grad_(True)
    r32 = loss_ref.votenet_loss(T(seeds), v, p, w, {k: T(x) for k, x in gt.items()}, **kw)
    r32["total_cost"].backward()
    assert r32["n_pos"] == r64["n_pos"] > 0 and r32["n_neg"] == r64["n_neg"] > 0
    for k in DECISIONS:
        assert torch.equal(r32[k], r64[k]), k
    for k in NAMES:
        assert abs(float(r32[k].detach()) - float(r64[k])) <= 1e-5 * max(1.0, abs(float(r64[k]))), k
    for name, g in (("votes_xyz", v.grad), ("proposals_xyz", p.grad), ("proposals_output", w.grad)):
        ref = g64[name]
        assert float((g.double() - ref).abs().max()) <= 1e-5 * max(1e-3, float(ref.abs().max())), name


@pytest.mark.parametrize("name", sorted(loss_ref.HAND_CASES))
def test_hand_case_decides_what_it_says(name):
    want = loss_ref.HAND_EXPECT[name]
    seeds, votes, prop, out, gt, kw = load_case("hand-" + name)
    assert kw.get("pos_thr", 0.3) == want.get("thr", (0.3, 0.6))[0] and kw.get("neg_thr", 0.6) == want.get("thr", (0.3, 0.6))[1]
    for a in (seeds, votes, prop, out, gt["bboxes_xyz"], gt["bboxes_lwh"], gt["heading_residuals"], gt["size_residuals"]):
        assert (a * 64 == np.round(a * 64)).all()  # multiples of 1/64
    assert (gt["bboxes_roty"] == 0).all()
    r, g = reference("hand-" + name)
    assert (r["n_pos"], r["n_neg"]) == (want["n_pos"], want["n_neg"])
    for k in DECISIONS:
        for (s, i), val in want.get(k, {}).items():
            assert r[k][s, i].item() == val, (k, s, i, r[k][s, i].item(), val)
    for cot, s, i in want.get("zero_rows", []):
        row = g["proposals_output"][s, i, 2:5] if cot == "centre" else g[cot][s, i]
        assert (row == 0).all(), (cot, s, i, row)


# ---------------------------------------------------------------- labels at or past their range (loss_ref.LABEL_CASES)
from loss_cases import label_box, label_case_ids  # noqa: E402


@pytest.mark.parametrize("base", sorted(loss_ref.LABEL_BASES))
def test_label_base_is_decided_alike_in_float32_and_float64(base):
    test_case_is_decided_alike_in_float32_and_float64("labelbase-" + base)
    (seeds, votes, prop, out, gt), (s, j) = loss_ref.label_base(base)
    r, _ = reference("labelbase-" + base)
    mine = r["positive"][s] & (r["bboxes_assignment"][s] == j)
    assert s == prop.shape[0] - 1 and int(mine.sum()) >= 2 and bool(mine[-1])  # the buffer's last row belongs to the mislabelled box
    assert int((r["positive"][s] & ~mine).sum()) >= 1 and int(r["positive"][0].sum()) >= 1  # and there are positives it must not touch


@pytest.mark.parametrize("cid", label_case_ids())
def test_label_case_reference_is_the_defined_behaviour(cid):
    """What the float64 reference says of a label outside its range, against the same case with the valid label: the class term is NaN
    and so is the cotangent of the class block of exactly the proposals assigned to that box; the residual term of those proposals is
    Huber of (0 - label residual) with no cotangent; every decision, every other loss term and every other cotangent entry is the
    valid case's."""
    s, j, field, valid = label_box(cid)
    base = "labelbase-" + loss_ref.LABEL_CASES[cid.split("-", 1)[1]][2]
    seeds, votes, prop, out, gt, kw = load_case(cid)
    _, _, _, _, gt0, _ = load_case(base)
    assert [k for k in gt if not np.array_equal(gt[k], gt0[k])] == [field]
    assert int((gt[field] != gt0[field]).sum()) == 1 and gt0[field][s, j] == valid
    bad = int(gt[field][s, j])
    assert not 0 <= bad < dict(heading_labels=12, size_labels=10, semantic_labels=10)[field]
    r, g = reference(cid)
    r0, g0 = reference(base)
    for k in DECISIONS:
        assert torch.equal(r[k], r0[k]), k
    assert (r["n_pos"], r["n_neg"]) == (r0["n_pos"], r0["n_neg"])
    for k in NAMES:
        if k in loss_ref.LABEL_NAN[field]:
            assert np.isnan(float(r[k])) and np.isfinite(float(r0[k])), k
        elif k not in loss_ref.LABEL_AFFECTS[field]:
            assert float(r[k]) == pytest.approx(float(r0[k]), rel=1e-12), k
        else:
            assert np.isfinite(float(r[k])), k
    mine = (r["positive"][s] & (r["bboxes_assignment"][s] == j)).numpy()
    cls_cols, res_cols = loss_ref.label_blocks(field, valid)
    want_nan = np.zeros(out.shape, bool)
    want_nan[s][np.ix_(mine, list(cls_cols))] = True
    gw, gw0 = g["proposals_output"].numpy(), g0["proposals_output"].numpy()
    assert np.array_equal(np.isnan(gw), want_nan)
    changed = want_nan.copy()
    if res_cols:
        changed[s][np.ix_(mine, res_cols)] = True
        assert (gw[s][np.ix_(mine, res_cols)] == 0).all() and (gw0[s][np.ix_(mine, res_cols)] != 0).all()
        # the residual term: the valid case's mean with the mislabelled proposals' terms replaced by Huber(0 - label residual)
        rk, gk = ("heading_residual_loss", "heading_residuals") if field == "heading_labels" else ("size_residual_loss", "size_residuals")
        hub = lambda e: np.where(np.abs(e) <= 1, 0.5 * e * e, np.abs(e) - 0.5)
        o64, lab = out[s][mine].astype(np.float64), np.atleast_1d(gt[gk][s, j].astype(np.float64))
        delta = (hub(0.0 - lab).sum() * mine.sum() - hub(o64[:, res_cols] - lab[None]).sum()) / r["n_pos"]
        assert float(r[rk]) == pytest.approx(float(r0[rk]) + delta, rel=1e-12)
    assert np.allclose(gw[~changed], gw0[~changed], rtol=1e-12, atol=0)
    for k in ("votes_xyz", "proposals_xyz"):
        assert torch.equal(g[k], g0[k]), k


def test_an_unguarded_row_index_gives_a_finite_heading_term():
    """heading_label == nh used as a row index (what the kernel did): the class term takes the first residual logit for the label's
    logit and stays FINITE, where the defined behaviour is NaN -- a kernel without the range check cannot pass the NaN assertions."""
    seeds, votes, prop, out, gt, kw = load_case("label-heading-nh")
    s, j, field, valid = label_box("label-heading-nh")
    r, _ = reference("label-heading-nh")
    pb, pp = torch.nonzero(r["positive"], as_tuple=True)
    pg = r["bboxes_assignment"][pb, pp]
    rows = torch.from_numpy(out.copy()).double()[pb, pp]
    hl = torch.from_numpy(gt["heading_labels"].copy()).long()[pb, pg]
    assert int((hl == 12).sum()) >= 2
    unguarded = (torch.logsumexp(rows[:, 5:17], 1) - rows[torch.arange(len(pb)), 5 + hl]).mean()
    assert np.isfinite(float(unguarded)) and np.isnan(float(r["heading_cls_loss"]))
