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
