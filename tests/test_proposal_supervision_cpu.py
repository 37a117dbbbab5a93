"""CPU: the paper's objectness and centre supervision without a device -- the numpy float32 restatement of
include/votenet_proposal_supervision.h (tests/proposal_supervision_ref.py, form a) against the independent float64 form (b: torch double
autograd with labels and arg-mins as constants), the real-box rule under the edge padding of the ground truth, the empty sets, the
re-formed box loss and total, and the interface: the header's entries, the switch of VoteNetHotPath, the library's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_supervision_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402

F = np.float32
NAMES = ["votenet_paper_proposal_loss", "votenet_proposal_targets", "votenet_propsup_last_error", "votenet_propsup_workspace_bytes"]


def close(got, want, floor=1.0):
    """the project's tolerance on loss values / cotangents: 1e-5 relative, floor 1.0 / 1e-3 (tests/test_gpu_loss.py)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.abs(got - want).max() <= 1e-5 * max(floor, np.abs(want).max()))


# ------------------------------------------------------------------ (a) against (b)
@pytest.mark.parametrize("shape", [(1, 40, 5, 8), (3, 64, 5, 5), (2, 256, 7, 16)], ids=lambda s: "b%d-p%d-g%d-bb%d" % s)
def test_float32_restatement_equals_float64_autograd(shape):
    b, p, real, bb = shape
    pxyz, pout, gxyz = R.random_case(100 + p, b, p, real, bb)
    a, ref = R.loss(pxyz, pout, gxyz), R.loss64(pxyz, pout, gxyz)
    print(shape, "Np Nn G", a["Np"], a["Nn"], a["G"], "obj", a["obj"], ref["obj"], "center", a["center"], ref["center"],
          "margins", ref["margin_thr"], ref["margin_arg"])
    assert (a["Np"], a["Nn"], a["G"]) == (ref["Np"], ref["Nn"], ref["G"]) and a["G"] == b * real
    assert a["Np"] > 0 and a["Nn"] > 0 and a["Np"] + a["Nn"] < b * p  # positives, negatives and grey proposals
    assert close(a["obj"], ref["obj"]) and close(a["center"], ref["center"])
    assert close(a["d_obj"], ref["d_out"][..., :2], 1e-3) and close(a["d_ctr"], ref["d_out"][..., 2:5], 1e-3)
    assert close(a["d_ctr"], ref["d_xyz"], 1e-3)
    grey = np.stack([~(r["pos"] | r["neg"]) for r in a["scenes"]])
    assert not a["d_obj"][grey].any() and not np.signbit(a["d_obj"][grey]).any()


def test_targets_are_the_decisions_of_the_loss():
    pxyz, pout, gxyz = R.random_case(7, 2, 64, 5, 8)
    label, near, dual, real = R.targets(pxyz, pout, gxyz)
    assert real.tolist() == [5, 5] and (dual[:, 5:] == -1).all() and (dual[:, :5] >= 0).all() and dual.max() < 64
    assert ((near >= 0) == (label == 1)).all() and near.max() < 5
    for s in range(2):  # float64 agrees on every decision (the case is clear of the margins)
        c = pxyz[s].astype(np.float64) + pout[s, :, 2:5].astype(np.float64)
        q = ((c[:, None] - gxyz[s, :5].astype(np.float64)[None]) ** 2).sum(-1)
        assert np.array_equal(q.argmin(0), dual[s, :5]) and np.array_equal(q.argmin(1)[label[s] == 1], near[s][label[s] == 1])


# ------------------------------------------------------------------ the real-box rule
def test_edge_padding_changes_nothing():
    pxyz, pout, gxyz = R.random_case(11, 2, 64, 5)
    for extra in (1, 3, 251):
        padded = R.edge_pad(gxyz, extra)
        a, b = R.loss(pxyz, pout, gxyz), R.loss(pxyz, pout, padded)
        assert a["G"] == b["G"] == 10 and (a["Np"], a["Nn"]) == (b["Np"], b["Nn"])
        for ra, rb in zip(a["scenes"], b["scenes"]):
            assert ra["g"] == rb["g"] == 5
            assert np.array_equal(ra["f"].view(np.int32), rb["f"].view(np.int32)) and np.array_equal(ra["i2"], rb["i2"])
        assert a["obj"].view(np.int32) == b["obj"].view(np.int32) and a["center"].view(np.int32) == b["center"].view(np.int32)
        assert np.array_equal(a["d_ctr"].view(np.int32), b["d_ctr"].view(np.int32))
        assert np.array_equal(a["d_obj"].view(np.int32), b["d_obj"].view(np.int32))
        ref = R.loss64(pxyz, pout, padded)
        assert ref["G"] == 10 and close(b["center"], ref["center"])


def test_real_boxes_is_the_evaluators_rule():
    from votenet_amd import evaluator
    rng = np.random.default_rng(2)
    xyz = rng.random((4, 6, 3)).astype(F)
    xyz[0, 3:] = xyz[0, 2]          # three copies of row 2: 3 real
    xyz[1, :] = xyz[1, 0]           # all equal: 1 real
    xyz[2, 4] = xyz[2, 3]           # an interior repetition is not padding
    xyz[3, 5] = xyz[3, 4]
    xyz[3, 5, 2] = np.nextafter(xyz[3, 5, 2], F(2))  # one ulp off in z: a box of its own
    gt = dict(bboxes_xyz=xyz, bboxes_lwh=np.ones_like(xyz), bboxes_roty=np.zeros((4, 6), F), semantic_labels=np.zeros((4, 6), np.int32))
    want = evaluator.gt_for_eval(gt)["count"].tolist()
    assert [R.real_boxes(x) for x in xyz] == want == [3, 1, 6, 6]
    nan = xyz[:1].copy()
    nan[0, -2:] = np.nan            # NaN rows never compare equal: not padding
    assert R.real_boxes(nan[0]) == 6


# ------------------------------------------------------------------ the empty sets
def test_empty_sets_and_one_box_give_zeros_not_nan():
    pxyz, pout, gxyz = R.random_case(13, 2, 40, 3)
    # M = 0: every proposal in the grey zone (0.45 from one centre, far from the others)
    grey = (gxyz[:, :1] + np.array([0.45, 0, 0], F)).repeat(40, axis=1) + np.zeros((2, 40, 3), F)
    gfar = gxyz.copy()
    gfar[:, 1:] += F(50.0)
    a = R.loss(grey, pout, gfar)
    assert (a["Np"], a["Nn"]) == (0, 0) and a["obj"] == 0.0 and not a["d_obj"].any() and not np.signbit(a["d_obj"]).any()
    assert np.isfinite(a["center"]) and np.isfinite(a["d_ctr"]).all() and a["center"] > 0  # the boxes still pull their nearest centres
    ref = R.loss64(grey, pout, gfar)
    assert close(a["center"], ref["center"]) and close(a["d_ctr"], ref["d_xyz"], 1e-3)
    # Np = 0 with negatives: objectness over the negatives alone, no positive centre term
    far = grey + F(20.0)
    a, ref = R.loss(far, pout, gxyz), R.loss64(far, pout, gxyz)
    assert a["Np"] == 0 and a["Nn"] == 80 and np.isfinite(a["obj"]) and a["obj"] > 0 and np.isfinite(a["center"])
    assert close(a["obj"], ref["obj"]) and close(a["center"], ref["center"]) and close(a["d_obj"], ref["d_out"][..., :2], 1e-3)
    # bb = 1, and bb = 1 with one proposal
    for p in (40, 1):
        a, ref = R.loss(pxyz[:, :p], pout[:, :p], gxyz[:, :1]), R.loss64(pxyz[:, :p], pout[:, :p], gxyz[:, :1])
        assert a["G"] == 2 and np.isfinite([a["obj"], a["center"]]).all() and np.isfinite(a["d_ctr"]).all()
        assert close(a["obj"], ref["obj"]) and close(a["center"], ref["center"]) and close(a["d_ctr"], ref["d_xyz"], 1e-3)
        assert all(r["i2"].shape == (1,) for r in a["scenes"])


# ------------------------------------------------------------------ ties and non-finite values (form a alone)
def test_first_index_wins_and_a_first_nan_sticks():
    q = np.array([[3, 1, 1, 0.5, 0.5], [np.nan, 1, 0, 0, 0], [2, np.nan, 1, np.nan, 1], [np.inf, np.inf, np.inf, np.inf, np.inf]], F)
    best, idx = R.first_min(q)
    assert idx.tolist() == [3, 0, 2, 0] and np.isnan(best[1]) and best[[0, 2, 3]].tolist() == [0.5, 1.0, np.inf]
    # one proposal wins several boxes: its terms are added in ascending j (float32 addition does not commute with that order)
    gxyz = np.array([[[0, 0, 0], [1e-3, 0, 0], [3, 0, 0], [3, 1e-4, 0]]], F)
    pxyz = np.array([[[0.1, 0.01, 0.02], [0.1, 0.01, 0.02], [9, 9, 9]]], F)
    pout = np.zeros((1, 3, R.W), F)
    a = R.loss(pxyz, pout, gxyz)
    r = a["scenes"][0]
    assert r["i2"].tolist() == [0, 0, 0, 0] and r["j1"][:2].tolist() == [1, 1] and a["Np"] == 2
    inv_p, inv_g = F(1) / (F(2) + F(1e-6)), F(1) / (F(4) + F(1e-6))
    c = pxyz[0, 0]
    want = (F(2) * (c - gxyz[0, 1])) * inv_p
    for j in range(4):
        want = want + (F(2) * (c - gxyz[0, j])) * inv_g
    assert np.array_equal(a["d_ctr"][0, 0].view(np.int32), want.view(np.int32))
    assert np.array_equal(a["d_ctr"][0, 1].view(np.int32), ((F(2) * (c - gxyz[0, 1])) * inv_p).view(np.int32))  # the duplicate: no dual term
    assert not a["d_ctr"][0, 2].any()


# ------------------------------------------------------------------ the loss vector
def test_box_loss_and_total_are_reformed_in_the_loss_kernels_order():
    l0 = R.fake_losses(5)
    assert l0[9] == (((l0[3] + F(0.1) * l0[4]) + l0[5]) + F(0.1) * l0[6]) + l0[7]
    assert l0[0] == ((l0[1] + F(0.5) * l0[2]) + l0[9]) + F(0.1) * l0[8]
    pxyz, pout, gxyz = R.random_case(17, 2, 40, 4)
    a = R.loss(pxyz, pout, gxyz, losses=l0)
    l = a["losses"]
    assert l[2] == a["obj"] and l[3] == a["center"] and l[9] != l0[9] and l[0] != l0[0]
    keep = [1, 4, 5, 6, 7, 8, 10, 11]
    assert np.array_equal(l[keep].view(np.int32), l0[keep].view(np.int32))
    want9 = float(l[3]) + 0.1 * float(l[4]) + float(l[5]) + 0.1 * float(l[6]) + float(l[7])
    assert close(l[9], want9) and close(l[0], float(l[1]) + 0.5 * float(l[2]) + want9 + 0.1 * float(l[8]))


# ------------------------------------------------------------------ the interface
def test_header_declares_the_four_entries_and_the_binding_follows_it(hiplib):
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, L.SIDE_LIBS["propsup"])) as f:
        protos = L.parse_header(f.read(), {})
    I, V, Fl, Lg = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_long
    assert sorted(protos) == NAMES
    assert protos["votenet_propsup_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_propsup_workspace_bytes"] == (ctypes.c_size_t, [I])
    assert protos["votenet_proposal_targets"] == (I, [I, I, I, V, V, Lg, V, Fl, Fl, V, V, V, V, V])
    assert protos["votenet_paper_proposal_loss"] == (I, [I] * 6 + [V, V, Lg, V, Fl, Fl, V, V, V, V, V, V])
    lib = L.side_lib("propsup")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == protos[name]


def test_the_mode_is_off_by_default_and_an_unknown_mode_is_refused():
    from votenet_amd import proposal_supervision as PS
    from votenet_amd.model import VoteNetHotPath
    assert PS.MODES == ("reference", "paper") and PS.OBJ_WEIGHTS == (0.2, 0.8)
    assert VoteNetHotPath.proposal_supervision is None
    net = object.__new__(VoteNetHotPath)  # the switch needs no device
    with pytest.raises(L.InvalidArgumentError, match="nonsense"):
        net.enable_proposal_supervision("nonsense")
    assert net.proposal_supervision is None
    net.enable_proposal_supervision()
    assert net.proposal_supervision == "paper" and net.vote_supervision is None  # independent of the vote mode
    net.enable_proposal_supervision("reference")
    assert net.proposal_supervision == "reference"
    net.disable_proposal_supervision()
    assert net.proposal_supervision is None


def test_the_library_checks_its_arguments_before_anything_is_launched(hiplib):
    """Every invalid-argument case returns 1 with the limit in the text: no device is needed."""
    lib = L.side_lib("propsup")
    buf = np.zeros(1 << 16, F)
    p0 = buf.ctypes.data
    err = lambda: lib.votenet_propsup_last_error().decode()

    def tg(b=2, p=16, bb=4, pxyz=p0, pout=p0, pitch=R.W, gxyz=p0, pos=0.3, neg=0.6, label=p0, near=p0, dual=p0, real=p0):
        return lib.votenet_proposal_targets(b, p, bb, pxyz, pout, pitch, gxyz, pos, neg, label, near, dual, real, None)

    def pl(b=2, p=16, bb=4, nh=12, ns=10, nc=10, pxyz=p0, pout=p0, pitch=R.W, gxyz=p0, pos=0.3, neg=0.6, losses=p0, d_xyz=p0 + (1 << 17),
           d_out=p0 + (1 << 17), counts=None, ws=p0):
        return lib.votenet_paper_proposal_loss(b, p, bb, nh, ns, nc, pxyz, pout, pitch, gxyz, pos, neg, losses, d_xyz, d_out, counts, ws, None)
    for fn in (tg, pl):
        for kw, text in ((dict(p=1025), "1 to 1024 proposals per scene, got p = 1025"), (dict(p=0), "1 to 1024 proposals"),
                         (dict(bb=257), "1 to 256 boxes per scene, got bb = 257"), (dict(bb=0), "1 to 256 boxes"),
                         (dict(b=0), "1 to 65535 scenes"), (dict(b=65536), "got b = 65536"), (dict(pos=0.6, neg=0.3), "pos_thr < neg_thr"),
                         (dict(pxyz=None), "null"), (dict(pout=None), "null"), (dict(gxyz=None), "null")):
            assert fn(**kw) == 1, kw
            assert text in err(), (kw, err())
    for kw in (dict(label=None), dict(near=None), dict(dual=None), dict(real=None)):
        assert tg(**kw) == 1 and "null" in err()
    assert tg(pitch=4) == 1 and "pitch" in err()
    for kw, text in ((dict(pitch=R.W - 1), "smaller than its width (79)"), (dict(nh=33), "nh, ns, nc <= 32"), (dict(ns=0), "nh, ns, nc"),
                     (dict(nc=-1), "nh, ns, nc"), (dict(losses=None), "null"), (dict(d_xyz=None), "null"), (dict(d_out=None), "null"),
                     (dict(ws=None), "null"), (dict(d_xyz=p0), "d_proposals_xyz may not overlap"),
                     (dict(d_xyz=p0 + 2 * 16 * 12 - 4), "d_proposals_xyz may not overlap"),
                     (dict(d_out=p0 + 4 * (2 * 16 * 128 - 50), pitch=128), "d_proposals_output may not overlap"),
                     (dict(ws=p0 + 2), "4-byte aligned")):
        assert pl(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert lib.votenet_propsup_workspace_bytes(8) == 16 + 8 * 12 and lib.votenet_propsup_workspace_bytes(-3) == 16
    with pytest.raises(L.InvalidArgumentError, match=r"1 to 1024 proposals per scene, got p = 1025"):
        L.check(tg(p=1025), side="propsup")
