"""CPU: the vote supervision from instance labels without a device -- the numpy float32 restatement of
include/votenet_instance_votes.h (tests/instance_votes_ref.py) against its independent float64 form on hand-made cases, the labels of
the synthetic rooms (synth.room_scene_labels), and the interface: the export list and the header's entries, the switch of
VoteNetHotPath and what it excludes, the library's argument checks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_votes_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402
from votenet_amd import synth  # noqa: E402

F = np.float32
NAMES = ["votenet_instance_vote_loss", "votenet_instvote_last_error", "votenet_instvote_workspace_bytes", "votenet_seed_points"]


def close(got, want):
    """the project's tolerance on loss values: 1e-5 relative, floor 1.0 (tests/test_gpu_loss.py)"""
    return abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))


# ------------------------------------------------------------------ the two restatements on hand-made cases
def test_a_hand_made_scene_seed_by_seed():
    """Six cloud points, four sa1 centres, five seeds, two boxes.  Seed 0: a point of box 1; seed 1: an unlabelled point; seed 2: idx2
    out of range; seed 3: idx1 out of range; seed 4: a row beyond bb."""
    idx1 = np.array([[5, 2, 9, 0]], np.int32)          # centre 2 points at cloud point 9 of 6
    idx2 = np.array([[0, 1, 4, 2, 3]], np.int32)       # seed 2 points at centre 4 of 4
    point_box = np.array([[2, 0, -1, 0, 0, 1]], np.int32)  # point 5 -> box 1, point 2 -> none, point 0 -> row 2 of 2
    xyz = np.array([[[0, 0, 0], [1, 2, 3]]], F)
    votes = np.array([[[1.5, 2, 2], [9, 9, 9], [9, 9, 9], [9, 9, 9], [9, 9, 9]]], F)
    got = R.loss(idx1, idx2, point_box, votes, xyz)
    assert got["seed_point"].tolist() == [[5, 2, -1, -1, 0]] and got["row"].tolist() == [[1, -1, -1, -1, -1]]
    assert got["P"] == 1 and got["Q"] == 3
    assert got["dist"][0].tolist() == [1.5, 0, 0, 0, 0] and close(got["L"], 1.5)
    inv = got["inv"]
    assert got["d_votes"][0].tolist() == [[inv, 0, -inv], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert (got["d_votes"].view(np.int32) != np.int32(-2 ** 31)).all()  # no -0.0
    assert R.seed_points(idx1, idx2, 6).tolist() == [[5, 2, -1, -1, 0]]
    L64, v, P, Q, sp = R.loss64(idx1, idx2, point_box, votes, xyz)
    assert (P, Q, sp) == (1, 3, [[5, 2, -1, -1, 0]]) and close(got["L"], float(L64.detach()))


@pytest.mark.parametrize("shape,repeated", [((1, 1, 1), False), ((2, 63, 2), False), ((3, 257, 7), True), ((2, 300, 256), False)],
                         ids=lambda v: "rep" if v is True else "perm" if v is False else "b%d-n%d-bb%d" % v)
def test_float32_and_float64_forms_agree(shape, repeated):
    b, n, bb = shape
    idx1, idx2, n0 = R.levels_case(b, n, 5 + n, repeated)
    point_box, xyz = R.labels_case(b, n0, bb, 7 + n)
    votes = R.votes_case(b, n, 9 + n)
    idx2[0, 0] = -1                                   # an invalid chain
    point_box[b - 1, idx1[b - 1, idx2[b - 1, n - 1]]] = bb  # the last seed's row is beyond the table (its own, or the whole scene's at n = 1)
    got = R.loss(idx1, idx2, point_box, votes, xyz)
    L64, v, P, Q, sp = R.loss64(idx1, idx2, point_box, votes, xyz)
    assert got["P"] == P and got["Q"] == Q and Q >= 1 and got["seed_point"].tolist() == sp
    if P:
        L64.backward()
        g = v.grad.numpy()
        assert np.abs(got["d_votes"] - g).max() <= 1e-5 * max(1e-3, np.abs(g).max())
    assert close(got["L"], float(L64.detach()))
    assert close(got["L"], got["dist"].astype(np.float64).sum() * float(got["inv"]))  # the device's order of the sum changes nothing here
    assert not got["d_votes"][~got["supervised"]].any()


def test_no_supervised_seed_gives_zero_and_nan_votes_keep_the_cotangent_finite():
    idx1, idx2, n0 = R.levels_case(2, 65, 3)
    point_box, xyz = R.labels_case(2, n0, 5, 4)
    votes = R.votes_case(2, 65, 5)
    none = R.loss(idx1, idx2, np.full_like(point_box, -1), votes, xyz)
    assert none["P"] == 0 and none["Q"] == 0 and none["L"] == 0.0 and not none["d_votes"].view(np.int32).any()
    base = R.loss(idx1, idx2, point_box, votes, xyz)
    j = int(np.nonzero(base["supervised"][1])[0][2])
    votes[1, j, 1] = np.nan
    votes[0, int(np.nonzero(~base["supervised"][0])[0][0])] = np.inf  # at an unsupervised seed: nothing of it arrives
    got = R.loss(idx1, idx2, point_box, votes, xyz)
    assert np.isnan(got["L"]) and np.isfinite(got["d_votes"]).all() and got["d_votes"][1, j, 1] == 0.0 and got["d_votes"][1, j, 0] != 0.0
    votes[1, j, 1] = np.inf
    got = R.loss(idx1, idx2, point_box, votes, xyz)
    assert np.isinf(got["L"]) and got["d_votes"][1, j, 1] == got["inv"]


# ------------------------------------------------------------------ the labels of the synthetic rooms
@pytest.mark.parametrize("seed", [1000, 77])
def test_room_scene_labels_follow_the_points(seed):
    """Every labelled point lies within 6 sigma of the surface of its own box: the noise is N(0, sigma = 5 mm) per coordinate, so the
    distance to the face the point was drawn on is at most the noise vector's length, which exceeds 6 sigma once in 10^7 points; the
    boxes come back rounded to float32 (2.4e-7 m at these coordinates), 1e-5 m covers that."""
    n = 4096
    pts, boxes = synth.room_scene(n, seed)
    inst, sem = synth.room_scene_labels(n, seed)
    again, _ = synth.room_scene(n, seed)
    assert np.array_equal(pts, again)
    assert inst.shape == (n,) and sem.shape == (n,) and inst.dtype == np.int32 and sem.dtype == np.int32
    assert inst.min() == -1 and inst.max() == len(boxes) - 1 and (inst >= 0).sum() == n - int(n * 0.6)
    assert ((inst < 0) == (sem < 0)).all() and sem.max() <= 9
    worst = 0.0
    for i, (cx, cy, cz, l, w, h, ang, cls) in enumerate(boxes.astype(np.float64)):
        mine = inst == i
        assert mine.sum() >= (n - int(n * 0.6)) // len(boxes) and (sem[mine] == int(cls)).all()
        q = pts[mine].astype(np.float64) - [cx, cy, cz]
        c, s = np.cos(ang), np.sin(ang)
        local = np.stack([c * q[:, 0] - s * q[:, 2], q[:, 1], s * q[:, 0] + c * q[:, 2]], 1)  # the box frame (room_scene's rotation undone)
        d = np.abs(local) - np.array([l, h, w]) / 2
        surf = np.where((d <= 0).all(1), (-d).min(1), np.linalg.norm(np.maximum(d, 0), axis=1))  # inside: to the nearest face
        worst = max(worst, float(surf.max()))
    print("seed", seed, "largest distance of a labelled point to its own box's surface: %.4f m" % worst)
    assert worst <= 6 * 0.005 + 1e-5
    # a point of another box, or of the floor, is in general NOT on this box's surface: the labels are not interchangeable
    cx, cy, cz, l, w, h, ang, _ = boxes[0].astype(np.float64)
    q = pts[inst != 0].astype(np.float64) - [cx, cy, cz]
    c, s = np.cos(ang), np.sin(ang)
    d = np.abs(np.stack([c * q[:, 0] - s * q[:, 2], q[:, 1], s * q[:, 0] + c * q[:, 2]], 1)) - np.array([l, h, w]) / 2
    assert (np.linalg.norm(np.maximum(d, 0), axis=1) > 0.05).mean() > 0.5


# ------------------------------------------------------------------ the interface
def test_the_export_list_is_the_header_and_the_binding_follows_it(hiplib):
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, L.SIDE_LIBS["instvote"])) as f:
        protos = L.parse_header(f.read(), {})
    I, V = ctypes.c_int, ctypes.c_void_p
    assert sorted(protos) == NAMES
    assert protos["votenet_instvote_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_instvote_workspace_bytes"] == (ctypes.c_size_t, [I])
    assert protos["votenet_seed_points"] == (I, [I] * 4 + [V] * 4)
    assert protos["votenet_instance_vote_loss"] == (I, [I] * 5 + [V] * 10)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.side_path("instvote")], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in nm.splitlines() if line.split()[-2] in "TW")
    assert exported == NAMES
    lib = L.side_lib("instvote")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == protos[name]


def test_the_modes_exclude_each_other_and_vote_supervision_keeps_its_own():
    from votenet_amd import instance_votes as IV
    from votenet_amd import vote_supervision as VS
    from votenet_amd.model import VoteNetHotPath
    assert VS.MODES == ("reference", "paper")
    assert IV.MODES == ("reference", "instance")
    assert VoteNetHotPath.instance_votes is None
    net = object.__new__(VoteNetHotPath)  # the switch needs no device
    assert net.instance_votes is None
    with pytest.raises(L.InvalidArgumentError, match="nonsense"):
        net.enable_instance_votes("nonsense")
    assert net.instance_votes is None
    net.enable_instance_votes()
    assert net.instance_votes == "instance"
    with pytest.raises(L.InvalidArgumentError, match="disable_instance_votes"):
        net.enable_vote_supervision("paper")
    assert net.vote_supervision is None
    net.enable_vote_supervision("reference")  # the reference's rule launches nothing: it combines freely
    assert net.vote_supervision == "reference" and net.instance_votes == "instance"
    net.disable_instance_votes()
    assert net.instance_votes is None
    net.enable_vote_supervision("paper")
    with pytest.raises(L.InvalidArgumentError, match="disable_vote_supervision"):
        net.enable_instance_votes()
    assert net.instance_votes is None and net.vote_supervision == "paper"
    net.enable_instance_votes("reference")
    assert net.instance_votes == "reference"
    net.disable_vote_supervision()
    net.enable_instance_votes()
    assert net.instance_votes == "instance"
    net.disable_instance_votes()
    assert net.instance_votes is None and net.vote_supervision is None


def test_the_library_checks_its_arguments_before_anything_is_launched(hiplib):
    """Every invalid-argument case returns 1 with the limit in the text: no device is needed."""
    lib = L.side_lib("instvote")
    buf = np.zeros(4096, F)
    p = buf.ctypes.data
    err = lambda: lib.votenet_instvote_last_error().decode()

    def sp(b=2, n0=64, n1=32, n=16, idx1=p, idx2=p, out=p):
        return lib.votenet_seed_points(b, n0, n1, n, idx1, idx2, out, None)

    def il(b=2, n0=64, n1=32, n=16, bb=4, idx1=p, idx2=p, point_box=p, votes=p, xyz=p, losses=p, d_votes=p + 8192, counts=None, ws=p):
        return lib.votenet_instance_vote_loss(b, n0, n1, n, bb, idx1, idx2, point_box, votes, xyz, losses, d_votes, counts, ws, None)
    for fn in (sp, il):
        for kw, text in ((dict(b=0), "1 to 65535 scenes"), (dict(b=65536), "got b = 65536"), (dict(n=0), "n >= 1"), (dict(n=-5), "n >= 1"),
                         (dict(b=60000, n=60000), "b * n * 3 < 2^31"), (dict(n1=0), "n1 >= 1"), (dict(n0=0), "n0 >= 1"),
                         (dict(b=60000, n0=60000), "b * n0 < 2^31"), (dict(idx1=None), "null"), (dict(idx2=None), "null")):
            assert fn(**kw) == 1, kw
            assert text in err(), (kw, err())
    assert sp(out=None) == 1 and "null" in err()
    for kw, text in ((dict(bb=257), "1 to 256 boxes per scene, got bb = 257"), (dict(bb=0), "1 to 256 boxes"), (dict(point_box=None), "null"),
                     (dict(votes=None), "null"), (dict(xyz=None), "null"), (dict(losses=None), "null"), (dict(d_votes=None), "null"),
                     (dict(ws=None), "null"), (dict(d_votes=p), "may not overlap"), (dict(d_votes=p + 2 * 16 * 12 - 4), "may not overlap"),
                     (dict(ws=p + 2), "4-byte aligned")):
        assert il(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert lib.votenet_instvote_workspace_bytes(8) == 16 + 8 * 4 and lib.votenet_instvote_workspace_bytes(-3) == 16
    with pytest.raises(L.InvalidArgumentError, match=r"1 to 256 boxes per scene, got bb = 257"):
        L.check(il(bb=257), side="instvote")
