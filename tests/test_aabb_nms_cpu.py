"""CPU: the axis-aligned NMS overlaps without a device -- the numpy float32 restatement of include/votenet_aabb_nms.h
(tests/aabb_nms_ref.py) against the oracle's rotated-box IoU where the two must agree (heading 0), hand-built cases with known answers
for every clause of the two rules, NaN and degenerate boxes, the C ABI entry points in the header, their derived binding, the
library's export list and its argument checks, and the keywords of predict / evaluate."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aabb_nms_ref as A  # noqa: E402
import detections_ref as R  # noqa: E402

import cases  # noqa: E402  (tests/golden, on the path by conftest.py)
from votenet_amd import _lib as L  # noqa: E402

F = np.float32
NAMES = ["votenet_aabb_last_error", "votenet_aabb_overlap_matrix", "votenet_class_nms_aabb", "votenet_class_nms_aabb_workspace_bytes"]
ALL = [(mode, measure) for mode in A.MODES for measure in A.MEASURES]


def box(lo, hi):
    """the box [lo_x, hi_x] x [lo_y, hi_y] x [lo_z, hi_z] in decode_boxes' corner order"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    l, h, w = hi - lo
    return cases.corner_box(l, w, h, None, (lo + hi) / 2).astype(F)


def obj_of(d):
    d = np.asarray(d, F)
    return np.stack([np.zeros_like(d), d], -1)


def one_class(n, nc=3):
    out = np.zeros((1, n, nc), F)
    out[..., 1] = 4.0
    return out


def kept(table, d, thr=0.25, cls=None):
    """the kept list of one scene whose boxes have margins d, all of one class unless cls is given"""
    cls = one_class(len(d)) if cls is None else cls
    return R.class_nms3d(table, obj_of([d]), cls, thr, 0.05, class_nms=True, per_class=False)["kept"][0]


# ------------------------------------------------------------------ the restatement is tied to the reference
GRID = 1024  # corner coordinates are multiples of 1 / 1024 below 8: 13 bits


def upright(rng, b, n, room):
    """Boxes with heading 0 by evaluator.box_corners, centres on the grid and sizes on twice the grid, so every corner is on it.
    Why a grid: tf_nms3d.cpp:69-100 (oracle_nms3d.cpp, segment_intersection) forms an edge crossing as a quotient in double and
    accepts it only if it lies INSIDE both segments' float bounding boxes, bounds included.  For an edge that is exactly parallel to
    an axis that box has no width: the quotient must come out as the edge's coordinate to the last bit, or the crossing is lost and
    the clip returns too small an area (with free float coordinates it does so for 220 of the 4512 pairs of seed 0, by up to 0.32).
    On the grid every product in that quotient is exact in double (three 13-bit factors), the quotient is k x / k = x, and the
    reference's clip is what it means to be."""
    from votenet_amd import evaluator as E
    centre = rng.integers(0, [room * GRID, GRID, room * GRID], (b, n, 3)) / GRID
    lwh = rng.integers(int(0.3 * GRID / 2), int(1.5 * GRID / 2), (b, n, 3)) * 2 / GRID
    boxes = E.box_corners(centre, lwh, np.zeros((b, n)))
    assert np.array_equal(boxes * GRID, np.round(boxes * GRID))
    return boxes


@pytest.mark.parametrize("seed,b,n,room", [(0, 2, 48, 3), (1, 3, 96, 4)])
def test_heading_zero_table_is_the_oracles_rotated_iou_and_keeps_the_same_boxes(O, seed, b, n, room):
    """A box with heading 0 is its own hull: the aabb3d / iou table is the rotated IoU of tf_nms3d.cpp (the oracle's restatement)
    within 1e-5, and the NMS over either table keeps the same boxes.  The scenes are chosen, not measured: no pair of them lies
    within 1e-4 of the threshold in either table -- the share of pairs that condition excludes is 0 for these seeds."""
    thr = 0.25
    rng = np.random.default_rng(seed)
    boxes = upright(rng, b, n, room)
    mine = A.overlap_table(boxes, "aabb3d", "iou")
    ref = np.stack([O.iou3d_matrix(boxes[s]) for s in range(b)])
    off = ~np.eye(n, dtype=bool)
    err = np.abs(mine - ref)
    print("largest difference %.3g over %d pairs, %d overlapping" % (err.max(), err.size, int((ref[:, off] > 0).sum())))
    assert err.max() <= 1e-5  # the diagonal included
    assert np.array_equal(mine, np.swapaxes(mine, 1, 2))  # the IoU of two boxes does not depend on which comes later
    excluded = (np.abs(mine - F(thr)) < 1e-4) | (np.abs(ref - F(thr)) < 1e-4)
    assert excluded[:, off].mean() == 0.0
    assert (ref[:, off] > thr).sum() >= n  # the scenes are crowded: the NMS has work
    obj = rng.normal(size=(b, n, 2)).astype(F) * 2
    cls = rng.normal(size=(b, n, 4)).astype(F)
    for cn in (True, False):
        for pc in (True, False):
            got = R.class_nms3d(mine, obj, cls, thr, 0.05, class_nms=cn, per_class=pc)
            exp = R.class_nms3d(ref, obj, cls, thr, 0.05, class_nms=cn, per_class=pc)
            assert got["kept"] == exp["kept"] and np.array_equal(got["rows"], exp["rows"]), (cn, pc)
            assert 0 < sum(map(len, got["kept"])) < int((R.margins(obj) > R.conf_logit(0.05)).sum())


# ------------------------------------------------------------------ geometry with known answers
def test_integer_boxes_at_exactly_the_threshold():
    """[0,5] x [0,1] x [0,1] and [3,8] x [0,1] x [0,1]: 2 / ((5 + 5) - 2) = 0.25 exactly.  The comparison is strict."""
    boxes = np.stack([box((0, 0, 0), (5, 1, 1)), box((3, 0, 0), (8, 1, 1))])[None]
    below = float(np.nextafter(F(0.25), F(0)))
    for mode in A.MODES:  # bev: the same rectangles on (x, z)
        t = A.overlap_table(boxes, mode, "iou")
        assert t[0, 1, 0] == F(0.25) and t[0, 0, 1] == F(0.25) and t[0, 0, 0] == 1.0
        assert kept(t, [2.0, 1.0], 0.25) == [0, 1]
        assert kept(t, [2.0, 1.0], below) == [0]
        assert A.overlap_table(boxes, mode, "over_later")[0, 1, 0] == F(0.4)  # 2 / 5


def test_bev_ignores_the_up_axis():
    boxes = np.stack([box((0, 0, 0), (1, 1, 1)), box((0, 5, 0), (1, 6, 1))])[None]  # they differ in y only
    assert A.overlap_table(boxes, "bev", "iou")[0, 1, 0] == 1.0 and A.overlap_table(boxes, "aabb3d", "iou")[0, 1, 0] == 0.0
    assert kept(A.overlap_table(boxes, "bev", "iou"), [2.0, 1.0]) == [0]
    assert kept(A.overlap_table(boxes, "aabb3d", "iou"), [2.0, 1.0]) == [0, 1]
    swapped = boxes[..., [0, 2, 1]]  # ... and y is the axis it ignores: boxes that differ in z only do not overlap
    assert A.overlap_table(swapped, "bev", "iou")[0, 1, 0] == 0.0


def test_over_later_is_asymmetric():
    """A small box inside a large one: all of it is covered when it comes later, an eighth of the large one when that does."""
    boxes = np.stack([box((0, 0, 0), (2, 2, 2)), box((0.5, 0.5, 0.5), (1.5, 1.5, 1.5))])[None]
    t = A.overlap_table(boxes, "aabb3d", "over_later")
    assert t[0, 1, 0] == 1.0 and t[0, 0, 1] == F(1.0) / F(8.0)
    assert A.overlap_table(boxes, "bev", "over_later")[0, 0, 1] == F(0.25)
    assert A.overlap_table(boxes, "aabb3d", "iou")[0, 1, 0] == F(0.125)
    assert kept(t, [2.0, 1.0], 0.25) == [0] and kept(t, [1.0, 2.0], 0.25) == [1, 0]  # the order decides who falls


def test_thin_rotated_boxes_side_by_side_fall_by_the_hull_and_stand_by_the_rotated_iou(O):
    """Two 2 x 0.1 slats at 45 degrees, 0.3 apart across their length: they do not touch (rotated IoU 0), their hulls are squares
    of side 2.1 / sqrt(2) shifted by 0.21 in x and z: IoU 0.58."""
    c = 0.3 / np.sqrt(2.0)
    boxes = np.stack([cases.corner_box(2.0, 0.1, 1.0, np.pi / 4, (0, 0, 0)), cases.corner_box(2.0, 0.1, 1.0, np.pi / 4, (c, 0, c))]).astype(F)[None]
    rot = O.iou3d_matrix(boxes[0])[None]
    hull = A.overlap_table(boxes, "aabb3d", "iou")
    side = 2.1 / np.sqrt(2.0)
    assert rot[0, 1, 0] == 0.0 and abs(hull[0, 1, 0] - (side - c) ** 2 / (2 * side ** 2 - (side - c) ** 2)) < 1e-5 and hull[0, 1, 0] > 0.25
    assert kept(rot, [2.0, 1.0]) == [0, 1] and kept(hull, [2.0, 1.0]) == [0]
    assert kept(A.overlap_table(boxes, "bev", "iou"), [2.0, 1.0]) == [0]


def test_a_suppressed_box_suppresses_nothing():
    """A removes B; B alone would have removed C; with B gone C stays."""
    boxes = np.stack([box((0, 0, 0), (1, 1, 1)), box((0.5, 0, 0), (1.5, 1, 1)), box((1, 0, 0), (2, 1, 1))])[None]
    for mode, measure in ALL:
        t = A.overlap_table(boxes, mode, measure)
        assert t[0, 1, 0] > 0.25 and t[0, 2, 1] > 0.25 and t[0, 2, 0] == 0.0
        assert kept(t, [3.0, 2.0, 1.0]) == [0, 2]
        assert kept(t[:, 1:, 1:], [2.0, 1.0]) == [0]  # B alone removes C
    cls = one_class(3)
    cls[0, 1] = [9.0, 0.0, 0.0]  # B in a class of its own: nobody removes anybody
    assert kept(A.overlap_table(boxes), [3.0, 2.0, 1.0], cls=cls) == [0, 1, 2]


# ------------------------------------------------------------------ NaN and degenerate boxes
def test_a_nan_in_any_coordinate_gives_a_nan_row_and_a_nan_column():
    """Three copies of one box, nudged: every pair overlaps by far more than any threshold.  A NaN in any of box 1's 24 coordinates:
    under aabb3d / iou its row and its column are NaN, it neither falls nor removes anything.  What the formulas give elsewhere:
    over_later -- its row is NaN, its column 0; bev -- the eight y coordinates take no part."""
    base = np.stack([box((0, 0, 0), (1, 1, 1)), box((0.1, 0, 0), (1.1, 1, 1)), box((0.2, 0, 0), (1.2, 1, 1))])[None]
    assert kept(A.overlap_table(base), [3.0, 2.0, 1.0]) == [0]
    for corner in range(8):
        for axis in range(3):
            boxes = base.copy()
            boxes[0, 1, corner, axis] = np.nan
            lo, hi = A.extents(boxes)
            assert np.isnan(lo[0, 1, axis]) and np.isnan(hi[0, 1, axis]) and np.isnan(lo[0, 1]).sum() == 1, (corner, axis)
            t = A.overlap_table(boxes, "aabb3d", "iou")
            assert np.isnan(t[0, 1, :]).all() and np.isnan(t[0, :, 1]).all() and np.isnan(t).sum() == 5, (corner, axis)
            for thr in (0.0, 0.25):
                assert kept(t, [3.0, 2.0, 1.0], thr) == [0, 1] and kept(t, [2.0, 3.0, 1.0], thr) == [1, 0], (corner, axis)
            t = A.overlap_table(boxes, "aabb3d", "over_later")
            assert np.isnan(t[0, 1, :]).all() and (t[0, [0, 2], 1] == 0).all()
            assert kept(t, [3.0, 2.0, 1.0], 0.0) == [0, 1] and kept(t, [2.0, 3.0, 1.0], 0.0) == [1, 0]
            for measure in A.MEASURES:
                t = A.overlap_table(boxes, "bev", measure)
                if axis == 1:
                    assert np.array_equal(t, A.overlap_table(base, "bev", measure))
                else:
                    assert np.isnan(t[0, 1, :]).all() and not (t[0, :, 1] > 0).any()


def test_boxes_without_volume_and_infinite_boxes():
    flat = np.zeros((8, 3), F)
    unit, near = box((0, 0, 0), (1, 1, 1)), box((0.1, 0, 0), (1.1, 1, 1))
    boxes = np.stack([flat, unit, flat, near])[None]
    for mode in A.MODES:
        t = A.overlap_table(boxes, mode, "iou")
        assert np.isnan(t[0, 0, 0]) and np.isnan(t[0, 2, 0]) and np.isnan(t[0, 0, 2])  # 0 / 0
        assert (t[0, [0, 2]][:, [1, 3]] == 0).all() and (t[0, [1, 3]][:, [0, 2]] == 0).all()
        assert kept(t, [4.0, 3.0, 2.0, 1.0], 0.0) == [0, 1, 2]  # threshold 0: any overlap removes, and only `near` has one
        t = A.overlap_table(boxes, mode, "over_later")
        assert np.isnan(t[0, [0, 2]]).all() and (t[0, [1, 3]][:, [0, 2]] == 0).all()  # the later box without volume: 0 / 0
        assert kept(t, [4.0, 3.0, 2.0, 1.0], 0.0) == [0, 1, 2]
    slab = box((0, 0, 0), (1, 0, 1))  # no height: a volume of 0, a rectangle of 1
    boxes = np.stack([slab, slab])[None]
    assert np.isnan(A.overlap_table(boxes, "aabb3d", "iou")).all() and (A.overlap_table(boxes, "bev", "iou") == 1).all()
    huge = np.where(unit > 0.5, F(np.inf), F(-np.inf)).astype(F)  # every extent infinite
    boxes = np.stack([huge, unit, huge])[None]
    t = A.overlap_table(boxes, "aabb3d", "iou")
    assert t[0, 1, 0] == 0 and t[0, 0, 1] == 0 and np.isnan(t[0, 2, 0]) and np.isnan(t[0, 0, 0])  # 1 / inf; inf / (inf - inf)
    assert kept(t, [3.0, 2.0, 1.0], 0.0) == [0, 1, 2]


# ------------------------------------------------------------------ the C ABI
def test_header_declares_the_entries_and_the_binding_follows_it():
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, "votenet_aabb_nms.h")) as f:
        text = f.read()
    protos = L.parse_header(text, {})
    assert sorted(protos) == NAMES
    assert protos["votenet_aabb_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_aabb_overlap_matrix"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                    ctypes.c_void_p, ctypes.c_void_p])
    assert protos["votenet_class_nms_aabb_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    with open(os.path.join(inc, "votenet_detections.h")) as f:
        sibling = L.parse_header(f.read(), {})["votenet_class_nms3d"]
    ret, args = protos["votenet_class_nms_aabb"]  # the sibling entry with mode and measure after per_class
    assert ret is sibling[0] and args == sibling[1][:10] + [ctypes.c_int] * 2 + sibling[1][10:]
    from votenet_amd import aabb_nms
    for name, table in (("VOTENET_AABB_3D", aabb_nms._MODE["aabb3d"]), ("VOTENET_AABB_BEV", aabb_nms._MODE["bev"]),
                        ("VOTENET_AABB_IOU", aabb_nms._MEASURE["iou"]), ("VOTENET_AABB_OVER_LATER", aabb_nms._MEASURE["over_later"])):
        assert "#define %s %d\n" % (name, table) in text
    lib = L.side_lib("aabb")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == (protos[name][0], protos[name][1])
    assert aabb_nms.OVERLAPS == ("rotated", "aabb3d", "bev") and aabb_nms.PAPER_OVERLAP == "aabb3d"


def test_library_exports_exactly_its_header_and_checks_its_arguments(hiplib):
    """Every invalid-argument case returns before anything is launched, with the limit in the text: no device is needed."""
    lib = L.side_lib("aabb")
    defined = lambda path: [line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                                                                        check=True).stdout.splitlines()]
    assert sorted(defined(L.side_path("aabb"))) == NAMES
    for other in (L.lib_path(), L.side_path("detect"), L.side_path("boxpts")):  # the other libraries export what they did
        assert not set(NAMES) & set(defined(other))
    buf = np.zeros(4096, F)
    p = buf.ctypes.data
    err = lambda: lib.votenet_aabb_last_error().decode()

    def nms(b=2, n=16, nc=10, thr=0.25, t=0.0, cn=1, pc=1, mode=0, meas=0, cap=None, rows=p, off=p, ws=p, wsb=1 << 20):
        return lib.votenet_class_nms_aabb(b, n, nc, p, p, p, thr, t, cn, pc, mode, meas, rows, b * n * nc if cap is None else cap, off, ws, wsb, None)
    for kw, text in ((dict(n=513), "at most 512 boxes"), (dict(nc=65), "[1, 64]"), (dict(nc=0), "[1, 64]"), (dict(thr=1.5), "[0, 1]"),
                     (dict(thr=-0.1), "[0, 1]"), (dict(thr=float("nan")), "[0, 1]"), (dict(t=float("nan")), "conf_logit"),
                     (dict(t=float("inf")), "conf_logit"), (dict(cn=2), "0 or 1"), (dict(pc=-1), "0 or 1"), (dict(cap=2 * 16 * 10 - 1), "320 rows"),
                     (dict(pc=0, cap=31), "32 rows"), (dict(off=None), "det_offset"), (dict(rows=None), "null"),
                     (dict(rows=p + 4), "16-byte"), (dict(b=-1), "batch"), (dict(b=65536), "[0, 65535]"),
                     (dict(mode=2), "mode must be 0 (3D) or 1 (bird's-eye), got 2"), (dict(mode=-1), "mode must be 0"),
                     (dict(meas=2), "measure must be 0 (IoU) or 1 (intersection over the later box), got 2"), (dict(meas=-1), "measure must be 0")):
        assert nms(**kw) == 1, kw
        assert text in err(), (kw, err())
    need = lib.votenet_class_nms_aabb_workspace_bytes(2, 16, 10)
    assert need == L.side_lib("detect").votenet_class_nms3d_workspace_bytes(2, 16, 10) and lib.votenet_class_nms_aabb_workspace_bytes(0, 0, 1) > 0
    assert nms(wsb=need - 1) == 3 and "workspace of %d bytes required" % need in err()
    assert nms(ws=None) == 3 and "workspace of %d bytes required" % need in err()
    with pytest.raises(L.VotenetError, match="workspace of %d bytes" % need):
        L.check(nms(wsb=0), side="aabb")
    with pytest.raises(L.InvalidArgumentError, match="at most 512 boxes per scene, got n = 513"):
        L.check(nms(n=513), side="aabb")

    def matrix(b=2, n=16, mode=0, meas=0, boxes=p, out=p):
        return lib.votenet_aabb_overlap_matrix(b, n, boxes, mode, meas, out, None)
    for kw, text in ((dict(b=-1), "[0, 65535], got -1"), (dict(b=65536), "[0, 65535]"), (dict(n=-1), "at most 32768 boxes"),
                     (dict(n=32769), "at most 32768 boxes per scene, got n = 32769"), (dict(mode=2), "mode must be 0"),
                     (dict(meas=3), "measure must be 0"), (dict(boxes=None), "null"), (dict(out=None), "null")):
        assert matrix(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert matrix(b=0) == 0 and matrix(n=0, boxes=None, out=None) == 0  # launches nothing


def test_build_force_also_removes_the_aabb_library_and_its_objects(monkeypatch, tmp_path):
    from votenet_amd import _lib
    here = tmp_path / "votenet_amd"
    (here / "csrc" / "aabb" / "obj").mkdir(parents=True)
    (here / "lib").mkdir()
    for f in (here / "csrc" / "aabb" / "obj" / "aabb_nms.o", here / "lib" / "libvotenet_aabb.so", here / "lib" / "libvotenet_hip.so"):
        f.write_bytes(b"stale")
    seen = {}

    def fake_run(cmd, **kw):
        seen["left"] = sorted(p.name for d in ("csrc/aabb/obj", "lib") for p in (here / d).iterdir())
        return subprocess.CompletedProcess(cmd, 0, "", "")
    monkeypatch.setattr(_lib, "_HERE", str(here))
    monkeypatch.setattr(_lib, "_LIB_PATH", str(here / "lib" / "libvotenet_hip.so"))
    monkeypatch.setattr(_lib.subprocess, "run", fake_run)
    _lib.build(force=True)
    assert seen["left"] == []


# ------------------------------------------------------------------ the keywords of predict and evaluate
BAD_KEYWORDS = [(dict(nms_overlap="aabb3d"), "needs protocol"), (dict(nms_overlap="bev", protocol="reference"), "needs protocol"),
                (dict(protocol="per_class", nms_overlap="hull"), "nms_overlap must be one of"),
                (dict(protocol="per_class", nms_overlap=None), "nms_overlap must be one of"),
                (dict(protocol="per_class", nms_overlap="aabb3d", nms_measure="giou"), "nms_measure must be one of"),
                (dict(protocol="per_class", nms_measure="over_later"), "needs nms_overlap"),
                (dict(protocol="per_class", nms_overlap="rotated", nms_measure="over_later"), "needs nms_overlap"),
                (dict(nms_measure="over_later"), "needs nms_overlap")]


def test_predict_and_evaluate_reject_bad_keywords_before_any_forward_pass():
    """No device, no network: predict on an object that is no more than its class, evaluate on a net that raises when it is used."""
    from votenet_amd import evaluator as E
    from votenet_amd import model as VM
    bare = VM.VoteNetHotPath.__new__(VM.VoteNetHotPath)

    class Untouchable:
        def predict(self, *a, **kw):
            raise AssertionError("evaluate called predict")
    for kw, text in BAD_KEYWORDS:
        with pytest.raises(L.InvalidArgumentError, match=text):
            bare.predict(None, **kw)
        with pytest.raises(L.InvalidArgumentError, match=text):
            E.evaluate(Untouchable(), [None], [None], **kw)
    with pytest.raises(L.InvalidArgumentError, match="protocol"):  # the protocol's own check still comes first
        bare.predict(None, protocol="paper", nms_overlap="aabb3d")


def test_evaluate_hands_the_keywords_to_predict_only_when_they_are_given():
    from votenet_amd import evaluator as E
    calls = []

    class Stop(Exception):
        pass

    class Net:
        def predict(self, *a, **kw):
            calls.append(kw)
            raise Stop
    for kw in (dict(), dict(protocol="per_class"), dict(protocol="per_class", nms_overlap="rotated"),
               dict(protocol="per_class", nms_overlap="aabb3d"), dict(protocol="per_class", nms_overlap="bev", nms_measure="over_later")):
        with pytest.raises(Stop):
            E.evaluate(Net(), [None], [None], **kw)
    assert [sorted(set(c) - {"next_x", "sync"}) for c in calls] == [[], ["protocol"], ["protocol"], ["nms_measure", "nms_overlap", "protocol"],
                                                                   ["nms_measure", "nms_overlap", "protocol"]]
    assert calls[3]["nms_overlap"] == "aabb3d" and calls[3]["nms_measure"] == "iou" and calls[4]["nms_measure"] == "over_later"
