"""CPU: the points inside predicted boxes without a device -- the numpy float32 restatement of include/votenet_box_points.h
(tests/box_points_ref.py) against the reference's own hull test on the committed fixture (tests/golden/box_points.npz, written by
tests/golden/make_box_points_golden.py from sunutils.extract_pc_in_box3d), exactly representable cases for every clause of the rule,
the gate, and the C ABI entry points in the header, their derived binding, the library's export list and its argument checks."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_points_ref as R  # noqa: E402

import cases  # noqa: E402  (tests/golden, on the path by conftest.py)
from votenet_amd import _lib as L  # noqa: E402

F = np.float32
NAMES = ["votenet_box_point_counts", "votenet_box_points_last_error", "votenet_gate_objectness"]


# ------------------------------------------------------------------ the reference's hull test
def test_restatement_equals_the_references_hull_test_outside_the_margin(golden):
    """Scipy's hull tolerance (float64 barycentric coordinates against -eps) and the fp32 dot products cannot be held to agree on a
    point closer to a face than 1e-5 * max(ee_k, 1) in some t_k: those pairs -- at most 0.1 % -- are left out; every other pair agrees."""
    g = golden("box_points")
    boxes, points, npts = g["boxes"], g["points"], int(g["npts"])
    mask = np.unpackbits(g["inside"], axis=1)[:, :npts].astype(bool)
    assert boxes.shape == (40, 8, 3) and points.shape == (40, 2048, 3) and boxes.dtype == F and points.dtype == F
    size = np.linalg.norm(boxes[:, [1, 3, 4]] - boxes[:, :1], axis=2)
    assert size.min() >= 0.2 - 1e-6 and size.max() <= 1.7 + 1e-6
    pairs = left_out = wrong = 0
    for i in range(len(boxes)):
        ins = R.inside(boxes[i:i + 1], points[i])[0]
        near = R.near_face(boxes[i:i + 1], points[i])[0]
        pairs += ins.size
        left_out += int(near.sum())
        wrong += int(((ins != mask[i]) & ~near).sum())
    print("%d pairs, %d left out, %d disagree, %.2f %% inside" % (pairs, left_out, wrong, 100.0 * mask.mean()))
    assert wrong == 0
    assert left_out <= 0.001 * pairs
    assert mask.mean() >= 0.01


# ------------------------------------------------------------------ exactly representable cases
def dyadic_box():
    """Axis-aligned, dyadic corners: x in [-4, -2] (l = 2), y in [-2, -1] (h = 1), z in [-1, -0.5] (w = 0.5).
    c0 = (-2, -1, -0.5); e_0 = (0, 0, -0.5), e_1 = (-2, 0, 0), e_2 = (0, -1, 0); ee = (0.25, 4, 1).  Corner 0 is the corner nearest
    the origin, so q = p - c0 is exact for a point one float either side of EVERY face (beside c0 by Sterbenz' lemma; at the far
    faces |p| >= |q|, so q is on p's grid), the edges are powers of two, and every t below is exact: no rounding hides a neighbour."""
    return cases.corner_box(2.0, 0.5, 1.0, None, (-3.0, -1.5, -0.75)).astype(F)


def edge_points():
    """(points, inside) around dyadic_box(): every t exactly 0 or ee on a face, an edge, a corner; the next float outside of each."""
    lo, hi = np.array([-4.0, -2.0, -1.0], F), np.array([-2.0, -1.0, -0.5], F)
    mid = (lo + hi) / F(2)
    pts, exp = [], []
    for axis in range(3):
        for bound, away in ((lo, -np.inf), (hi, np.inf)):
            face = mid.copy()
            face[axis] = bound[axis]
            pts.append(face), exp.append(True)                      # on a face: t = 0 or t = ee
            out = face.copy()
            out[axis] = np.nextafter(bound[axis], F(away))
            pts.append(out), exp.append(False)                      # the next float outside
            inn = face.copy()
            inn[axis] = np.nextafter(bound[axis], F(-away))
            pts.append(inn), exp.append(True)                       # ... and inside
    for bx in (lo, hi):
        for by in (lo, hi):
            edge = np.array([bx[0], by[1], mid[2]], F)
            pts.append(edge), exp.append(True)                      # on an edge
            for bz in (lo, hi):
                corner = np.array([bx[0], by[1], bz[2]], F)
                pts.append(corner), exp.append(True)                # on a corner
                out = corner.copy()
                out[2] = np.nextafter(bz[2], F(np.inf if bz is hi else -np.inf))
                pts.append(out), exp.append(False)
    pts.append(mid), exp.append(True)
    return np.array(pts, F), np.array(exp, bool)


def test_closed_box_faces_edges_corners_and_the_next_float_outside():
    box = dyadic_box()
    c0, e, ee = R.box_constants(box)
    assert c0.tolist() == [-2.0, -1.0, -0.5] and ee.tolist() == [0.25, 4.0, 1.0]
    assert e.tolist() == [[0, 0, -0.5], [-2, 0, 0], [0, -1, 0]]
    pts, exp = edge_points()
    got = R.inside(box[None], pts)[0]
    assert np.array_equal(got, exp), np.nonzero(got != exp)
    assert R.counts(box[None, None], pts[None]).tolist() == [[int(exp.sum())]]
    t, _ = R.projections(box[None], pts)
    on = ((t[:, 0] == 0) | (t[:, 0] == ee[:, None])).any(0)
    assert (on & got).sum() >= 6 + 4 + 8  # the boundary points are exactly on it, and count


def test_nonfinite_points_and_boxes_count_nothing():
    box = dyadic_box()
    mid = [-3.0, -1.5, -0.75]
    bad = np.array([[np.nan, -1.5, -0.75], [-3.0, np.nan, -0.75], [-3.0, -1.5, np.nan], [np.inf, -1.5, -0.75], [-3.0, -np.inf, -0.75],
                    [np.inf, np.inf, np.inf], [-np.inf, np.inf, np.nan], mid], F)
    assert R.inside(box[None], bad)[0].tolist() == [False] * 7 + [True]
    for corner in (0, 1, 3, 4):  # a NaN in any coordinate of a corner that is read
        for axis in range(3):
            b2 = box.copy()
            b2[corner, axis] = np.nan
            assert not R.inside(b2[None], np.array([mid], F)).any(), (corner, axis)
    b2 = box.copy()
    b2[[2, 5, 6, 7]] = np.nan  # the corners that are not read
    assert R.inside(b2[None], np.array([mid], F)).all()


def test_zero_thickness_box_holds_its_own_plane():
    """h = 0: e_2 = 0, ee_2 = 0, t_2 = 0 for EVERY point -- 0 >= 0 and 0 <= 0 hold, so the third test says nothing and the box holds
    whatever lies in its l x w column, at any height.  The rule has no special case and this is what it says."""
    flat = cases.corner_box(2.0, 0.5, 0.0, None, (-3.0, -1.5, -0.75)).astype(F)
    _, e, ee = R.box_constants(flat)
    assert ee.tolist() == [0.25, 4.0, 0.0] and not e[2].any()
    pts = np.array([[-3.0, -1.5, -0.75], [-3.0, 7.0, -0.75], [-3.0, -3.0, -1.0], [-2.0, 0.0, -0.5], [-1.75, -1.5, -0.75], [-3.0, -1.5, -0.25],
                    [-3.0, np.inf, -0.75]], F)
    assert R.inside(flat[None], pts)[0].tolist() == [True, True, True, True, False, False, False]  # inf * 0 is NaN
    point = np.zeros((8, 3), F)  # every corner one point: all e = 0, every finite point is "inside"
    assert R.inside(point[None], np.array([[3.0, -2.0, 9.0], [np.nan, 0, 0]], F))[0].tolist() == [True, False]


# ------------------------------------------------------------------ the gate
def test_gate_rule_restated():
    rng = np.random.default_rng(0)
    obj = rng.normal(size=(2, 7, 2)).astype(F)
    obj[0, 0] = [np.inf, -0.0]
    obj.view(np.uint32)[0, 1] = [0x7fc00123, 0xffc00001]  # NaN payloads of a kept row survive
    cnt = np.array([[5, 9, 4, 0, 5, 6, 100], [0, 1, 2, 3, 4, 5, 6]], np.int32)
    g = R.gate(obj, cnt, 5)
    keep = cnt >= 5
    assert np.array_equal(g.view(np.uint32)[keep], obj.view(np.uint32)[keep])
    assert (g.view(np.uint32)[~keep] == 0x7fc00000).all() and np.isnan(g[~keep]).all()
    assert np.array_equal(R.gate(obj, cnt, 0).view(np.uint32), obj.view(np.uint32))
    assert keep.sum() == 7 and g is not obj


# ------------------------------------------------------------------ the C ABI
def test_header_declares_the_entries_and_the_binding_follows_it():
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, "votenet_box_points.h")) as f:
        protos = L.parse_header(f.read(), {})
    assert sorted(protos) == NAMES
    assert protos["votenet_box_points_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_box_point_counts"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_long] + [ctypes.c_void_p] * 4)
    assert protos["votenet_gate_objectness"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3)
    lib = L.side_lib("boxpts")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == (protos[name][0], protos[name][1])


def test_library_exports_exactly_its_header_and_checks_its_arguments(hiplib):
    """Every invalid-argument case returns 1 before anything is launched, with the limit in the text: no device is needed."""
    lib = L.side_lib("boxpts")
    defined = lambda path: [line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                                                                        check=True).stdout.splitlines()]
    assert sorted(defined(L.side_path("boxpts"))) == NAMES
    for other in (L.lib_path(), L.side_path("detect")):  # the other libraries export what they did
        assert not set(NAMES) & set(defined(other))
    buf = np.zeros(4096, F)
    p = buf.ctypes.data
    err = lambda: lib.votenet_box_points_last_error().decode()

    def count(b=2, n=16, npts=64, boxes=p, points=p, counts=p):
        return lib.votenet_box_point_counts(b, n, npts, boxes, points, counts, None)
    for kw, text in ((dict(n=0), "1 to 1024 boxes"), (dict(n=1025), "1 to 1024 boxes per scene, got n = 1025"), (dict(npts=-1), "[0, 2^24)"),
                     (dict(npts=2 ** 24), "[0, 2^24), got npts = 16777216"), (dict(b=-1), "[0, 65535], got -1"), (dict(b=65536), "[0, 65535]"),
                     (dict(boxes=None), "null"), (dict(points=None), "null points"), (dict(counts=None), "null")):
        assert count(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert count(b=0) == 0 and count(b=0, boxes=None, points=None, counts=None) == 0  # launches nothing

    def gate(b=2, n=16, counts=p, mp=5, obj=p, gated=p + 8192):
        return lib.votenet_gate_objectness(b, n, counts, mp, obj, gated, None)
    for kw, text in ((dict(n=0), "1 to 1024 boxes"), (dict(n=1025), "1 to 1024 boxes"), (dict(b=-1), "[0, 65535]"), (dict(mp=-1), "min_points must be >= 0, got -1"),
                     (dict(counts=None), "null"), (dict(obj=None), "null"), (dict(gated=None), "null"), (dict(gated=p), "may not alias"),
                     (dict(gated=p + 8), "may not alias"), (dict(obj=p + 8192 + 2 * 16 * 8 - 8), "may not alias")):
        assert gate(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert gate(b=0) == 0
    with pytest.raises(L.InvalidArgumentError, match=r"1 to 1024 boxes per scene, got n = 1025"):
        L.check(count(n=1025), side="boxpts")


def test_build_force_also_removes_the_boxpts_library_and_its_objects(monkeypatch, tmp_path):
    from votenet_amd import _lib
    here = tmp_path / "votenet_amd"
    (here / "csrc" / "boxpts" / "obj").mkdir(parents=True)
    (here / "lib").mkdir()
    for f in (here / "csrc" / "boxpts" / "obj" / "box_points.o", here / "lib" / "libvotenet_boxpts.so", here / "lib" / "libvotenet_hip.so"):
        f.write_bytes(b"stale")
    seen = {}

    def fake_run(cmd, **kw):
        seen["left"] = sorted(p.name for d in ("csrc/boxpts/obj", "lib") for p in (here / d).iterdir())
        return subprocess.CompletedProcess(cmd, 0, "", "")
    monkeypatch.setattr(_lib, "_HERE", str(here))
    monkeypatch.setattr(_lib, "_LIB_PATH", str(here / "lib" / "libvotenet_hip.so"))
    monkeypatch.setattr(_lib.subprocess, "run", fake_run)
    _lib.build(force=True)
    assert seen["left"] == []
