"""CPU: the ground-truth selection's fixtures (tests/golden/select_boxes.npz, written by make_select_boxes_golden.py from the
reference's own sunutils functions and scipy's Delaunay), the numpy restatement the GPU tests compare the kernel with
(tests/select_boxes_ref.py), the host parsers (votenet_amd/sunrgbd.py) and what can be checked of the ABI and of the
Python entries without a device."""
import fnmatch
import os
import re

import numpy as np
import pytest

import select_boxes_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def fixture_scene(g, s, tag):
    """-> (subsampled float64 rows, slice of the scene's objects, the reference's results) of scene s, tag 'f64' / 'f32'."""
    raw = g["raw64_%d" % s] if tag == "f64" else g["raw32_%d" % s].astype(np.float64)
    n_out = int(g["n_out"])
    o0, o1 = g["obj_offset"][s], g["obj_offset"][s + 1]
    ref = {k: g["%s_%s_%d" % (k, tag, s)] for k in ("n_inside", "status", "center", "size", "heading", "cls")}
    ref["inside"] = np.unpackbits(g["inside_%s_%d" % (tag, s)], axis=1, count=n_out).astype(bool).reshape(o1 - o0, n_out)
    return raw[g["choice_%d" % s]], slice(o0, o1), ref


def restate(g, s, pts, sl):
    return SR.select_scene(pts, g["Rtilt"][s], g["K"][s], g["obj_cls"][sl], g["obj_box2d"][sl], g["obj_centroid"][sl],
                           g["obj_half_extent"][sl], g["obj_heading"][sl])


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_restatement_reproduces_the_reference_fixtures(golden, tag):
    """inside masks, counts, status and kept order exactly (no point is left out: zero within 1e-9 of a face or a 2D-box side
    disagree); size / heading / class exactly; centres within 1e-12 absolute: the reference forms a corner coordinate as a
    3-term BLAS dot plus one add and averages two corners, a handful of roundings at magnitude < 10 m is <= ~1e-14."""
    g = golden("select_boxes")
    tested = 0
    for s in range(int(g["b"])):
        pts, sl, ref = fixture_scene(g, s, tag)
        got = restate(g, s, pts, sl)
        differ = got["inside"] != ref["inside"]
        print("scene %d %s: %d objects, %d (point, object) pairs, %d differ, closest margin %.3g, max centre error %.3g"
              % (s, tag, len(ref["status"]), differ.size, differ.sum(), got["margin"].min() if differ.size else np.inf,
                 np.abs(got["center"] - ref["center"]).max() if len(ref["center"]) else 0.0))
        assert differ.sum() == 0
        tested += differ.size
        assert np.array_equal(got["n_inside"], ref["n_inside"]) and np.array_equal(got["status"], ref["status"])
        assert np.array_equal(got["cls"], ref["cls"]) and np.array_equal(got["size"], ref["size"])
        assert np.array_equal(got["heading"], ref["heading"])
        assert got["center"].shape == ref["center"].shape
        if len(ref["center"]):
            assert np.abs(got["center"] - ref["center"]).max() <= 1e-12
    assert tested > 100000


def test_fixtures_hold_the_cases_they_were_built_for(golden):
    g = golden("select_boxes")
    off = g["obj_offset"]
    st0, n0 = g["status_f64_0"], g["n_inside_f64_0"]
    assert list(st0) == [0, 0, 1, 2, 2, 3, 3, 3, 0, 0, 0]                   # whitelist, h = 0, h = 4e-8 | h = 6e-8, 3 4 | 5 6 points
    assert list(n0[6:10]) == [3, 4, 5, 6]
    assert list(g["obj_half_extent"][3:6, 2]) == [0.0, 4e-8, 6e-8]
    assert not np.allclose(g["Rtilt"][0], np.eye(3)) and np.array_equal(g["Rtilt"][1], np.eye(3))
    # the cut: without the 2D box the hull alone holds more points than the reference counted
    pts, sl, ref = fixture_scene(g, 0, "f64")
    obj = {k: g["obj_" + k][sl].copy() for k in ("cls", "box2d", "centroid", "half_extent", "heading")}
    obj["box2d"][:] = [-1e9, -1e9, 1e9, 1e9]
    wide = SR.select_scene(pts, g["Rtilt"][0], g["K"][0], **obj)
    assert wide["n_inside"][10] > ref["n_inside"][10] >= 5
    assert np.array_equal(wide["n_inside"][:2], ref["n_inside"][:2])
    # points behind the camera are counted where the reference counts them
    pts, sl, ref = fixture_scene(g, 1, "f64")
    assert (pts[ref["inside"][0], 1] < 0).sum() > 0
    assert off[3] - off[2] > 64                                               # more objects than one LDS pass of the kernel
    assert (g["status_f64_3"] != 0).all() and off[5] == off[4]                # a scene that keeps nothing; one with no labels
    assert g["raw64_0"].shape[1] == 6 and g["raw64_1"].shape[1] == 4


def test_parsers_give_the_fixture_arrays_exactly(golden):
    from votenet_amd import sunrgbd
    g = golden("select_boxes")
    lab = sunrgbd.parse_label(open(os.path.join(GOLD, "select_boxes_label.txt")).read())
    sl = slice(g["obj_offset"][0], g["obj_offset"][1])
    for k in ("cls", "box2d", "centroid", "half_extent", "heading"):
        assert lab[k].dtype == g["obj_" + k].dtype and np.array_equal(lab[k], g["obj_" + k][sl]), k
    assert lab["names"][2] == "lamp" and lab["cls"][2] == -1
    rt, km = sunrgbd.parse_calib(open(os.path.join(GOLD, "select_boxes_calib.txt")).read())
    assert np.array_equal(rt, g["Rtilt"][0]) and np.array_equal(km, g["K"][0])
    assert rt.flags["C_CONTIGUOUS"] and km[0, 2] == 365.0 and km[2, 0] == 0.0
    from votenet_amd import synth
    assert len(sunrgbd.CLASS_NAMES) == len(synth.MEAN_SIZES) == 10
    assert sunrgbd.CLASS_NAMES[:3] == ("bed", "table", "sofa") and sunrgbd.CLASS_NAMES[-1] == "bathtub"
    empty = sunrgbd.parse_label("")
    packed = sunrgbd.pack_objects([lab, empty, lab])
    assert list(packed["obj_offset"]) == [0, 11, 11, 22] and packed["box2d"].shape == (22, 4)
    assert np.array_equal(packed["heading"][11:], lab["heading"]) and packed["cls"].dtype == np.int32
    assert list(sunrgbd.pack_objects([empty])["obj_offset"]) == [0, 0]


def test_abi_declares_and_exports_select_boxes(hiplib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "votenet_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+votenet_select_boxes\s*\(", text) and re.search(r"\bsize_t\s+votenet_select_boxes_workspace_bytes\s*\(", text)
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "votenet_amd", "csrc", "exports.map")).read(), flags=re.S)
    globs = re.findall(r"^\s*([A-Za-z_*][\w*]*);", exports.split("local:")[0], flags=re.M)
    assert any(fnmatch.fnmatchcase("votenet_select_boxes", p) for p in globs), globs
    assert hiplib.votenet_select_boxes_workspace_bytes(8, 320) >= 320 * 4
    # the launcher validates before it touches the device: a null cloud is an invalid argument
    assert hiplib.votenet_select_boxes(*([1, 16] + [None] + [0, 3] + [None] * 2 + [0, 0] + [None] * 17 + [0, None])) == 1
    assert b"select_boxes" in hiplib.votenet_last_error()


def test_argument_checks_that_need_no_device(hiplib):
    import torch
    from votenet_amd import _lib, input_pipeline as IP, sunrgbd
    objects = sunrgbd.pack_objects([sunrgbd.parse_label("")])
    calib = [(np.eye(3), np.eye(3))]
    with pytest.raises(_lib.InvalidArgumentError):   # the cloud lives on the device
        IP.select_boxes(torch.zeros(100, 3), np.array([0, 100]), calib, objects, n_out=10)
    with pytest.raises(_lib.InvalidArgumentError):
        IP.select_boxes(np.zeros((100, 3)), np.array([0, 100]), calib, objects, n_out=10)
    with pytest.raises(_lib.InvalidArgumentError):   # one draw per input scene
        IP.build_batch(torch.zeros(100, 3), np.array([0, 100]), calib, objects, aug=IP.draw_augmentation(2), n_out=10)
    with pytest.raises(_lib.InvalidArgumentError):
        IP.build_batch(torch.zeros(100, 3), np.array([0, 100]), calib, objects, n_out=10)
