"""CPU: the oracle restatement against the committed golden vectors and, where the reference's
own compiled code is available (oracle/_ref), against that code directly."""
import hashlib

import numpy as np
import pytest

import cases


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_grouping_optest_golden(O, golden):
    c, g = cases.grouping_optest(), golden("grouping_optest")
    idx, cnt = O.query_ball_point(c["radius"], c["nsample"], c["xyz1"], c["xyz2"])
    assert (idx == g["idx"]).all() and (cnt == g["pts_cnt"]).all()
    assert (O.group_point(c["points"], idx) == g["out"]).all()
    assert (O.group_point_grad(c["points"], idx, c["grad_out"]) == g["grad"]).all()


def test_grouping_demo_golden(O, golden):
    c, g = cases.grouping_demo(), golden("grouping_demo")
    idx, cnt = O.query_ball_point(c["radius"], c["nsample"], c["xyz1"], c["xyz2"])
    assert sha(idx) == str(g["idx_sha"]) and (cnt == g["pts_cnt"]).all()
    assert sha(O.group_point(c["points"], idx)) == str(g["out_sha"])


def test_cfg1_golden(O, golden):
    g = golden("cfg1")
    xyz = cases.cfg1_cloud()
    fidx = O.farthest_point_sample(512, xyz)
    assert (fidx == g["fps_idx"]).all()
    new_xyz = O.gather_point(xyz, fidx)
    idx, cnt = O.query_ball_point(0.2, 32, xyz, new_xyz)
    assert (idx == g["idx"]).all() and (cnt == g["pts_cnt"]).all()
    assert sha(O.group_point(xyz, idx)) == str(g["grouped_xyz_sha"])


def test_interpolate_optest_golden(O, golden):
    c, g = cases.interpolate_optest(), golden("interpolate_optest")
    dist, idx = O.three_nn(c["xyz1"], c["xyz2"])
    assert (dist == g["dist"]).all() and (idx == g["idx"]).all()
    w = np.full_like(dist, 1.0 / 3.0)
    assert (O.three_interpolate(c["points"], idx, w) == g["out"]).all()
    assert (O.three_interpolate_grad(c["points"], idx, w, c["grad_out"]) == g["grad"]).all()
    assert (O.three_nn_weights(dist) == g["weights_idw"]).all()


def test_interpolate_demo_golden(O, golden):
    c, g = cases.interpolate_demo(), golden("interpolate_demo")
    dist, idx = O.three_nn(c["xyz1"], c["xyz2"])
    assert sha(dist) == str(g["dist_sha"]) and sha(idx) == str(g["idx_sha"])
    w = np.full_like(dist, 1.0 / 3.0)
    assert sha(O.three_interpolate(c["points"], idx, w)) == str(g["out_sha"])


def test_nms_smoke_known_answer(O, golden):
    """The reference's own smoke input (tf_nms3d.py:21-46) and its recorded output."""
    c, g = cases.nms_smoke(), golden("nms_smoke")
    assert (O.nms3d(c["bboxes"], c["scores"], c["objectiveness"], 0.5) == g["keep_050"]).all()
    assert (O.nms3d(c["bboxes"], c["scores"], c["objectiveness"], 0.25) == g["keep_025"]).all()
    assert abs(O.bev_intersection(c["bboxes"][0, 0], c["bboxes"][0, 1]) - float(g["bev_intersection"])) < 1e-6
    # volumes 1.0 / 0.512 -> iou = I3/(VA+VB-I3), I3 = 0.8 * 0.6227418
    i3 = 0.8 * float(g["bev_intersection"])
    assert abs(O.iou3d(c["bboxes"][0, 0], c["bboxes"][0, 1]) - i3 / (1.0 + 0.512 - i3)) < 1e-6


def test_nms_random_golden(O, golden):
    c, g = cases.nms_random(), golden("nms_random")
    for s in range(c["bboxes"].shape[0]):
        assert (O.iou3d_matrix(c["bboxes"][s]) == g["iou"][s]).all()
    assert (O.nms3d(c["bboxes"], c["scores"], c["objectiveness"], 0.25) == g["keep_025"]).all()
    assert (O.nms3d(c["bboxes"], c["scores"], c["objectiveness"], 0.5) == g["keep_050"]).all()


def test_fps_golden(O, golden):
    g = golden("fps_cases")
    for name, (xyz, m) in cases.fps_cases().items():
        assert (O.farthest_point_sample(m, xyz) == g[name]).all(), name


# ---- against the reference's compiled CPU code: its outputs stored in ref_build.npz (make_golden.py ref_build), and the code
# itself when oracle/_ref exists
@pytest.mark.parametrize("seed,b,n,m,r,k", cases.REF_BUILD_BALL)
def test_ball_query_vs_reference_build(O, golden, seed, b, n, m, r, k):
    g = golden("ref_build")
    xyz1, xyz2, pts, go = cases.ref_build_ball(seed, b, n, m, k)
    idx, cnt = O.query_ball_point(r, k, xyz1, xyz2)
    grouped, grad = O.group_point(pts, idx), O.group_point_grad(pts, idx, go)
    # a query without any hit is left untouched by the reference (pre-zeroed) and 0 in the oracle
    assert sha(idx) == str(g["ball%d_idx" % seed])
    assert sha(grouped) == str(g["ball%d_group" % seed])
    assert sha(grad) == str(g["ball%d_group_grad" % seed])
    if O.ref("grouping") is not None:
        assert (idx == O.ref_query_ball_point(r, k, xyz1, xyz2)).all()
        assert (grouped == O.ref_group_point(pts, idx)).all()
        assert (grad == O.ref_group_point_grad(pts, idx, go)).all()


@pytest.mark.parametrize("seed,b,n,m,c", cases.REF_BUILD_NN)
def test_three_nn_vs_reference_build(O, golden, seed, b, n, m, c):
    g = golden("ref_build")
    xyz1, xyz2, pts, go = cases.ref_build_nn(seed, b, n, m, c)
    dist, idx = O.three_nn(xyz1, xyz2)
    w = O.three_nn_weights(np.where(np.isfinite(dist), dist, 1.0).astype(np.float32))
    out, grad = O.three_interpolate(pts, idx, w), O.three_interpolate_grad(pts, idx, w, go)
    # includes the (inf, 0) fill when m < 3
    assert sha(idx) == str(g["nn%d_idx" % seed]) and sha(dist) == str(g["nn%d_dist" % seed])
    assert sha(out) == str(g["nn%d_interp" % seed])
    assert sha(grad) == str(g["nn%d_interp_grad" % seed])
    if O.ref("interpolate") is not None:
        rd, ri = O.ref_three_nn(xyz1, xyz2)
        assert (idx == ri).all() and (dist == rd).all()
        assert (out == O.ref_three_interpolate(pts, idx, w)).all()
        assert (grad == O.ref_three_interpolate_grad(pts, idx, w, go)).all()
