"""GPU: the points inside predicted boxes and the empty-box gate (libvotenet_boxpts.so: votenet_box_point_counts,
votenet_gate_objectness; votenet_amd/box_points.py, the `min_points` of VoteNetHotPath.predict / evaluator.evaluate) against the numpy
float32 restatement of include/votenet_box_points.h (tests/box_points_ref.py).  The rule is fp32 arithmetic in a fixed order and the
counts are integers: every comparison of counts is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_points_ref as R  # noqa: E402
import detections_ref as DR  # noqa: E402
from test_box_points_cpu import dyadic_box, edge_points  # noqa: E402  (the exactly representable cases)

import cases  # noqa: E402  (tests/golden, on the path by conftest.py)

pytestmark = pytest.mark.gpu

F = np.float32
NC = 10
ROOM = np.array([4.0, 1.5, 4.0])
GARBAGE = 0x5A5A5A5A


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def draw(b, n, npts, seed):
    """Boxes at random centres, sizes 0.2 .. 1.7 and headings in a room; half of each scene's points uniform over the room, half in
    clumps on the centres of a few boxes: boxes hold between no point and hundreds."""
    from votenet_amd import evaluator as E
    rng = np.random.default_rng(seed)
    center = rng.random((b, n, 3)) * ROOM
    boxes = E.box_corners(center, rng.uniform(0.2, 1.7, (b, n, 3)), rng.uniform(0, 2 * np.pi, (b, n)))
    pts = rng.random((b, npts, 3)) * ROOM
    half = npts // 2
    if half:
        pick = rng.integers(0, min(n, 4), (b, half))
        pts[:, :half] = center[np.arange(b)[:, None], pick] + rng.normal(size=(b, half, 3)) * 0.15
    return boxes.astype(F), pts.astype(F)


# ------------------------------------------------------------------ the counts
@pytest.mark.parametrize("b,n,npts", [(1, 1, 1), (1, 1, 0), (2, 63, 65), (3, 64, 257), (2, 65, 1000), (1, 1024, 513), (8, 256, 2048)])
def test_counts_equal_the_restatement(hiplib, dev, b, n, npts):
    """63 / 64 / 65 boxes: either side of one 64-box flush; 65 / 257 / 513 / 1000 points: tails of the wave and of the 512-point tile,
    one to four tiles; 1024 boxes: the limit, eight LDS chunks; 8 x 256 x 2048: the model's boxes."""
    from votenet_amd import box_points as BP
    boxes, pts = draw(b, n, npts, 11 * n + npts)
    if npts == 1:
        pts[0, 0] = boxes[0, 0].mean(0)  # the one point, in the one box
    got = BP.box_point_counts(T(boxes, dev), T(pts, dev))
    assert got.dtype == torch.int32 and tuple(got.shape) == (b, n) and got.is_cuda
    exp = R.counts(boxes, pts)
    got = got.cpu().numpy()
    print("(%d, %d, %d): counts %d .. %d, %d boxes empty" % (b, n, npts, exp.min(), exp.max(), int((exp == 0).sum())))
    assert np.array_equal(got, exp)
    if npts == 1:
        assert exp.tolist() == [[1]]
    if npts >= 1000:
        assert exp.min() == 0 and exp.max() >= 100
    assert int(exp.sum()) > 0 or npts == 0


def adversarial():
    """One scene, 1500 points (three tiles, the last of 476), 70 boxes.  Box 0 holds every finite point (its count is summed across
    every tile and wave); boxes 1-3 are one box three times; box 4 is the dyadic box with its face / edge / corner points and their
    neighbours; box 5 has a NaN corner, box 6 is box 3 with NaN in the corners that are not read; NaN / Inf points at 0, 63, 64 and npts - 1."""
    npts, n = 1500, 70
    boxes, pts = draw(1, n, npts, 99)
    boxes[0, 0] = cases.corner_box(64.0, 64.0, 64.0).astype(F)
    boxes[0, 1] = boxes[0, 2] = boxes[0, 3]
    boxes[0, 4] = dyadic_box()
    boxes[0, 5, 3, 2] = np.nan
    boxes[0, 6] = boxes[0, 3]
    boxes[0, 6, [2, 5, 6, 7]] = np.nan
    edge, _ = edge_points()
    pts[0, 100:100 + len(edge)] = edge
    pts[0, 600:600 + len(edge)] = edge  # ... in the second tile as well
    pts[0, 0] = [np.nan, 1.0, 1.0]
    pts[0, 63] = [1.0, np.inf, 1.0]
    pts[0, 64] = [-np.inf, np.nan, np.inf]
    pts[0, npts - 1] = [np.nan, np.nan, np.nan]
    return boxes, pts, len(edge)


def test_adversarial_scene(hiplib, dev):
    from votenet_amd import box_points as BP
    boxes, pts, nedge = adversarial()
    exp = R.counts(boxes, pts)
    got = BP.box_point_counts(T(boxes, dev), T(pts, dev)).cpu().numpy()
    assert np.array_equal(got, exp)
    npts = pts.shape[1]
    assert exp[0, 0] == npts - 4                      # every finite point
    assert exp[0, 1] == exp[0, 2] == exp[0, 3] > 0    # the duplicates
    assert exp[0, 4] == 2 * int(edge_points()[1].sum()) and nedge > exp[0, 4] // 2  # the closed box, twice
    assert exp[0, 5] == 0 and exp[0, 6] == exp[0, 3]  # a NaN corner that is read; NaN corners that are not


def test_the_committed_fixture_equals_its_reference_mask_outside_the_margin(hiplib, dev, golden):
    """One box per scene with its own 2 048 points.  The pairs within 1e-5 * max(ee_k, 1) of a face (tests/test_box_points_cpu.py: at
    most 0.1 %) are taken out of the cloud (NaN); the count of every box is then the reference's membership of the rest, exactly."""
    from votenet_amd import box_points as BP
    g = golden("box_points")
    boxes, pts, npts = g["boxes"][:, None].copy(), g["points"].copy(), int(g["npts"])
    mask = np.unpackbits(g["inside"], axis=1)[:, :npts].astype(bool)
    near = np.stack([R.near_face(boxes[i], pts[i])[0] for i in range(len(boxes))])
    assert near.sum() <= 0.001 * near.size
    pts[near] = np.nan
    got = BP.box_point_counts(T(boxes, dev), T(pts, dev)).cpu().numpy()
    exp = (mask & ~near).sum(1)
    assert np.array_equal(got[:, 0], exp) and exp.sum() >= 0.01 * mask.size


def test_two_calls_write_the_same_bytes_and_overwrite_garbage(hiplib, dev):
    from votenet_amd import _lib as L
    boxes, pts = draw(8, 256, 2048, 5)
    bb, pp = T(boxes, dev), T(pts, dev)
    lib = L.side_lib("boxpts")
    outs = []
    for fill in (GARBAGE, -1):
        counts = torch.full((8, 256), fill, dtype=torch.int32, device=dev)
        L.check(lib.votenet_box_point_counts(8, 256, 2048, L.ptr(bb), L.ptr(pp), L.ptr(counts), L.stream_ptr()), side="boxpts")
        outs.append(counts)
    assert torch.equal(outs[0], outs[1]) and np.array_equal(outs[0].cpu().numpy(), R.counts(boxes, pts))
    counts = torch.full((8, 256), GARBAGE, dtype=torch.int32, device=dev)  # no points: zeros, written in full
    L.check(lib.votenet_box_point_counts(8, 256, 0, L.ptr(bb), None, L.ptr(counts), L.stream_ptr()), side="boxpts")
    assert not counts.any()


def test_invalid_arguments_raise_and_launch_nothing(hiplib, dev):
    from votenet_amd import InvalidArgumentError, box_points as BP
    z = lambda *s, **kw: torch.zeros(*s, device=dev, **kw)
    with pytest.raises(InvalidArgumentError, match="1 to 1024 boxes per scene, got n = 1025"):
        BP.box_point_counts(z(1, 1025, 8, 3), z(1, 16, 3))
    with pytest.raises(InvalidArgumentError, match="bbox shape"):
        BP.box_point_counts(z(1, 16, 4, 3), z(1, 16, 3))
    with pytest.raises(InvalidArgumentError, match="points shape"):
        BP.box_point_counts(z(2, 16, 8, 3), z(1, 16, 3))
    with pytest.raises(InvalidArgumentError, match="points shape"):
        BP.box_point_counts(z(1, 16, 8, 3), z(1, 16, 4))
    with pytest.raises(InvalidArgumentError, match="float32"):
        BP.box_point_counts(z(1, 16, 8, 3), z(1, 16, 3, dtype=torch.float64))
    with pytest.raises(InvalidArgumentError, match="int32 counts"):
        BP.gate_objectness(z(1, 16, 2), z(1, 16, dtype=torch.int64), 5)
    with pytest.raises(InvalidArgumentError, match="int32 counts"):
        BP.gate_objectness(z(1, 16, 2), z(1, 15, dtype=torch.int32), 5)
    with pytest.raises(InvalidArgumentError, match="min_points must be >= 0, got -1"):
        BP.gate_objectness(z(1, 16, 2), z(1, 16, dtype=torch.int32), -1)
    with pytest.raises(InvalidArgumentError, match="integer"):
        BP.gate_objectness(z(1, 16, 2), z(1, 16, dtype=torch.int32), 2.5)
    assert BP.PAPER_MIN_POINTS == 5


# ------------------------------------------------------------------ the gate
def clear_of(table, thr):
    with np.errstate(invalid="ignore"):
        return not (np.abs(table - np.float32(thr)) < 1e-5).any()


@pytest.fixture(scope="module")
def gated_scene(hiplib, dev):
    """3 scenes x 96 crowded boxes (cases.nms_random) and a cloud in clumps: about half of the boxes hold fewer than 5 points."""
    from votenet_amd import box_points as BP
    from votenet_amd import tf_nms3d
    b, n, thr = 3, 96, 0.25
    for k in range(50):
        c = cases.nms_random(b=b, n=n, seed=17 + 1000 * k, room=3.0)
        iou = tf_nms3d.iou3d_matrix(T(c["bboxes"], dev)).cpu().numpy()
        if clear_of(iou, thr):  # a condition on the inputs, as in tests/test_gpu_detections.py
            break
    else:
        raise AssertionError("no seed found")
    rng = np.random.default_rng(3)
    boxes = c["bboxes"]
    ctr = boxes.mean(2)  # (b, n, 3)
    pick = rng.integers(0, n // 8, (b, 240))  # tight clumps on the centres of the first 12 boxes only
    pts = (ctr[np.arange(b)[:, None], pick] + rng.normal(size=(b, 240, 3)) * 0.04).astype(F)
    obj = (rng.normal(size=(b, n, 2)) * 2).astype(F)
    cls = (rng.normal(size=(b, n, NC)) * 2).astype(F)
    counts = BP.box_point_counts(T(boxes, dev), T(pts, dev))
    cnt = counts.cpu().numpy()
    assert np.array_equal(cnt, R.counts(boxes, pts))
    empty = cnt < 5
    assert empty.sum(1).min() >= 10 and (~empty).sum(1).min() >= 10
    assert (empty & (obj[..., 1] > obj[..., 0])).sum() >= 10  # empty boxes that would have been candidates
    return dict(boxes=boxes, obj=obj, cls=cls, iou=iou, thr=thr, counts=counts, cnt=cnt, empty=empty)


def test_gate_keeps_bits_and_writes_nan(gated_scene, dev):
    from votenet_amd import box_points as BP
    s = gated_scene
    obj = s["obj"].copy()
    obj[0, 0] = [np.inf, -0.0]
    obj.view(np.uint32)[0, 1] = [0x7fc00123, 0xffc00001]  # NaN payloads: a copy of the bits
    o = T(obj, dev)
    for mp in (0, 1, 5, 10 ** 6):
        g = BP.gate_objectness(o, s["counts"], mp)
        assert g.data_ptr() != o.data_ptr() and g.dtype == torch.float32 and tuple(g.shape) == obj.shape
        assert np.array_equal(g.cpu().numpy().view(np.uint32), R.gate(obj, s["cnt"], mp).view(np.uint32)), mp
    g0 = BP.gate_objectness(o, s["counts"], 0).cpu().numpy()
    assert np.array_equal(g0.view(np.uint32), obj.view(np.uint32))  # an exact copy
    g5 = BP.gate_objectness(o, s["counts"], 5).cpu().numpy()
    assert np.isnan(g5[s["empty"]]).all() and np.array_equal(g5.view(np.uint32)[~s["empty"]], obj.view(np.uint32)[~s["empty"]])
    assert np.isnan(BP.gate_objectness(o, s["counts"], 10 ** 6).cpu().numpy()).all()
    # the input is not touched: compared as bits, because obj holds NaNs and NaN == NaN is false
    assert np.array_equal(o.cpu().numpy().view(np.uint32), obj.view(np.uint32))


@pytest.mark.parametrize("class_nms,per_class,conf", [(True, True, 0.05), (False, False, 0.0), (True, False, 0.5)])
def test_class_nms3d_on_gated_logits_is_the_restatement_without_the_empty_boxes(gated_scene, dev, class_nms, per_class, conf):
    """The restatement (tests/detections_ref.py) runs per scene on the NON-EMPTY boxes only -- their rows and columns of the device's
    overlap table, their logits -- and its box numbers are mapped back."""
    from votenet_amd import box_points as BP
    from votenet_amd import detections as D
    s = gated_scene
    gated = BP.gate_objectness(T(s["obj"], dev), s["counts"], 5)
    det = D.class_nms3d(T(s["boxes"], dev), gated, T(s["cls"], dev), s["thr"], conf, class_nms=class_nms, per_class=per_class)
    scene, box, klass, score, offset = D.rows_to_host(det)
    rows, scores, exp_offset = [], [], [0]
    for k in range(s["boxes"].shape[0]):
        idx = np.nonzero(~s["empty"][k])[0]
        sub = DR.class_nms3d(s["iou"][k][np.ix_(idx, idx)][None], s["obj"][k, idx][None], s["cls"][k, idx][None], s["thr"], conf,
                             class_nms=class_nms, per_class=per_class)
        rows += [(k, int(idx[bx]), int(c)) for _, bx, c in sub["rows"]]
        scores.append(sub["score"])
        exp_offset.append(len(rows))
    assert np.array_equal(offset, exp_offset) and len(rows) > 0
    assert np.stack([scene, box, klass], 1).tolist() == [list(r) for r in rows]
    assert np.allclose(score, np.concatenate(scores), rtol=1e-5, atol=2.0 ** -126)
    assert not s["empty"][scene, box].any()
    plain = D.rows_to_host(D.class_nms3d(T(s["boxes"], dev), T(s["obj"], dev), T(s["cls"], dev), s["thr"], conf, class_nms=class_nms,
                                         per_class=per_class))
    assert s["empty"][plain[0], plain[1]].any()  # without the gate, empty boxes are among the detections


def test_nms3d_on_gated_logits_keeps_no_empty_box_and_the_rest_as_if_they_were_no_objects(gated_scene, dev):
    from votenet_amd import box_points as BP
    from votenet_amd import tf_nms3d
    s = gated_scene
    bb, score = T(s["boxes"], dev), T(s["cls"].max(-1), dev)
    gated = BP.gate_objectness(T(s["obj"], dev), s["counts"], 5)
    keep = tf_nms3d.NMS3D(bb, score, gated, s["thr"]).cpu().numpy()
    assert len(keep) > 0 and not s["empty"][keep[:, 0], keep[:, 1]].any()
    off = s["obj"].copy()
    off[s["empty"]] = [1.0, 0.0]  # "not an object": o1 > o0 is false
    want = tf_nms3d.NMS3D(bb, score, T(off, dev), s["thr"]).cpu().numpy()
    assert np.array_equal(keep, want)
    plain = tf_nms3d.NMS3D(bb, score, T(s["obj"], dev), s["thr"]).cpu().numpy()
    assert s["empty"][plain[:, 0], plain[:, 1]].any()
    padded, count = tf_nms3d.NMS3D(bb, score, gated, s["thr"], padded=True)
    assert int(count) == len(keep) and np.array_equal(padded[:len(keep)].cpu().numpy(), keep)


# ------------------------------------------------------------------ the whole path
NPTS = 20480


@pytest.fixture(scope="module")
def net(hiplib, dev):
    """A VoteNet after a few training steps on synthetic rooms (the fixture of tests/test_gpu_detections.py)."""
    from votenet_amd import loss as VL
    from votenet_amd import synth
    from votenet_amd.model import VoteNetHotPath
    net = VoteNetHotPath(dev, seed=0)
    net.init_optimizer(1e-3)
    x = torch.from_numpy(synth.room_batch(2, NPTS, 5000)).to(dev)
    gt = VL.gt_to_device(synth.room_gt(2, NPTS, 5000), dev)
    for _ in range(20):
        net.train_step(x, gt=gt)
    torch.cuda.synchronize()
    return net


def cloud(dev, seed):
    """A synthetic room with four stray points far outside it, 10 m apart: farthest point sampling makes each a seed, a vote and a
    proposal, and the box decoded there holds one point at the most -- boxes that the gate must drop, beside the room's own."""
    from votenet_amd import synth
    x = synth.room_batch(2, NPTS, seed)
    x[:, :4] = np.array([[30.0, 0.5, 30.0], [40.0, 0.5, 30.0], [30.0, 0.5, 40.0], [40.0, 0.5, 40.0]], F)
    return torch.from_numpy(x).to(dev)


@pytest.mark.parametrize("protocol", ["reference", "per_class"])
def test_predict_with_min_points_drops_the_empty_boxes(net, dev, protocol):
    from votenet_amd import box_points as BP
    from votenet_amd import detections as D
    x = cloud(dev, 90000)
    pred = net.predict(x, batch_statistics=True, protocol=protocol, min_points=5)
    plain = net.predict(x, batch_statistics=True, protocol=protocol)
    assert set(pred) == set(plain) | {"point_counts"}
    counts = pred["point_counts"]
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (2, 256)
    assert torch.equal(counts, BP.box_point_counts(pred["bboxes"], x))
    cnt = counts.cpu().numpy()
    assert np.array_equal(cnt, R.counts(pred["bboxes"].cpu().numpy(), x.cpu().numpy()))
    assert not torch.isnan(pred["proposals_output"]).any()  # the network's own output, ungated
    if protocol == "reference":
        named = pred["nms_idx"].cpu().numpy()
        scene, box = named[:, 0], named[:, 1]
        padded = net.predict(x, batch_statistics=True, sync=False, min_points=5)
        k = int(padded["nms_count"])
        assert k == len(named) and "point_counts" in padded and padded["nms_idx"].shape[0] == 2 * 256
    else:
        scene, box = D.rows_to_host(pred)[:2]
    print("%s: %d of 512 boxes hold fewer than 5 points, %d rows" % (protocol, int((cnt < 5).sum()), len(box)))
    assert len(box) > 0 and (cnt[scene, box] >= 5).all()
    assert (cnt < 5).any() and (cnt >= 5).any()  # at least one box dropped, at least one kept


def test_predict_without_min_points_is_what_it_was(net, dev):
    """predict() and predict(min_points=0): the same keys and the same tensors, bit for bit (inference-mode BatchNorm: a scene's
    outputs are reproducible from call to call, tests/test_gpu_model.py)."""
    x = cloud(dev, 90002)
    for kw in (dict(), dict(sync=False), dict(protocol="per_class")):
        a, b = net.predict(x, **kw), net.predict(x, min_points=0, **kw)
        assert set(a) == set(b) and "point_counts" not in a
        valid = {}  # rows beyond the count are not written: only the rows that are
        if "nms_count" in a:
            valid["nms_idx"] = int(a["nms_count"])
        if "det_offset" in a:
            valid["det_rows"] = int(a["det_offset"][-1])
        for k in a:
            assert torch.equal(a[k][:valid.get(k)], b[k][:valid.get(k)]), (kw, k)
        assert all(v > 0 for v in valid.values())
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="min_points"):
            net.predict(x, min_points=bad)


FRESH = """
import sys
sys.path.insert(0, %r)
import torch
from votenet_amd import _lib, synth
from votenet_amd.model import VoteNetHotPath
dev = torch.device("cuda:0")
net = VoteNetHotPath(dev, seed=0, npoints=(512, 256, 128, 64))
x = torch.from_numpy(synth.room_batch(1, 4096, 7)).to(dev)
for kw in (dict(), dict(protocol="per_class")):
    net.predict(x, batch_statistics=True, **kw)
torch.cuda.synchronize()
maps = open("/proc/self/maps").read()
assert "libvotenet_hip.so" in maps and "libvotenet_detect.so" in maps
assert not _lib.side_loaded("boxpts") and "libvotenet_boxpts" not in maps and "votenet_amd.box_points" not in sys.modules
pred = net.predict(x, batch_statistics=True, min_points=5)
assert "point_counts" in pred and "libvotenet_boxpts" in open("/proc/self/maps").read()
print("fresh ok")
"""


def test_a_fresh_process_predict_does_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr


def test_evaluate_with_min_points_equals_the_restated_evaluation_of_its_rows(net, dev):
    """Two batches, the per-class protocol with min_points=5.  evaluate()'s predictions are recorded as it makes them; the restated
    evaluation (tests/detections_ref.py) runs on the rows the device wrote and the device's own overlap table."""
    from votenet_amd import detections as D
    from votenet_amd import evaluator as E
    from votenet_amd import synth
    from votenet_amd import tf_nms3d
    thresholds = (0.25, 0.5)
    val_x = [cloud(dev, 90000 + 2 * i) for i in range(2)]
    val_gt = [E.gt_for_eval(synth.room_gt(2, NPTS, 90000 + 2 * i)) for i in range(2)]
    seen, predict = [], net.predict

    def recording_predict(*a, **kw):
        assert kw.get("sync") is False and kw.get("protocol") == "per_class" and kw.get("min_points") == 5
        seen.append(predict(*a, batch_statistics=True, **kw))
        return seen[-1]
    net.predict = recording_predict
    try:
        res = E.evaluate(net, val_x, val_gt, thresholds, protocol="per_class", min_points=5)
    finally:
        del net.predict
    assert len(seen) == 2
    scene, box, klass, score, tables, labels, count = [], [], [], [], [], [], []
    for i, (p, g) in enumerate(zip(seen, val_gt)):
        s, b, k, sc, off = D.rows_to_host(p)
        cnt = p["point_counts"].cpu().numpy()
        assert off[-1] > 0 and (cnt[s, b] >= 5).all() and (cnt < 5).any()
        scene.append(s + 2 * i), box.append(b), klass.append(k), score.append(sc)
        tables.append(tf_nms3d.iou3d_cross(p["bboxes"], T(g["boxes"], dev)).cpu().numpy())
        labels.append(g["labels"]), count.append(g["count"])
    G = max(t.shape[2] for t in tables)
    tables = [np.pad(t, ((0, 0), (0, 0), (0, G - t.shape[2]))) for t in tables]
    labels = [np.pad(l, ((0, 0), (0, G - l.shape[1])), constant_values=-1) for l in labels]
    args = (np.concatenate(scene), np.concatenate(box), np.concatenate(klass), np.concatenate(score), np.concatenate(tables),
            np.concatenate(labels), np.concatenate(count), NC)
    for thr in thresholds:
        exp = DR.eval_rows(*args, thr)
        assert sorted(res[thr]["ap"]) == sorted(exp["ap"]) and len(exp["ap"]) > 0
        for c in exp["ap"]:
            assert not np.isnan(res[thr]["ap"][c]) and abs(res[thr]["ap"][c] - exp["ap"][c]) <= 1e-12, (thr, c)
        assert abs(res[thr]["mAP"] - exp["mAP"]) <= 1e-12
    # min_points = 0 is evaluate() as it was: predict is called without the argument
    calls = []
    net.predict = lambda *a, **kw: calls.append(kw) or predict(*a, batch_statistics=True, **kw)
    try:
        E.evaluate(net, val_x[:1], val_gt[:1], thresholds, protocol="per_class")
    finally:
        del net.predict
    assert calls and all("min_points" not in kw for kw in calls)
