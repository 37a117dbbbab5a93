"""GPU: the axis-aligned NMS overlaps (libvotenet_aabb.so: votenet_aabb_overlap_matrix, votenet_class_nms_aabb;
votenet_amd/aabb_nms.py, the `nms_overlap` / `nms_measure` of VoteNetHotPath.predict / evaluator.evaluate).  The table is compared bit
for bit with the numpy float32 restatement of include/votenet_aabb_nms.h (tests/aabb_nms_ref.py); the NMS with
tests/detections_ref.class_nms3d over the DEVICE's table, so every decision is exact; scores to 1e-5 relative of their float64
evaluation, as tests/test_gpu_detections.py compares them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aabb_nms_ref as A  # noqa: E402
import detections_ref as R  # noqa: E402

import cases  # noqa: E402  (tests/golden, on the path by conftest.py)

pytestmark = pytest.mark.gpu

F = np.float32
NC = 10
TINY = 2.0 ** -126  # below fp32's smallest normal number a product has no 1e-5 relative precision to hold it to
ALL = [(mode, measure) for mode in A.MODES for measure in A.MEASURES]
FLAGS = [(cn, pc) for cn in (True, False) for pc in (True, False)]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def spoil(boxes):
    """Scene 0 of a batch of n >= 12 boxes gets the boxes of tests/test_aabb_nms_cpu.py's NaN and degenerate cases, in place."""
    s = boxes[0]
    s[1, 3, 0] = np.nan                      # a NaN in x, in y, in z: one coordinate each
    s[2, 6, 1] = np.nan
    s[3, 0, 2] = np.nan
    s[4] = np.nan                            # all NaN
    s[5] = 0.0                               # no volume: a point
    s[6, :, 1] = s[6, 0, 1]                  # no height: a volume of 0, a rectangle on the ground
    s[7] = np.where(s[7] > s[7].mean(0), F(np.inf), F(-np.inf))  # every extent infinite
    s[8, 0, 0] = np.inf                      # one infinite corner
    s[9] = s[0]                              # a copy of box 0: overlap 1
    s[10] = s[0] + F(0.01)                   # ... and a nudged one
    s[11] = s[5]                             # two boxes without volume: 0 / 0
    return boxes


def device_table(boxes, dev, mode, measure):
    from votenet_amd import aabb_nms
    t = aabb_nms.overlap_matrix(T(boxes, dev), mode, measure)
    assert t.dtype == torch.float32 and tuple(t.shape) == (boxes.shape[0], boxes.shape[1], boxes.shape[1])
    return t.cpu().numpy()


# ------------------------------------------------------------------ the overlap matrix
@pytest.mark.parametrize("n", [1, 65])
def test_overlap_matrix_equals_the_restatement_bit_for_bit(hiplib, dev, n):
    """65: a second tile of later boxes, of one box.  n = 1: scene 0 a random box, scene 1 a box without volume."""
    boxes = cases.nms_random(b=2, n=n, seed=11 + n, room=2.5)["bboxes"]
    if n == 1:
        boxes[1] = 0.0
    else:
        spoil(boxes)
    for mode, measure in ALL:
        got = device_table(boxes, dev, mode, measure)
        exp = A.overlap_table(boxes, mode, measure)
        diff = int((~((got == exp) | (np.isnan(got) & np.isnan(exp)))).sum())
        print("%s / %s, n = %d: %d of %d entries differ, %d NaN, %d above 0.25" % (mode, measure, n, diff, got.size, int(np.isnan(exp).sum()),
                                                                                 int((exp > 0.25).sum())))
        assert same_bits(got, exp), (mode, measure)
        if n > 1:
            assert np.isnan(exp[0, 4]).all() and np.isnan(exp[0]).sum() >= 2 * n and (exp[1] > 0.25).sum() > n and not np.isnan(exp[1]).any()


# ------------------------------------------------------------------ the NMS against the restatement
def check(boxes, obj, cls, dev, thr=0.25, conf=0.05, combos=ALL, flags=FLAGS):
    """class_nms_aabb on the device == detections_ref.class_nms3d over the device's own table, for every mode, measure and flag pair."""
    from votenet_amd import aabb_nms
    from votenet_amd import detections as D
    bb, ob, cs = T(boxes, dev), T(obj, dev), T(cls, dev)
    b, n, nc = cls.shape
    out = {}
    for mode, measure in combos:
        table = device_table(boxes, dev, mode, measure)
        for cn, pc in flags:
            det = aabb_nms.class_nms_aabb(bb, ob, cs, thr, conf, class_nms=cn, per_class=pc, overlap=mode, measure=measure)
            assert tuple(det["det_rows"].shape) == (b * n * (nc if pc else 1), 4) and det["det_rows"].dtype == torch.int32
            assert tuple(det["det_offset"].shape) == (b + 1,) and det["det_offset"].dtype == torch.int32
            scene, box, klass, score, offset = D.rows_to_host(det)
            exp = R.class_nms3d(table, obj, cls, thr, conf, class_nms=cn, per_class=pc)
            assert np.array_equal(offset, exp["det_offset"]), (mode, measure, cn, pc, offset, exp["det_offset"])
            assert np.array_equal(np.stack([scene, box, klass], 1), exp["rows"]), (mode, measure, cn, pc)
            assert score.dtype == np.float32
            assert np.allclose(score, exp["score"], rtol=1e-5, atol=TINY, equal_nan=True), (mode, measure, cn, pc)
            out[mode, measure, cn, pc] = exp
    return out


@pytest.mark.parametrize("b,n,nc", [(1, 1, 1), (2, 63, 10), (3, 64, 10), (2, 65, 3), (1, 512, 10)])
def test_class_nms_aabb_equals_the_restatement_over_the_device_table(hiplib, dev, b, n, nc):
    """63 / 64 / 65: either side of one word of the mask rows; 512: the limit, eight words, every LDS array full.  With two scenes or
    more the last has no candidate; with three, scene 1 is one tight cluster that its first box clears."""
    boxes = cases.nms_random(b=b, n=n, seed=5 * n + b, room=2.5 if n < 512 else 7.0)["bboxes"]
    rng = np.random.default_rng(n)
    obj = rng.normal(size=(b, n, 2)).astype(F) * 2
    cls = rng.normal(size=(b, n, nc)).astype(F) * 2
    if b >= 2:
        obj[b - 1] = np.array([9.0, 0.0], F)  # d = -9: below the threshold
    if b >= 3:
        for i in range(n):
            boxes[1, i] = cases.corner_box(1.0, 1.2, 0.9, 0.3, tuple(rng.normal(size=3) * 0.01)).astype(F)
        cls[1, :, 2] += 20.0
    out = check(boxes, obj, cls, dev)
    cand = int((R.margins(obj) > R.conf_logit(0.05)).sum())
    for mode, measure in ALL:
        by_class, across = out[mode, measure, True, False], out[mode, measure, False, False]
        assert all(len(r["kept"][b - 1]) == 0 for r in (by_class, across)) or b == 1
        if b >= 3:
            assert by_class["kept"][1] == [int(np.argmax(R.margins(obj)[1]))]
        if n > 1:  # the suppression and the class rule both did something
            a, c = by_class["det_offset"][-1], across["det_offset"][-1]
            assert 0 < c < cand and (c < a <= cand), (mode, measure, c, a, cand)
    if n > 1:  # ... and the modes and measures are not one table under four names
        kept = {k: out[k + (False, False)]["kept"] for k in ALL}
        assert kept["aabb3d", "iou"] != kept["bev", "iou"] and kept["aabb3d", "iou"] != kept["aabb3d", "over_later"]


def test_adversarial_inputs_and_nothing_written_beyond_the_total(hiplib, dev):
    """Scene 0: NaN, infinite and flat boxes among the candidates.  Scene 1: margins rounded to integers -- ties, broken by index.
    Scene 2: NaN margins (never candidates), rows of NaN class logits, some entries and whole rows.  The rows land in a buffer
    prefilled with a pattern: what lies beyond det_offset[b] is still the pattern."""
    from votenet_amd import _lib as L
    from votenet_amd import detections as D
    b, n, nc, thr = 3, 70, 4, 0.25
    boxes = spoil(cases.nms_random(b=b, n=n, seed=91, room=2.5)["bboxes"])
    rng = np.random.default_rng(6)
    obj = rng.normal(size=(b, n, 2)).astype(F) * 2
    cls = rng.normal(size=(b, n, nc)).astype(F)
    obj[0, :12] = np.array([0.0, 20.0], F) + rng.random((12, 1)).astype(F)  # the spoilt boxes are candidates, visited first,
    obj[0, 0] = np.array([0.0, 50.0], F)                                      # box 0 before its copies
    cls[0, :12, 1] += 20.0
    obj[1] = np.round(obj[1], 0)
    obj[2, ::7, 0] = np.nan
    obj[2, 3] = np.array([np.inf, np.inf], F)
    cls[2, 1::5, 2] = np.nan
    cls[2, 2::9] = np.nan
    d = R.margins(obj)
    assert len(np.unique(d[1])) < n // 3 and np.isnan(d[2]).sum() >= 10
    out = check(boxes, obj, cls, dev, thr)
    check(boxes, obj, cls, dev, thr, conf=0.0, combos=[("aabb3d", "iou")])
    exp = out["aabb3d", "iou", True, False]
    assert {1, 2, 3, 4, 5, 11} <= set(exp["kept"][0])  # NaN rows and columns, 0 / 0: kept, and they removed nothing ...
    assert 0 in exp["kept"][0] and 9 not in exp["kept"][0] and 10 not in exp["kept"][0]  # ... while box 0 removed its copies
    assert not any(np.isnan(d[2, i]) for i in exp["kept"][2]) and any(np.isnan(cls[2, i]).all() for i in exp["kept"][2])
    ties = [i for i in exp["kept"][1]]
    assert any(d[1, i] == d[1, j] and i < j for i, j in zip(ties, ties[1:]))  # equal margins in index order
    # the raw entry on a prefilled buffer
    lib = L.side_lib("aabb")
    bb, ob, cs = T(boxes, dev), T(obj, dev), T(cls, dev)
    for pc in (0, 1):
        cap = b * n * (nc if pc else 1)
        rows = torch.full((cap + 64, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        off = torch.full((b + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        need = lib.votenet_class_nms_aabb_workspace_bytes(b, n, nc)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        L.check(lib.votenet_class_nms_aabb(b, n, nc, L.ptr(bb), L.ptr(ob), L.ptr(cs), thr, float(D.conf_logit(0.05)), 1, pc, 0, 0,
                                           L.ptr(rows), cap, L.ptr(off), L.ptr(ws), need, L.stream_ptr()), side="aabb")
        want = out["aabb3d", "iou", True, bool(pc)]
        total = int(want["det_offset"][-1])
        assert 0 < total < cap and off.cpu().tolist() == want["det_offset"].tolist() + [0x5A5A5A5A]
        assert np.array_equal(rows[:total, :3].cpu().numpy(), want["rows"]) and bool((rows[total:] == 0x5A5A5A5A).all())


def test_two_runs_write_the_same_bytes(hiplib, dev):
    from votenet_amd import aabb_nms
    c = cases.nms_random(b=4, n=256, seed=33, room=5.0)
    rng = np.random.default_rng(0)
    bb, ob = T(c["bboxes"], dev), T(c["objectiveness"] * 2, dev)
    cs = T(rng.normal(size=(4, 256, NC)).astype(F), dev)
    for mode, measure in ALL:
        a, b2 = (aabb_nms.class_nms_aabb(bb, ob, cs, overlap=mode, measure=measure) for _ in range(2))
        total = int(a["det_offset"][-1])
        assert total > 0 and torch.equal(a["det_offset"], b2["det_offset"]) and torch.equal(a["det_rows"][:total], b2["det_rows"][:total])
        m1, m2 = (aabb_nms.overlap_matrix(bb, mode, measure) for _ in range(2))
        assert torch.equal(m1.view(torch.int32), m2.view(torch.int32))


def test_invalid_arguments_raise_and_launch_nothing(hiplib, dev):
    from votenet_amd import InvalidArgumentError, aabb_nms
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(InvalidArgumentError, match="at most 512 boxes per scene, got n = 513"):
        aabb_nms.class_nms_aabb(z(1, 513, 8, 3), z(1, 513, 2), z(1, 513, NC))
    with pytest.raises(InvalidArgumentError, match=r"classes must be in \[1, 64\], got 65"):
        aabb_nms.class_nms_aabb(z(1, 16, 8, 3), z(1, 16, 2), z(1, 16, 65))
    with pytest.raises(InvalidArgumentError, match=r"iou_threshold must be in \[0, 1\]"):
        aabb_nms.class_nms_aabb(z(1, 16, 8, 3), z(1, 16, 2), z(1, 16, NC), 1.5)
    for kw in (dict(overlap="rotated"), dict(overlap="hull"), dict(measure="giou")):
        with pytest.raises(InvalidArgumentError, match="overlap must be|measure must be"):
            aabb_nms.class_nms_aabb(z(1, 16, 8, 3), z(1, 16, 2), z(1, 16, NC), **kw)
        with pytest.raises(InvalidArgumentError, match="overlap must be|measure must be"):
            aabb_nms.overlap_matrix(z(1, 16, 8, 3), **kw)
    with pytest.raises(InvalidArgumentError, match="bbox shape"):
        aabb_nms.overlap_matrix(z(1, 16, 4, 3))
    assert tuple(aabb_nms.overlap_matrix(z(0, 16, 8, 3)).shape) == (0, 16, 16)


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


def same_rows(a, b):
    total = int(a["det_offset"][-1])
    return total > 0 and torch.equal(a["det_offset"], b["det_offset"]) and torch.equal(a["det_rows"][:total], b["det_rows"][:total])


def test_predict_with_an_overlap_is_class_nms_aabb_on_its_own_boxes(net, dev):
    from votenet_amd import aabb_nms
    from votenet_amd import box_points
    from votenet_amd import synth
    x = torch.from_numpy(synth.room_batch(2, NPTS, 90000)).to(dev)
    plain = net.predict(x, batch_statistics=True, protocol="per_class")
    for mode, measure in ALL:
        pred = net.predict(x, batch_statistics=True, protocol="per_class", nms_overlap=mode, nms_measure=measure)
        assert set(pred) == set(plain) and pred["det_rows"].shape == plain["det_rows"].shape
        obj = pred["proposals_output"][..., :2].contiguous()
        own = aabb_nms.class_nms_aabb(pred["bboxes"], obj, pred["class_scores"], overlap=mode, measure=measure)
        assert same_rows(own, pred), (mode, measure)
    pred = net.predict(x, batch_statistics=True, protocol=dict(conf_thresh=0.0, per_class=False), nms_overlap="bev")
    own = aabb_nms.class_nms_aabb(pred["bboxes"], pred["proposals_output"][..., :2].contiguous(), pred["class_scores"], conf_thresh=0.0,
                                  per_class=False, overlap="bev")
    assert same_rows(own, pred) and pred["det_rows"].shape[0] == 2 * 256
    # with min_points the NMS sees the gated logits
    pred = net.predict(x, batch_statistics=True, protocol="per_class", min_points=5, nms_overlap="aabb3d")
    assert set(pred) == set(plain) | {"point_counts"}
    gated = box_points.gate_objectness(pred["proposals_output"][..., :2].contiguous(), pred["point_counts"], 5)
    own = aabb_nms.class_nms_aabb(pred["bboxes"], gated, pred["class_scores"], overlap="aabb3d")
    assert same_rows(own, pred)
    cnt = pred["point_counts"].cpu().numpy()
    rows = pred["det_rows"][:int(pred["det_offset"][-1])].cpu().numpy()
    assert (cnt[rows[:, 0], rows[:, 1]] >= 5).all()
    assert not torch.isnan(pred["proposals_output"]).any()  # the network's own output, ungated


def test_predict_without_the_keywords_is_what_it_was(net, dev):
    """predict(...) and predict(..., nms_overlap="rotated", nms_measure="iou"): the same keys and the same tensors, bit for bit, and the
    per-class rows are detections.class_nms3d's (inference-mode BatchNorm: a scene's outputs are reproducible from call to call)."""
    from votenet_amd import detections as D
    from votenet_amd import synth
    x = torch.from_numpy(synth.room_batch(2, NPTS, 90002)).to(dev)
    for kw in (dict(), dict(sync=False), dict(protocol="per_class"), dict(protocol="per_class", min_points=5)):
        a, b = net.predict(x, **kw), net.predict(x, nms_overlap="rotated", nms_measure="iou", **kw)
        assert set(a) == set(b)
        valid = {}  # rows beyond the count are not written: only the rows that are
        if "nms_count" in a:
            valid["nms_idx"] = int(a["nms_count"])
        if "det_offset" in a:
            valid["det_rows"] = int(a["det_offset"][-1])
        for k in a:
            assert torch.equal(a[k][:valid.get(k)], b[k][:valid.get(k)]), (kw, k)
        assert all(v > 0 for v in valid.values())
    pred = net.predict(x, protocol="per_class")
    assert same_rows(D.class_nms3d(pred["bboxes"], pred["proposals_output"][..., :2].contiguous(), pred["class_scores"]), pred)
    for kw in (dict(nms_overlap="aabb3d"), dict(protocol="per_class", nms_overlap="hull"), dict(protocol="per_class", nms_measure="over_later")):
        with pytest.raises(ValueError, match="nms_overlap|nms_measure"):
            net.predict(x, **kw)


FRESH = """
import sys
sys.path.insert(0, %r)
import torch
from votenet_amd import _lib, synth
from votenet_amd.model import VoteNetHotPath
dev = torch.device("cuda:0")
net = VoteNetHotPath(dev, seed=0, npoints=(512, 256, 128, 64))
x = torch.from_numpy(synth.room_batch(1, 4096, 7)).to(dev)
for kw in (dict(), dict(protocol="per_class"), dict(protocol="per_class", nms_overlap="rotated")):
    net.predict(x, batch_statistics=True, **kw)
torch.cuda.synchronize()
maps = open("/proc/self/maps").read()
assert "libvotenet_hip.so" in maps and "libvotenet_detect.so" in maps
assert not _lib.side_loaded("aabb") and "libvotenet_aabb" not in maps
pred = net.predict(x, batch_statistics=True, protocol="per_class", nms_overlap="aabb3d")
assert "det_rows" in pred and "libvotenet_aabb" in open("/proc/self/maps").read()
print("fresh ok")
"""


def test_a_fresh_process_predict_does_not_load_the_new_library(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr


def test_evaluate_with_an_overlap_equals_the_restated_evaluation_of_its_rows(net, dev):
    """Two batches, the per-class protocol with the paper's overlap.  evaluate()'s predictions are recorded as it makes them; the
    restated evaluation (tests/detections_ref.py) runs on the rows the device wrote and the device's own ROTATED overlap table: the
    matcher's overlap is not the NMS's."""
    from votenet_amd import aabb_nms
    from votenet_amd import detections as D
    from votenet_amd import evaluator as E
    from votenet_amd import synth
    from votenet_amd import tf_nms3d
    thresholds = (0.25, 0.5)
    val_x = [torch.from_numpy(synth.room_batch(2, NPTS, 90000 + 2 * i)).to(dev) for i in range(2)]
    val_gt = [E.gt_for_eval(synth.room_gt(2, NPTS, 90000 + 2 * i)) for i in range(2)]
    seen, predict = [], net.predict

    def recording_predict(*a, **kw):
        assert kw.get("sync") is False and kw.get("protocol") == "per_class" and kw.get("nms_overlap") == "aabb3d" and kw.get("nms_measure") == "iou"
        seen.append(predict(*a, batch_statistics=True, **kw))
        return seen[-1]
    net.predict = recording_predict
    try:
        res = E.evaluate(net, val_x, val_gt, thresholds, protocol="per_class", nms_overlap=aabb_nms.PAPER_OVERLAP)
    finally:
        del net.predict
    assert len(seen) == 2
    scene, box, klass, score, tables, labels, count = [], [], [], [], [], [], []
    for i, (p, g) in enumerate(zip(seen, val_gt)):
        own = aabb_nms.class_nms_aabb(p["bboxes"], p["proposals_output"][..., :2].contiguous(), p["class_scores"])
        assert same_rows(own, p)
        s, b, k, sc, off = D.rows_to_host(p)
        scene.append(s + 2 * i), box.append(b), klass.append(k), score.append(sc)
        tables.append(tf_nms3d.iou3d_cross(p["bboxes"], T(g["boxes"], dev)).cpu().numpy())
        labels.append(g["labels"]), count.append(g["count"])
    G = max(t.shape[2] for t in tables)
    tables = [np.pad(t, ((0, 0), (0, 0), (0, G - t.shape[2]))) for t in tables]
    labels = [np.pad(l, ((0, 0), (0, G - l.shape[1])), constant_values=-1) for l in labels]
    args = (np.concatenate(scene), np.concatenate(box), np.concatenate(klass), np.concatenate(score), np.concatenate(tables),
            np.concatenate(labels), np.concatenate(count), NC)
    for thr in thresholds:
        exp = R.eval_rows(*args, thr)
        assert sorted(res[thr]["ap"]) == sorted(exp["ap"]) and len(exp["ap"]) > 0
        for c in exp["ap"]:
            assert not np.isnan(res[thr]["ap"][c]) and abs(res[thr]["ap"][c] - exp["ap"][c]) <= 1e-12, (thr, c)
        assert abs(res[thr]["mAP"] - exp["mAP"]) <= 1e-12
        print("per-class protocol, aabb3d overlap, thr %.2f: mAP %.4f over %d rows, %d true positives" % (thr, exp["mAP"], len(args[0]), int(exp["tp"].sum())))
