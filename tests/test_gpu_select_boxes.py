"""GPU: votenet_select_boxes / input_pipeline.select_boxes / build_batch against the reference's fixtures
(tests/golden/select_boxes.npz) and the numpy restatement (tests/select_boxes_ref.py).
Bar: inside masks, counts, status, kept order, size / heading / class exact; centres within 1e-12 absolute (a handful of
float64 roundings at magnitude < 10 m is <= ~1e-14).  A point may be left out of the `inside` comparison only if the
restatement puts it within 1e-9 of a box face (normalised) or of a 2D-box side (pixels); at most 1e-4 of the tested
points, and none for an object whose reference count is 3-6."""
import os

import numpy as np
import pytest
import torch

import select_boxes_ref as SR
from oracle import oracle_input as OI
from test_select_boxes_cpu import fixture_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OBJ_KEYS = ("cls", "box2d", "centroid", "half_extent", "heading")


def ragged_rows(arrays, dev):
    """clouds with different numbers of columns -> one (rows, widest) device tensor (the narrower ones zero-padded) + offsets."""
    from votenet_amd import input_pipeline as IP
    cols = max(a.shape[1] for a in arrays)
    return IP.pack_ragged([np.pad(a, [(0, 0), (0, cols - a.shape[1])]) for a in arrays], dev)


def fixture_objects(g):
    obj = {k: g["obj_" + k] for k in OBJ_KEYS}
    obj["obj_offset"] = g["obj_offset"]
    return obj


def compare_inside(got, exp, margin, ref_count, what):
    """got / exp (nobj, n) bool.  -> number of points left out under the rule of this file's docstring."""
    differ = got != exp
    left_out = differ & (margin < SR.EXCLUDE)
    assert not (differ & ~left_out).any(), "%s: %d points differ away from any face" % (what, (differ & ~left_out).sum())
    small = (ref_count >= 3) & (ref_count <= 6)
    assert not left_out[small].any(), "%s: a point left out of an object holding 3-6 points" % what
    return int(left_out.sum())


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_fixtures_with_host_choice(hiplib, dev, golden, f64):
    from votenet_amd import input_pipeline as IP
    g = golden("select_boxes")
    b, n_out, tag = int(g["b"]), int(g["n_out"]), "f64" if f64 else "f32"
    raw, off = ragged_rows([g[("raw64_%d" if f64 else "raw32_%d") % s] for s in range(b)], dev)
    assert raw.shape[1] == 6 and raw.dtype == (torch.float64 if f64 else torch.float32)
    choice = np.stack([g["choice_%d" % s] for s in range(b)])
    out = IP.select_boxes(raw, off, (g["Rtilt"], g["K"]), fixture_objects(g), n_out, choice, want_inside=True)
    inside, n_inside, status = out["inside"].cpu().numpy().astype(bool), out["n_inside"].cpu().numpy(), out["status"].cpu().numpy()
    center, size, heading, cls = (out[k].cpu().numpy() for k in ("center", "size", "heading", "cls"))
    assert out["center"].dtype == torch.float64 and out["cls"].dtype == torch.int32 and out["box_offset"].dtype == np.int64
    left_out = tested = 0
    for s in range(b):
        pts, sl, ref = fixture_scene(g, s, tag)
        rs = SR.select_scene(pts, g["Rtilt"][s], g["K"][s], *[g["obj_" + k][sl] for k in OBJ_KEYS])
        lo = compare_inside(inside[sl], ref["inside"], rs["margin"], ref["n_inside"], "scene %d" % s)
        left_out += lo
        tested += ref["inside"].size
        k0, k1 = out["box_offset"][s], out["box_offset"][s + 1]
        print("scene %d %s: %d objects, %d kept, %d points left out, max centre error %.3g"
              % (s, tag, sl.stop - sl.start, k1 - k0, lo, np.abs(center[k0:k1] - ref["center"]).max() if k1 > k0 else 0.0))
        if lo == 0:
            assert np.array_equal(n_inside[sl], ref["n_inside"])
        assert np.array_equal(status[sl], ref["status"])
        assert k1 - k0 == len(ref["cls"])
        assert np.array_equal(size[k0:k1], ref["size"]) and np.array_equal(heading[k0:k1], ref["heading"])
        assert np.array_equal(cls[k0:k1], ref["cls"])
        if k1 > k0:
            assert np.abs(center[k0:k1] - ref["center"]).max() <= 1e-12
    assert left_out <= 1e-4 * tested
    assert len(center) == out["box_offset"][-1]


def real_size_batch(seed, b=8, max_obj=40):
    rng = np.random.default_rng(seed)
    clouds, calib, scenes = [], [], []
    for s in range(b):
        n = int(rng.integers(50000, 200001))
        clouds.append(np.column_stack([rng.uniform(-3, 3, n), rng.uniform(0.5, 7, n), rng.uniform(-1.5, 1.5, n)]))
        a, c = rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05)
        rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        f = rng.uniform(500, 600)
        calib.append((rx @ rz, np.array([[f, 0, rng.uniform(300, 400)], [0, f, rng.uniform(220, 300)], [0, 0, 1.0]])))
        nobj = int(rng.integers(1, max_obj + 1)) if s else max_obj
        cen = np.column_stack([rng.uniform(-2.5, 2.5, nobj), rng.uniform(1.5, 6, nobj), rng.uniform(-1, 1, nobj)])
        ext = rng.uniform(0.02, 0.9, (nobj, 3))
        # a 2D box around the projected centre, sometimes narrow enough to cut the 3D box
        u, v = SR.project_to_image(cen, *calib[-1])
        wpx = rng.uniform(20, 400, (nobj, 2))
        scenes.append({"cls": rng.integers(-1, 10, nobj).astype(np.int32),
                       "box2d": np.column_stack([u - wpx[:, 0], v - wpx[:, 1], u + wpx[:, 0], v + wpx[:, 1]]),
                       "centroid": cen, "half_extent": ext, "heading": rng.uniform(-np.pi, np.pi, nobj)})
    return clouds, calib, scenes


def test_real_size_with_device_draw_matches_the_restatement(hiplib, dev):
    """8 scenes x 50 000 - 200 000 raw rows -> 20 480, up to 40 objects, choice=None: the rows tested are the rows
    subsample_augment returns for the same seed / scene0, which are the rows oracle_input.feistel_choice names."""
    from votenet_amd import input_pipeline as IP, sunrgbd
    clouds, calib, scenes = real_size_batch(11)
    b, n_out, seed, scene0 = len(clouds), IP.POINT_NUM, 77, 5
    raw, off = IP.pack_ragged(clouds, dev)
    objects = sunrgbd.pack_objects(scenes)
    out = IP.select_boxes(raw, off, calib, objects, n_out, None, seed, scene0, want_inside=True)
    rows = IP.subsample_augment(raw, off, n_out, None, None, seed, scene0, depth_to_camera=False).cpu().numpy()
    inside, n_inside, status = out["inside"].cpu().numpy().astype(bool), out["n_inside"].cpu().numpy(), out["status"].cpu().numpy()
    left_out = tested = 0
    seen = set()
    for s in range(b):
        ch = OI.feistel_choice(len(clouds[s]), n_out, seed, scene0 + s)
        pts = clouds[s][ch]
        assert np.array_equal(pts.astype(np.float32), rows[s])
        sl = slice(objects["obj_offset"][s], objects["obj_offset"][s + 1])
        rs = SR.select_scene(pts, calib[s][0], calib[s][1], *[objects[k][sl] for k in OBJ_KEYS])
        lo = compare_inside(inside[sl], rs["inside"], rs["margin"], rs["n_inside"], "scene %d" % s)
        left_out += lo
        tested += rs["inside"].size
        print("scene %d: %d rows, %d objects, status counts %s, %d left out" % (s, len(clouds[s]), sl.stop - sl.start,
                                                                               np.bincount(rs["status"], minlength=4), lo))
        if lo == 0:
            assert np.array_equal(n_inside[sl], rs["n_inside"]) and np.array_equal(status[sl], rs["status"])
        k0, k1 = out["box_offset"][s], out["box_offset"][s + 1]
        if lo == 0:
            assert k1 - k0 == len(rs["kept"])
            assert np.array_equal(out["size"][k0:k1].cpu().numpy(), rs["size"]) and np.array_equal(out["cls"][k0:k1].cpu().numpy(), rs["cls"])
            assert np.array_equal(out["heading"][k0:k1].cpu().numpy(), rs["heading"])
            if k1 > k0:
                assert np.abs(out["center"][k0:k1].cpu().numpy() - rs["center"]).max() <= 1e-12
        seen |= set(rs["status"].tolist())
    assert left_out <= 1e-4 * tested and seen == {0, 1, 3}


def test_two_runs_are_bit_identical_and_a_second_stream_works(hiplib, dev):
    from votenet_amd import input_pipeline as IP, sunrgbd
    clouds, calib, scenes = real_size_batch(12, b=3, max_obj=70)
    raw, off = IP.pack_ragged([c.astype(np.float32) for c in clouds], dev)
    objects = sunrgbd.pack_objects(scenes)
    run = lambda: IP.select_boxes(raw, off, calib, objects, 4096, None, 9, 0, want_inside=True)
    a, c = run(), run()
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        d = run()
    st.synchronize()
    runs = [c, d]
    if torch.cuda.device_count() > 1:  # a tensor on another device than the current one: the call switches for its duration
        other = torch.device("cuda:1")
        e = IP.select_boxes(raw.to(other), off, calib, objects, 4096, None, 9, 0, want_inside=True)
        assert e["center"].device == other and torch.cuda.current_device() == 0
        runs.append(e)
    for r in runs:
        assert np.array_equal(a["box_offset"], r["box_offset"])
        for k in ("center", "size", "heading", "cls", "n_inside", "status", "inside"):
            assert torch.equal(a[k].cpu(), r[k].cpu()), k
    assert a["box_offset"][-1] > 0


def test_build_batch_is_the_three_calls_and_a_dropped_scene_consumes_its_draw(hiplib, dev, golden):
    from votenet_amd import input_pipeline as IP
    g = golden("select_boxes")
    b, n_out = int(g["b"]), int(g["n_out"])
    raw, off = ragged_rows([g["raw64_%d" % s] for s in range(b)], dev)
    choice = np.stack([g["choice_%d" % s] for s in range(b)])
    calib, objects = (g["Rtilt"], g["K"]), fixture_objects(g)
    aug = IP.draw_augmentation(b, np.random.RandomState(4))
    points, gt, scene_index = IP.build_batch(raw, off, calib, objects, aug, choice, n_out=n_out)
    assert list(scene_index) == [0, 1, 2, 5] and scene_index.dtype == np.int64    # scene 3 keeps nothing, scene 4 has no labels
    sel = IP.select_boxes(raw, off, calib, objects, n_out, choice)
    all_points = IP.subsample_augment(raw, off, n_out, aug, choice)               # the full draw list
    assert torch.equal(points, all_points[[0, 1, 2, 5]])
    cnt = np.diff(sel["box_offset"])
    sub = IP.Augmentation(aug.flip_x[scene_index], aug.flip_z[scene_index], aug.angle[scene_index], aug.scale[scene_index])
    by_hand = IP.augment_boxes(sel["center"], sel["size"], sel["heading"], sel["cls"], np.concatenate([[0], np.cumsum(cnt[scene_index])]), sub)
    assert set(gt) == {k for k, _, _ in IP.GT_FIELDS}
    for k in gt:
        assert torch.equal(gt[k], by_hand[k]), k
    # evaluation (no draws) and the device draw go through as well
    p2, gt2, idx2 = IP.build_batch(raw, off, calib, objects, None, None, seed=3, scene0=2, n_out=n_out)
    keep = torch.from_numpy(idx2).to(dev)
    assert torch.equal(p2, IP.subsample_augment(raw, off, n_out, None, None, 3, 2)[keep]) and gt2["bboxes_xyz"].shape[0] == len(idx2)
    # a batch whose scenes all keep nothing
    o34 = {k: objects[k][objects["obj_offset"][3]:objects["obj_offset"][5]] for k in OBJ_KEYS}
    o34["obj_offset"] = objects["obj_offset"][3:6] - objects["obj_offset"][3]
    r34 = raw[off[3]:off[5]]
    p, q, idx = IP.build_batch(r34, off[3:6] - off[3], (g["Rtilt"][3:5], g["K"][3:5]), o34, IP.draw_augmentation(2), choice[3:5], n_out=n_out)
    assert p is None and q is None and len(idx) == 0


def test_text_to_model_inputs_matches_the_oracle(hiplib, dev, golden):
    """The fixture label / calibration text -> parse -> build_batch -> the eight ground-truth inputs, against
    oracle_input.augment_boxes / batch_boxes applied to the reference's kept boxes of that scene; points against
    oracle_input.augment_points."""
    from votenet_amd import input_pipeline as IP, sunrgbd, synth
    g = golden("select_boxes")
    n_out = int(g["n_out"])
    lab = sunrgbd.parse_label(open(os.path.join(GOLD, "select_boxes_label.txt")).read())
    cal = sunrgbd.parse_calib(open(os.path.join(GOLD, "select_boxes_calib.txt")).read())
    rawn = g["raw64_0"]
    raw = torch.from_numpy(rawn).to(dev)
    aug = IP.draw_augmentation(1, np.random.RandomState(8))
    points, gt, idx = IP.build_batch(raw, np.array([0, len(rawn)]), [cal], sunrgbd.pack_objects([lab]), aug, g["choice_0"][None], n_out=n_out)
    assert list(idx) == [0]
    exp_pts = OI.augment_points(rawn, g["choice_0"], aug.flip_x[0], aug.flip_z[0], aug.angle[0], aug.scale[0])
    assert np.array_equal(points[0].cpu().numpy(), exp_pts)
    ms = np.asarray(synth.MEAN_SIZES, np.float64)
    per = OI.augment_boxes(g["center_f64_0"], g["size_f64_0"], g["heading_f64_0"], g["cls_f64_0"], aug.flip_x[0], aug.flip_z[0],
                           aug.angle[0], aug.scale[0], ms, synth.NH)
    exp = OI.batch_boxes([per])
    assert gt["bboxes_xyz"].shape == (1, 5, 3)
    for k, v in exp.items():
        got = gt[k].cpu().numpy()
        if k != "bboxes_xyz":  # size / heading / class enter exactly: bit-exact like test_gpu_input.py
            assert np.array_equal(got, v), k
        else:  # the centres enter within 1e-12 of the reference's: the float32 results differ by one unit in the last place at most
            assert (np.abs(got - v) <= np.spacing(np.abs(v))).all(), k


def test_invalid_arguments_raise_and_leave_no_sticky_error(hiplib, dev, golden):
    from votenet_amd import _lib, input_pipeline as IP, sunrgbd
    g = golden("select_boxes")
    lab = sunrgbd.parse_label(open(os.path.join(GOLD, "select_boxes_label.txt")).read())
    objects = sunrgbd.pack_objects([lab, lab])
    cal = (np.eye(3), g["K"][0])
    raw = torch.zeros(100, 3, device=dev)
    off = np.array([0, 60, 100])
    with pytest.raises(_lib.InvalidArgumentError):   # 40 rows, 50 wanted
        IP.select_boxes(raw, off, [cal, cal], objects, 50)
    bad = dict(objects, obj_offset=np.array([0, 15, 11]))
    with pytest.raises(_lib.InvalidArgumentError):   # obj_offset not monotone
        IP.select_boxes(raw, off, [cal, cal], bad, 10)
    with pytest.raises(_lib.InvalidArgumentError):   # as many calibrations as scenes
        IP.select_boxes(raw, off, [cal], objects, 10)
    with pytest.raises(_lib.InvalidArgumentError):
        IP.select_boxes(raw, off, [cal, cal], objects, 10, choice=np.full((2, 10), 70))
    with pytest.raises(_lib.InvalidArgumentError):   # the C entry validates on its own: a workspace that is too small
        rt = np.ascontiguousarray(np.tile(np.eye(3).reshape(1, 9), (2, 1)))
        o = np.array([0, 1, 2], np.int64)
        z = torch.zeros(64, dtype=torch.float64, device=dev)
        zi = torch.zeros(64, dtype=torch.int32, device=dev)
        _lib.check(hiplib.votenet_select_boxes(2, 10, raw.data_ptr(), 0, 3, off.astype(np.int64).ctypes.data, None, 0, 0, rt.ctypes.data,
                                               rt.ctypes.data, o.ctypes.data, zi.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                               z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), zi.data_ptr(), zi.data_ptr(),
                                               zi.data_ptr(), zi.data_ptr(), None, zi.data_ptr(), 4, None))
    torch.cuda.synchronize()
    out = IP.select_boxes(raw, off, [cal, cal], objects, 40)   # the device is still usable, and an empty cloud keeps nothing
    assert out["box_offset"].tolist() == [0, 0, 0] and out["center"].shape == (0, 3)
    assert set(out["status"].cpu().numpy().tolist()) <= {1, 2, 3}
    torch.cuda.synchronize()


def test_device_draw_at_the_width_boundaries(hiplib, dev):
    """select_boxes tests the rows feistel_perm draws: scene sizes on both sides of every width of its loop, in one ragged batch across
    the 8-scene chunks.  Every scene has one object whose box holds exactly the even raw rows (z = 0; the odd ones lie at z = 100), so
    the `inside` mask of output row j is the parity of the drawn row: against oracle_input.feistel_choice row for row."""
    from test_gpu_input import DRAW_BATCHES, DRAW_SCENE0, DRAW_SEEDS
    from votenet_amd import input_pipeline as IP, sunrgbd
    sizes, n_out = DRAW_BATCHES["n256"]
    clouds = [np.stack([np.arange(n), np.ones(n), 100.0 * (np.arange(n) % 2)], 1).astype(np.float32) for n in sizes]
    raw, off = IP.pack_ragged(clouds, dev)
    calib = [(np.eye(3), np.eye(3))] * len(sizes)   # pixel (x / y, -z / y) with y = 1: every point in front of the camera
    one = {"cls": np.array([3], np.int32), "box2d": np.array([[-1e9, -1e9, 1e9, 1e9]]), "centroid": np.array([[0.0, 1.0, 0.0]]),
           "half_extent": np.array([[1e9, 1e9, 1.0]]), "heading": np.array([0.0])}
    objects = sunrgbd.pack_objects([one] * len(sizes))
    for seed in DRAW_SEEDS:
        out = IP.select_boxes(raw, off, calib, objects, n_out, None, seed, DRAW_SCENE0, want_inside=True)
        inside, n_inside = out["inside"].cpu().numpy().astype(bool), out["n_inside"].cpu().numpy()
        for s, n in enumerate(sizes):
            want = OI.feistel_choice(n, n_out, seed, DRAW_SCENE0 + s) % 2 == 0
            assert np.array_equal(inside[s], want), (seed, s, n)
            assert n_inside[s] == want.sum() >= 5
        assert (out["status"].cpu().numpy() == 0).all() and out["box_offset"].tolist() == list(range(len(sizes) + 1))
