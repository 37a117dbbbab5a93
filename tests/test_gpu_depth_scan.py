"""GPU: the raw scan from the depth image (libvotenet_depth.so: votenet_depth_scan; votenet_amd/depth_scan.py).  Every output is
compared BIT FOR BIT with the numpy restatement of include/votenet_depth_scan.h (tests/depth_scan_ref.py, itself held to the
reference's geometry in tests/test_depth_scan_cpu.py), offsets included."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_scan_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

T = 2048  # depth_scan.TILE_PIXELS: one workgroup's pixels
SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), T - 1: (23, 89), T: (32, 64), T + 1: (3, 683), 3 * T + 5: (43, 143)}
PATTERNS = ("all", "none", "alternating", "last", "random")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def image(rng, h, w, pattern="random", encoding="sunrgbd"):
    d = R.random_depth(rng, h, w, encoding, zeros=0.3 if pattern == "random" else 0.0)
    flat = d.reshape(-1)
    if pattern == "none":
        flat[:] = 0
    elif pattern == "alternating":
        flat[rng.integers(0, 2)::2] = 0
    elif pattern == "last":
        flat[:-1] = 0
    assert pattern != "all" or flat.all()
    return d


def batch(rng, shapes, patterns=None, encoding="sunrgbd", colour=True):
    depth = [image(rng, h, w, (patterns or {}).get(i, "random"), encoding) for i, (h, w) in enumerate(shapes)]
    rgb = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes] if colour else None
    calib = [R.tilted_calib(rng, h, w) for h, w in shapes]
    return depth, rgb, calib


def check(depth, rgb, calib, what, **kw):
    """scan_from_depth == the restatement: rows, their count and the offsets."""
    from votenet_amd import depth_scan
    raw, off = depth_scan.scan_from_depth(depth, calib, rgb, **kw)
    exp, eoff = R.scan(depth, calib, rgb, **kw)
    assert off.dtype == np.int64 and np.array_equal(off, eoff), (what, off, eoff)
    assert raw.dtype == torch.float32 and raw.is_cuda and tuple(raw.shape) == exp.shape, (what, tuple(raw.shape), exp.shape)
    got = raw.cpu().numpy()
    bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d rows differ, first row %d: %s != %s" % (what, len(bad), len(exp), bad[0], got[bad[0]], exp[bad[0]])
    return got, off


# ------------------------------------------------------------------ one scene
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_one_scene_equals_the_restatement_bit_for_bit(hiplib, dev, n):
    """1, 63 / 64 / 65: either side of a wave of single pixels; one tile - 1 / one tile / one tile + 1; three tiles + 5."""
    from votenet_amd import depth_scan
    assert depth_scan.TILE_PIXELS == T
    h, w = SHAPES[n]
    assert h * w == n
    rng = np.random.default_rng(n)
    for pattern in PATTERNS:
        for colour in (False, True):
            depth, rgb, calib = batch(rng, [(h, w)], {0: pattern}, colour=colour)
            got, off = check(depth, rgb, calib, (n, pattern, colour))
            valid = {"all": n, "none": 0, "last": 1}.get(pattern)
            assert valid is None or off[-1] == valid
            assert got.shape[1] == (6 if colour else 3)
    print("%d pixels (%d x %d): %s, with and without colour" % (n, h, w, ", ".join(PATTERNS)))


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("b", [1, 2, 17])
def test_batches_of_scenes_of_different_sizes(hiplib, dev, b):
    """An odd pixel count first, so that the next scene starts off every boundary; a scene without a valid pixel in the middle; scenes
    of one pixel and of several tiles side by side (most workgroups of the small ones have no tile)."""
    cycle = [(7, 9), (43, 143), (1, 1), (32, 64), (3, 683), (5, 13), (23, 89), (48, 64)]
    shapes = [cycle[i % len(cycle)] for i in range(b)]
    rng = np.random.default_rng(100 + b)
    patterns = {b // 2: "none"} if b > 2 else {}
    if b == 17:
        patterns.update({3: "all", 5: "last", 10: "none", 11: "alternating"})
    for colour in (True, False):
        depth, rgb, calib = batch(rng, shapes, patterns, colour=colour)
        got, off = check(depth, rgb, calib, (b, colour))
        assert all(off[s + 1] == off[s] for s, p in patterns.items() if p == "none")
        assert off[-1] > 0 and (b == 1 or int(np.cumsum([h * w for h, w in shapes])[0]) % 2 == 1)
    # the calibration as the two (b, 3, 3) arrays, and the images as device tensors: the same rows
    from votenet_amd import depth_scan
    rt, km = np.stack([c[0] for c in calib]), np.stack([c[1] for c in calib])
    raw, off2 = depth_scan.scan_from_depth([torch.from_numpy(d).to(dev) for d in depth], (rt, km))
    assert np.array_equal(off2, off) and same_bits(raw.cpu().numpy(), got)


# ------------------------------------------------------------------ options
def test_encodings_pixel_origins_clamps_and_colour(hiplib, dev):
    shapes = [(5, 13), (43, 143), (48, 64)]
    rng = np.random.default_rng(7)
    seen = set()
    for encoding in ("sunrgbd", "mm"):
        for colour in (False, True):
            depth, rgb, calib = batch(rng, shapes, encoding=encoding, colour=colour)
            mm = np.concatenate([R.decode(d, encoding).reshape(-1) for d in depth])
            for origin in (0.0, 1.0):
                for max_depth in (8.0, 2.5, 100.0):
                    got, _ = check(depth, rgb, calib, (encoding, colour, origin, max_depth), encoding=encoding, pixel_origin=origin,
                                   max_depth=max_depth)
                    assert ((mm > 1000 * max_depth).sum() > 100) == (max_depth < 100.0)  # the clamp took part, or not at all
                    seen.add(got[:, :3].tobytes())
    assert len(seen) == 2 * 2 * 2 * 3  # no two settings gave the same coordinates
    # the same stored values read under the other encoding are other points
    depth, rgb, calib = batch(rng, shapes[:1], encoding="mm", colour=False)
    a, _ = check(depth, rgb, calib, "mm", encoding="mm")
    b, _ = check(depth, rgb, calib, "sunrgbd", encoding="sunrgbd")
    assert a.shape == b.shape and not same_bits(a, b)


def test_invalid_arguments_raise(hiplib, dev):
    from votenet_amd import InvalidArgumentError, depth_scan
    rng = np.random.default_rng(0)
    depth, rgb, calib = batch(rng, [(5, 13), (8, 8)])
    for args, kw in [((depth, calib[:1]), {}), ((depth, calib, rgb[:1]), {}), ((depth, calib, [rgb[1], rgb[0]]), {}),
                     (([d.astype(np.int32) for d in depth], calib), {}), ((depth, calib, [c.astype(np.float32) for c in rgb]), {}),
                     (([depth[0].reshape(-1), depth[1]], calib), {}), ((depth, calib), dict(encoding="metres")), (([], []), {}),
                     ((depth * 17, calib * 17), {})]:
        with pytest.raises(InvalidArgumentError):
            depth_scan.scan_from_depth(*args, **kw)
    bad_k = [(c[0], c[1].copy()) for c in calib]
    bad_k[1][1][1, 1] = 0.0
    with pytest.raises(InvalidArgumentError, match=r"scene 1 has K\[0,0\]"):
        depth_scan.scan_from_depth(depth, bad_k)


# ------------------------------------------------------------------ capacity
def test_rows_beyond_the_capacity_are_never_written(hiplib, dev):
    """The raw entry on a buffer prefilled with a pattern, the capacity inside a tile, at a tile's first row, at 0 and at exactly the
    valid total; depth and raw at addresses off every 16-byte boundary."""
    from votenet_amd import InvalidArgumentError, depth_scan
    from votenet_amd import _lib as L
    from votenet_amd import input_pipeline as IP
    lib = L.side_lib("depth")
    shapes = [(7, 9), (43, 143), (23, 89)]
    rng = np.random.default_rng(3)
    depth, rgb, calib = batch(rng, shapes)
    hw = np.ascontiguousarray(shapes, dtype=np.int32)
    off = np.zeros(len(shapes) + 1, np.int64)
    off[1:] = np.cumsum(hw[:, 0] * hw[:, 1])
    rt, km = IP._calib_arrays(calib, len(shapes), "test")
    SENT = 0x5A5A5A5A
    for colour in (True, False):
        exp, eoff = R.scan(depth, calib, rgb if colour else None)
        total, stride = len(exp), exp.shape[1]
        first_tile = int((R.decode(depth[0], 0) != 0).sum() + (R.decode(depth[1], 0).reshape(-1)[:T - 63 % 8] != 0).sum())
        for skew in (0, 1):  # elements / floats by which depth and raw start off an allocation's (aligned) first byte
            d = torch.from_numpy(np.concatenate([np.zeros(skew, np.uint16)] + [x.reshape(-1) for x in depth]).view(np.int16)).to(dev)[skew:]
            c = torch.from_numpy(np.concatenate([np.zeros(skew, np.uint8)] + [x.reshape(-1) for x in rgb])).to(dev)[skew:] if colour else None
            for cap in (0, 1, total // 2, first_tile, total - 1, total):
                buf = torch.full((skew + (total + 64) * stride,), SENT, dtype=torch.int32, device=dev)
                raw = buf[skew:].view(torch.float32)
                off_dev = torch.full((len(shapes) + 2,), SENT, dtype=torch.int64, device=dev)
                need = lib.votenet_depth_scan_workspace_bytes(len(shapes), int(off[-1]))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                L.check(lib.votenet_depth_scan(len(shapes), d.data_ptr(), L.ptr(c), IP._hp(off), IP._hp(hw), IP._hp(rt), IP._hp(km), 0, 1.0, 8.0,
                                               raw.data_ptr(), stride, cap, off_dev.data_ptr(), ws.data_ptr(), need, L.stream_ptr()), side="depth")
                assert off_dev.cpu().tolist() == eoff.tolist() + [SENT], (colour, skew, cap)
                got = buf.cpu().numpy()
                assert (got[:skew] == SENT).all() and (got[skew + cap * stride:] == SENT).all(), (colour, skew, cap)
                assert np.array_equal(got[skew:skew + cap * stride], exp[:cap].reshape(-1).view(np.int32)), (colour, skew, cap)
        for cap in (0, total - 1):
            with pytest.raises(InvalidArgumentError, match="%d valid pixels, capacity_rows = %d" % (total, cap)):
                depth_scan.scan_from_depth(depth, calib, rgb if colour else None, capacity_rows=cap)
        raw, off2 = depth_scan.scan_from_depth(depth, calib, rgb if colour else None, capacity_rows=total)
        assert same_bits(raw.cpu().numpy(), exp) and np.array_equal(off2, eoff)


# ------------------------------------------------------------------ determinism
def test_two_runs_write_the_same_bytes(hiplib, dev):
    from votenet_amd import depth_scan
    rng = np.random.default_rng(9)
    depth, rgb, calib = batch(rng, [(120, 160)] * 4 + [(97, 131)] * 3)
    a, oa = depth_scan.scan_from_depth(depth, calib, rgb)
    b, ob = depth_scan.scan_from_depth(depth, calib, rgb)
    assert a.shape[0] > 50000 and np.array_equal(oa, ob) and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ the whole input pipeline
def labelled_scenes(rng):
    """Two 48 x 64 scenes -- a surface 2 to 3 m away, a fifth of the pixels without a reading -- each with two labelled objects around
    points of its own scan (so that enough subsampled points fall inside) and one outside the class list."""
    from votenet_amd import sunrgbd
    shapes = [(48, 64), (48, 64)]
    depth = [R.encode(np.where(rng.random(s) < 0.2, 0, rng.integers(2000, 3000, s)).astype(np.uint16), "sunrgbd") for s in shapes]
    rgb = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    calib = [R.tilted_calib(rng, h, w) for h, w in shapes]
    scenes = []
    for d, c in zip(depth, calib):
        pts = R.scan_one(d, c[0], c[1]).astype(np.float64)
        lab = {k: [] for k, _, _ in sunrgbd.OBJECT_FIELDS}
        for cls, anchor in ((3, pts[len(pts) // 3]), (0, pts[2 * len(pts) // 3]), (-1, pts[0])):
            lab["cls"].append(cls)
            lab["box2d"].append([1.0, 1.0, 65.0, 49.0])
            lab["centroid"].append(anchor)
            lab["half_extent"].append([0.9, 0.8, 0.7])
            lab["heading"].append(rng.uniform(-1, 1))
        scenes.append(lab)
    return depth, rgb, calib, sunrgbd.pack_objects(scenes)


@pytest.mark.parametrize("features", [False, True])
def test_build_batch_from_depth_is_build_batch_on_the_restated_scan(hiplib, dev, features):
    from votenet_amd import depth_scan
    from votenet_amd import input_pipeline as IP
    rng = np.random.default_rng(21)
    depth, rgb, calib, objects = labelled_scenes(rng)
    aug = IP.draw_augmentation(2, np.random.RandomState(4))
    kw = dict(aug=aug, seed=11, scene0=5, n_out=256)
    if features:
        kw.update(height=True, extra_cols=3)
    exp_raw, exp_off = R.scan(depth, calib, rgb)
    assert (np.diff(exp_off) >= 256).all()
    e_points, e_gt, e_index = IP.build_batch(torch.from_numpy(exp_raw).to(dev), exp_off, calib, objects, **kw)
    points, gt, index = depth_scan.build_batch_from_depth(depth, calib, objects, rgb, **kw)
    assert np.array_equal(index, e_index) and index.tolist() == [0, 1]
    assert tuple(points.shape) == (2, 256, 3) and torch.equal(points.view(torch.int32), e_points.view(torch.int32))
    assert set(gt) == set(e_gt) == {k for k, _, _ in IP.GT_FIELDS} | ({"features"} if features else set())
    for key in gt:
        assert gt[key].dtype == e_gt[key].dtype and gt[key].shape == e_gt[key].shape, key
        a, b = gt[key].cpu().numpy(), e_gt[key].cpu().numpy()
        assert a.tobytes() == b.tobytes(), key
    assert gt["bboxes_xyz"].shape[1] == 2 and sorted(gt["semantic_labels"][0].tolist()) == [0, 3]  # both listed objects train, the third does not
    if features:
        assert tuple(gt["features"].shape) == (2, 256, 4)
        colours = np.unique(gt["features"][..., 1:].cpu().numpy())
        assert len(colours) > 200 and set(colours) <= set((np.arange(256) / 255.0).astype(np.float32))
    # too few valid pixels for n_out: select_boxes' error
    with pytest.raises(IP.L.InvalidArgumentError, match="fewer than n_out"):
        depth_scan.build_batch_from_depth(depth, calib, objects, rgb, n_out=48 * 64)


# ------------------------------------------------------------------ lazy loading
FRESH = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import depth_scan_ref as R
import test_gpu_depth_scan as G
from votenet_amd import _lib, depth_scan
from votenet_amd import input_pipeline as IP
dev = torch.device("cuda:0")
depth, rgb, calib, objects = G.labelled_scenes(np.random.default_rng(21))
raw, off = R.scan(depth, calib, rgb)
points, gt, index = IP.build_batch(torch.from_numpy(raw).to(dev), off, calib, objects, seed=1, n_out=256)
torch.cuda.synchronize()
maps = open("/proc/self/maps").read()
assert "libvotenet_hip.so" in maps and len(index) == 2
assert not _lib.side_loaded("depth") and "libvotenet_depth" not in maps
raw2, off2 = depth_scan.scan_from_depth(depth, calib, rgb)
assert np.array_equal(off2, off) and np.array_equal(raw2.cpu().numpy().view(np.uint32), raw.view(np.uint32))
assert _lib.side_loaded("depth") and "libvotenet_depth.so" in open("/proc/self/maps").read()
print("fresh ok")
"""


def test_a_fresh_process_build_batch_does_not_load_the_new_library(hiplib):
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", FRESH % (os.path.dirname(here), here)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr
