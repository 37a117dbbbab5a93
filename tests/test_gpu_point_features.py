"""GPU: votenet_subsample_augment_features (csrc/features/point_features.hip) -- the points of votenet_subsample_augment bit for bit, the
carried raw columns, and the height above the floor: the two order statistics exact, the floor within one float32 ulp of the numpy
restatement (tests/point_features_ref.py, itself held to np.percentile by tests/test_point_features_cpu.py), height = up - floor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_features_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (301, 1007, 5003)  # ragged raw scenes
STRIDE = 6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scenes(dtype, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        a = np.concatenate([rng.normal(size=(n, 3)) * 2.0, rng.random((n, 3))], 1)
        out.append(a.astype(dtype))
    return out


def pack(arrays, dev):
    off = np.zeros(len(arrays) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrays, 0))).to(dev), off


def check_heights(points, feats, floor, stats, column=0):
    """The height column of every scene against the restatement on the DEVICE's points."""
    p, f, fl, st = points.cpu().numpy(), feats.cpu().numpy(), floor.cpu().numpy(), stats.cpu().numpy()
    for s in range(p.shape[0]):
        up = -p[s, :, 1]
        fin = np.sort(up[np.isfinite(up)])
        want_floor, a, b, m = R.floor_ref(up)
        if m:
            lo = int(np.floor(0.0099 * (m - 1)))
            assert st[s, 0] == fin[lo] and st[s, 1] == fin[min(lo + 1, m - 1)], (s, st[s], fin[lo:lo + 2])  # exact order statistics
            assert st[s, 0] == a and st[s, 1] == b
        else:
            assert st[s, 0] == 0 and st[s, 1] == 0 and fl[s] == 0
        assert abs(float(fl[s]) - float(want_floor)) <= R.ulp32(want_floor), (s, fl[s], want_floor)
        assert np.array_equal(bits(f[s, :, column]), bits(R.heights_ref(p[s], fl[s]))), s  # up - floor_from_device, bit for bit


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n_out", [1, 2, 102, 256])
def test_points_colours_and_heights(hiplib, dev, n_out, f64):
    from votenet_amd import input_pipeline as IP
    arrays = scenes(np.float64 if f64 else np.float32)
    raw, off = pack(arrays, dev)
    b = len(arrays)
    rng = np.random.RandomState(n_out)
    choice = IP.draw_choice(rng, np.diff(off), n_out)
    for aug in (None, IP.draw_augmentation(b, np.random.RandomState(3 + n_out))):
        for ch in (choice, None):
            stats = torch.full((b, 2), 7.0, device=dev)
            points, feats, floor = IP.subsample_augment_features(raw, off, n_out, aug, ch, seed=77, scene0=5, height=True, extra_cols=3,
                                                                 order_stats=stats)
            assert points.shape == (b, n_out, 3) and feats.shape == (b, n_out, 4) and floor.shape == (b,)
            assert torch.equal(points, IP.subsample_augment(raw, off, n_out, aug, ch, seed=77, scene0=5))  # bit for bit
            f = feats.cpu().numpy()
            if ch is not None:
                rows = [choice[s] for s in range(b)]
                got = points.cpu().numpy()
                for s in range(b):  # the float64 transform restated, one rounding: bit for bit
                    kw = {}
                    if aug is not None:
                        flip, _, cs, sn, sc = aug.host_arrays()
                        kw = dict(train=True, flip=int(flip[s]), cos_sin=(cs[s], sn[s]), scale=sc[s])
                    assert np.array_equal(bits(got[s]), bits(R.points_ref(arrays[s][rows[s]], True, **kw))), (s, aug is not None)
            else:  # the device's draw: the rows are the un-augmented, un-turned points, matched against the raw cloud
                plain = IP.subsample_augment(raw, off, n_out, None, None, seed=77, scene0=5, depth_to_camera=False).cpu().numpy()
                rows = []
                for s in range(b):
                    table = {bits(r[:3]).tobytes(): i for i, r in enumerate(arrays[s])}
                    assert len(table) == len(arrays[s])
                    rows.append(np.array([table[bits(q).tobytes()] for q in plain[s]]))
                    assert len(set(rows[-1])) == n_out  # without replacement
            for s in range(b):
                assert np.array_equal(bits(f[s, :, 1:]), bits(arrays[s][rows[s], 3:6])), (s, aug is not None, ch is not None)
            check_heights(points, feats, floor, stats)
            if aug is not None:  # the heights follow the augmented cloud: the scale draw scales them
                assert not torch.equal(points, IP.subsample_augment(raw, off, n_out, None, ch, seed=77, scene0=5))


def identity_case(ys, dev, extra=None):
    """Scenes whose up values are given (up = -y; camera frame already, every row taken in order) -> points, feats, floor, stats."""
    from votenet_amd import input_pipeline as IP
    n = len(ys[0])
    assert all(len(y) == n for y in ys)
    arrays = []
    for i, y in enumerate(ys):
        a = np.zeros((n, STRIDE), np.float32)
        a[:, 0], a[:, 2] = np.arange(n), i
        a[:, 1] = y
        a[:, 3:] = np.arange(n)[:, None] + np.array([0.25, 0.5, 0.75]) if extra is None else extra
        arrays.append(a)
    raw, off = pack(arrays, dev)
    choice = torch.arange(n, dtype=torch.int32, device=dev).repeat(len(ys), 1)
    stats = torch.full((len(ys), 2), 7.0, device=dev)
    points, feats, floor = IP.subsample_augment_features(raw, off, n, None, choice, depth_to_camera=False, height=True, extra_cols=3,
                                                         order_stats=stats)
    assert np.array_equal(points.cpu().numpy()[..., 1], np.stack(ys), equal_nan=True)
    return points, feats, floor, stats


def test_flat_floor_and_signed_zeros(hiplib, dev):
    rng = np.random.default_rng(2)
    n = 3000
    flat = (rng.random(n) * 2.4 - 1.2).astype(np.float32)
    flat[rng.permutation(n)[:900]] = np.float32(1.2034)          # 30 % of the scene on one plane, the lowest (up = -y): both ranks inside it
    mid = (rng.random(n) * 2.5).astype(np.float32)
    mid[rng.permutation(n)[:900]] = np.float32(2.625)            # ... the same plane with exactly 30 points below it: ranks 29 and 30
    mid[:30] = 3.0 + np.arange(30, dtype=np.float32)             # straddle its edge
    zeros = np.zeros(n, np.float32)                               # up = -0.0 everywhere
    mixed = rng.normal(size=n).astype(np.float32)
    mixed[:600] = 0.0
    mixed[600:1200] = -0.0
    neg = (rng.random(n) + 5.0).astype(np.float32)               # every up negative
    pos = -(rng.random(n) + 5.0).astype(np.float32)              # every up positive
    tiny = (rng.normal(size=n) * 1e-41).astype(np.float32)       # denormals of both signs
    few = rng.normal(size=n).astype(np.float32)
    few[:n - 30] = -50.0                                          # ranks 29 / 30 of 3000: the last of 30 low points and the plane above
    few[n - 30:] = 10.0 + np.arange(30, dtype=np.float32)
    points, feats, floor, stats = identity_case([flat, mid, zeros, mixed, neg, pos, tiny, few], dev)
    check_heights(points, feats, floor, stats)
    st = stats.cpu().numpy()
    assert st[0, 0] == st[0, 1] == np.float32(-1.2034) and float(floor[0]) == np.float32(-1.2034)
    assert st[1, 0] == np.float32(-3.0) and st[1, 1] == np.float32(-2.625)
    assert st[2, 0] == 0 and st[2, 1] == 0 and float(floor[2]) == 0 and float(feats[2, :, 0].abs().max()) == 0
    assert st[7, 0] == np.float32(-10.0) and st[7, 1] == np.float32(50.0)  # adjacent ranks in different top digits
    f = feats.cpu().numpy()
    assert np.array_equal(f[0, :, 1:], np.arange(n, dtype=np.float32)[:, None] + np.array([0.25, 0.5, 0.75], np.float32))


def test_rows_that_are_not_finite_stay_out(hiplib, dev):
    rng = np.random.default_rng(3)
    n = 400
    y = rng.normal(size=n).astype(np.float32)
    holes = [3, 64, 65, 200, 399]
    y[holes] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    allbad = np.full(n, np.nan, np.float32)
    one = np.full(n, np.inf, np.float32)
    one[17] = -2.5                                                # m = 1
    two = np.full(n, -np.inf, np.float32)
    two[[5, 300]] = [1.0, -3.0]                                   # m = 2
    points, feats, floor, stats = identity_case([y, allbad, one, two], dev)
    check_heights(points, feats, floor, stats)
    f = feats.cpu().numpy()[..., 0]
    assert (f[0, holes] == 0).all() and np.isfinite(f).all()
    assert float(floor[1]) == 0 and (f[1] == 0).all()
    assert float(floor[2]) == 2.5 and f[2, 17] == 0 and (np.delete(f[2], 17) == 0).all()
    st = stats.cpu().numpy()
    assert st[3, 0] == -1.0 and st[3, 1] == 3.0
    assert abs(float(floor[3]) - np.percentile(np.array([-1.0, 3.0]), 0.99)) <= R.ulp32(floor[3].item())


def test_small_m_cases_of_the_rank_formula(hiplib, dev):
    """n_out = 1, 2 and 102 with every point finite: k = 0, 0.0099, 0.9999 (t just under 1)."""
    from votenet_amd import input_pipeline as IP
    rng = np.random.default_rng(4)
    for n in (1, 2, 102):
        ys = [rng.normal(size=n).astype(np.float32) * 3 for _ in range(3)]
        points, feats, floor, stats = identity_case(ys, dev)
        check_heights(points, feats, floor, stats)
        for s in range(3):
            assert abs(float(floor[s]) - np.percentile(-ys[s].astype(np.float64), 0.99)) <= R.ulp32(floor[s].item())


@pytest.mark.parametrize("height,extra", [(False, 3), (True, 0), (True, 1), (False, 1), (True, 4)])
def test_feature_layouts(hiplib, dev, height, extra):
    from votenet_amd import input_pipeline as IP
    arrays = [np.concatenate([a, a[:, 3:5] + 1.0], 1) for a in scenes(np.float64, 9)]  # stride 8
    raw, off = pack(arrays, dev)
    n_out = 102
    aug = IP.draw_augmentation(3, np.random.RandomState(1))
    choice = IP.draw_choice(np.random.RandomState(2), np.diff(off), n_out)
    stats = torch.full((3, 2), 7.0, device=dev)
    points, feats, floor = IP.subsample_augment_features(raw, off, n_out, aug, choice, height=height, extra_cols=extra, order_stats=stats)
    assert torch.equal(points, IP.subsample_augment(raw, off, n_out, aug, choice))
    h = 1 if height else 0
    assert feats.shape == (3, n_out, h + extra)
    f = feats.cpu().numpy()
    for s in range(3):
        assert np.array_equal(bits(f[s, :, h:]), bits(arrays[s][choice[s], 3:3 + extra]))
    if height:
        check_heights(points, feats, floor, stats)
    else:
        assert floor is None and float(stats.min()) == 7.0  # neither is written


def test_invalid_arguments(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import input_pipeline as IP
    raw, off = pack(scenes(np.float32), dev)
    for kw in (dict(height=False, extra_cols=0), dict(extra_cols=5), dict(height=False, extra_cols=5), dict(extra_cols=-1),
               dict(extra_cols=4)):  # (stride 6: 3 + 4 columns are not there)
        with pytest.raises(L.InvalidArgumentError):
            IP.subsample_augment_features(raw, off, 64, **kw)
    with pytest.raises(L.InvalidArgumentError):
        IP.subsample_augment_features(raw, off, 400)  # scene 0 has 301 rows
    with pytest.raises(L.InvalidArgumentError):
        IP.subsample_augment_features(raw, off, 10, choice=np.full((3, 10), 400))
    with pytest.raises(L.InvalidArgumentError):
        IP.subsample_augment_features(raw, off, 10, aug=IP.draw_augmentation(2))
    with pytest.raises(L.InvalidArgumentError):
        IP.subsample_augment_features(raw[:, :2].contiguous(), off, 10)
    with pytest.raises(L.InvalidArgumentError):
        IP.subsample_augment_features(raw, off, 10, order_stats=torch.zeros(3, 3, device=dev))
    # the C entry's own checks (the wrapper's come first): straight through the binding
    F = L.side_lib("features")
    out, feats, floor = torch.empty(3, 10, 3, device=dev), torch.empty(3, 10, 4, device=dev), torch.empty(3, device=dev)

    def call(want_height=1, extra=3, stride=6, o=out, f=feats, fl=floor):
        return F.votenet_subsample_augment_features(3, 10, L.ptr(raw), 0, stride, off.ctypes.data, None, 0, 0, 1, None, None, None, None,
                                                    want_height, extra, L.ptr(o), L.ptr(f), L.ptr(fl), None, L.stream_ptr())
    for kw in (dict(want_height=0, extra=0), dict(extra=5), dict(want_height=2), dict(stride=5), dict(f=None), dict(fl=None), dict(o=None)):
        assert call(**kw) == 1, kw
        with pytest.raises(L.InvalidArgumentError, match="subsample_augment_features"):
            L.check(1, side="features")
    assert call() == 0 and call(want_height=0, fl=None) == 0
    torch.cuda.synchronize()


def test_build_batch_carries_the_features(hiplib, dev, golden):
    from test_gpu_select_boxes import fixture_objects, ragged_rows
    from votenet_amd import input_pipeline as IP
    g = golden("select_boxes")
    b, n_out = int(g["b"]), int(g["n_out"])
    raw, off = ragged_rows([g["raw64_%d" % s] for s in range(b)], dev)
    choice = np.stack([g["choice_%d" % s] for s in range(b)])
    calib, objects = (g["Rtilt"], g["K"]), fixture_objects(g)
    aug = IP.draw_augmentation(b, np.random.RandomState(4))
    extra = min(3, raw.shape[1] - 3)
    plain_points, plain_gt, plain_index = IP.build_batch(raw, off, calib, objects, aug, choice, n_out=n_out)
    assert "features" not in plain_gt
    points, gt, scene_index = IP.build_batch(raw, off, calib, objects, aug, choice, n_out=n_out, height=True, extra_cols=extra)
    assert torch.equal(points, plain_points) and np.array_equal(scene_index, plain_index) and len(scene_index) < b
    assert set(gt) == set(plain_gt) | {"features"} and all(torch.equal(gt[k], plain_gt[k]) for k in plain_gt)
    _, feats, _ = IP.subsample_augment_features(raw, off, n_out, aug, choice, height=True, extra_cols=extra)
    assert torch.equal(gt["features"], feats[torch.from_numpy(scene_index).to(dev)]) and gt["features"].shape == (len(scene_index), n_out, 1 + extra)


def test_device_draw_at_the_width_boundaries(hiplib, dev):
    """The features entry draws through the same feistel_perm: scene sizes on both sides of every width of its loop, in one ragged batch
    across the 16-scene chunk, against oracle_input.feistel_choice row for row (test_gpu_input.check_draw), and the points of
    subsample_augment bit for bit."""
    from test_gpu_input import DRAW_BATCHES, DRAW_SCENE0, DRAW_SEEDS, check_draw, draw_scenes
    from votenet_amd import input_pipeline as IP
    sizes, n_out = DRAW_BATCHES["n256"]
    raw, off = pack(draw_scenes(sizes), dev)
    for seed in DRAW_SEEDS:
        points, feats, floor = IP.subsample_augment_features(raw, off, n_out, None, None, seed=seed, scene0=DRAW_SCENE0,
                                                             depth_to_camera=False, height=True, extra_cols=0)
        assert torch.equal(points, IP.subsample_augment(raw, off, n_out, None, None, seed=seed, scene0=DRAW_SCENE0, depth_to_camera=False))
        got = points.cpu().numpy()
        assert np.array_equal(got[:, :, 1], np.repeat(np.arange(len(sizes), dtype=np.float32)[:, None], n_out, 1))
        check_draw(got[:, :, 0].astype(np.int64), sizes, n_out, seed, DRAW_SCENE0, ("features", seed))
