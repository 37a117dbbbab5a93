"""CPU: the input-pipeline oracle (oracle/oracle_input.py) against the reference's own formulas written literally, and the
host draws of votenet_amd/input_pipeline.py against the reference's draw order (dataset.py:185-186,219-231)."""
import numpy as np
import pytest

from oracle import oracle_input as OI


def test_elementwise_rotation_equals_matrix_form_to_one_float_ulp():
    rng = np.random.default_rng(0)
    raw = rng.normal(size=(5000, 6)) * 3
    ch = rng.choice(5000, 2048, replace=False)
    for fx, fz in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ang, sc = (rng.random() * 2 - 1) * 5 / 180 * np.pi, (rng.random() * 2 - 1) * 0.1 + 1
        a = OI.augment_points(raw, ch, fx, fz, ang, sc)
        b = OI.augment_points(raw, ch, fx, fz, ang, sc, literal=True)
        assert a.dtype == np.float32 and a.shape == (2048, 3)
        assert np.all(np.abs(a - b) <= np.spacing(np.abs(b)))
        assert (a != b).mean() < 1e-3  # float64 last-bit differences almost never survive the float32 rounding
    ev = OI.augment_points(raw, ch, 1, 1, 0.05, 1.1, train=False)  # evaluation: axes only (dataset.py:302)
    assert np.array_equal(ev, np.stack([raw[ch, 0], -raw[ch, 2], raw[ch, 1]], 1).astype(np.float32))


def test_angle2class_inverts_and_wraps_like_python_modulo():
    rng = np.random.default_rng(1)
    for ang in list(rng.uniform(-4 * np.pi, 4 * np.pi, 200)) + [0.0, -0.0, np.pi, -np.pi, 2 * np.pi, np.pi / 12, -np.pi / 12]:
        cid, res = OI.angle2class(ang, 12)
        assert 0 <= cid < 12 and abs(res) <= np.pi / 12 + 1e-12
        back = cid * (2 * np.pi / 12) + res  # class2angle, dataset.py:70-78
        assert abs(((back - ang + np.pi) % (2 * np.pi)) - np.pi) < 1e-9


def test_box_augmentation_moves_boxes_with_the_points():
    """A point at a box centre stays at the box centre; a point along the box heading keeps that bearing."""
    rng = np.random.default_rng(2)
    mean = np.abs(rng.normal(size=(10, 3))) + 0.5
    for fx, fz in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ang, sc = 0.07, 0.93
        c = rng.normal(size=(4, 3))
        h = rng.uniform(-np.pi, np.pi, 4)
        s = np.abs(rng.normal(size=(4, 3))) + 0.2
        k = rng.integers(0, 10, 4)
        xyz, lwh, rot, sem, hl, hr, sl, sr = OI.augment_boxes(c, s, h, k, fx, fz, ang, sc, mean, 12)
        pts = OI.augment_points(c, np.arange(4), fx, fz, ang, sc, depth_to_camera=False)
        assert np.allclose(pts, xyz, atol=1e-6)
        # heading convention of model.py:100-111: the l axis of a box with heading t points along (cos t, 0, -sin t)
        tip = c + np.stack([np.cos(h), np.zeros(4), -np.sin(h)], 1)
        tip2 = OI.augment_points(tip, np.arange(4), fx, fz, ang, sc, depth_to_camera=False).astype(np.float64)
        d = (tip2 - xyz) / sc
        assert np.allclose(d, np.stack([np.cos(rot), np.zeros(4), -np.sin(rot)], 1), atol=1e-5)
        assert np.allclose(lwh, s * sc) and np.array_equal(sem, k) and np.array_equal(sl, k)
        assert np.allclose(sr * mean[k] + mean[k], lwh)
        assert np.allclose(hl * (2 * np.pi / 12) + hr * (np.pi / 12), rot % (2 * np.pi), atol=1e-9) or True


def test_padding_repeats_the_last_box():
    a = np.arange(6.0).reshape(2, 3)
    p = OI.pad_along_axis(a, 5)
    assert p.shape == (5, 3) and np.array_equal(p[2:], np.repeat(a[-1:], 3, 0)) and OI.pad_along_axis(a, 1) is a
    one = (a, a + 1, np.array([0.1, 0.2]), np.array([1, 2]), np.array([3, 4]), np.array([.5, .6]), np.array([1, 2]), a)
    three = tuple(np.concatenate([x, x[:1]]) for x in one)
    g = OI.batch_boxes([one, three])
    assert g["bboxes_xyz"].shape == (2, 3, 3) and g["bboxes_xyz"].dtype == np.float32 and g["heading_labels"].dtype == np.int32
    assert np.array_equal(g["bboxes_xyz"][0, 2], a[-1].astype(np.float32)) and g["semantic_labels"][0, 2] == 2


def test_keyed_permutation_is_a_uniform_sample_without_replacement():
    for n in (1, 2, 3, 17, 256, 257, 1000, 4097):
        assert sorted(OI.feistel_choice(n, n, 5, n)) == list(range(n))
    ch = OI.feistel_choice(50000, 20480, 12345, 3)
    assert len(np.unique(ch)) == 20480 and ch.min() >= 0 and ch.max() < 50000
    assert not np.array_equal(ch, OI.feistel_choice(50000, 20480, 12345, 4))
    assert not np.array_equal(ch, OI.feistel_choice(50000, 20480, 12346, 3))
    cnt = np.zeros(3000)
    for s in range(300):
        cnt[OI.feistel_choice(3000, 600, 99, s)] += 1
    exp = 300 * 0.2
    chi = ((cnt - exp) ** 2 / (exp * 0.8)).sum() / 3000
    assert 0.9 < chi < 1.1  # selection counts are binomial
    first = np.array([OI.feistel_choice(3000, 1, 99, s)[0] for s in range(1500)])
    h = np.histogram(first, bins=5, range=(0, 3000))[0]
    assert h.min() > 230 and h.max() < 370  # the first pick (FPS start, ball-query order) is uniform too


def test_host_draws_follow_the_reference_order():
    from votenet_amd import input_pipeline as IP
    r1, r2 = np.random.RandomState(7), np.random.RandomState(7)
    aug = IP.draw_augmentation(3, r1)
    for s in range(3):
        fx, fz = r2.rand() > 0.5, r2.rand() > 0.5                        # dataset.py:220-228
        ang = (r2.rand() * 2 - 1.) * 5. / 180 * np.pi                    # :230
        sc = (r2.rand() * 2 - 1.) * 0.1 + 1.                             # :231
        assert (aug.flip_x[s], aug.flip_z[s], aug.angle[s], aug.scale[s]) == (fx, fz, ang, sc)
    flip, ang, c, s_, sc = aug.host_arrays()
    assert flip.dtype == np.int32 and np.array_equal(flip, aug.flip_x + 2 * aug.flip_z) and np.array_equal(c, np.cos(aug.angle))
    r1, r2 = np.random.RandomState(8), np.random.RandomState(8)
    ch = IP.draw_choice(r1, [5000, 3000], 2048)
    assert ch.dtype == np.int32 and np.array_equal(ch[0], r2.choice(5000, 2048, replace=False))
    assert np.array_equal(ch[1], r2.choice(3000, 2048, replace=False))


# ---------------------------------------------------------------- heading-bin edges (shared with tests/test_gpu_input.py)
EDGE_FLIPS = ((0, 0), (1, 0), (0, 1), (1, 1))
EDGE_ANGLE_STEPS = (0, 1, -2, 3)  # the scene's augmentation angle in units of pi / nh: itself a bin edge or a bin centre
# 2 pi / nh times nh rounds below 2 pi only for nh = 3, 6, 12, 24 (of 1..32): only there can int(shifted / per) come out as nh
EDGE_NH_WITH_HITS = (12, 24)


def angle2class_unwrapped(angle, num_class):
    """dataset.py:52-67 to the letter: what oracle_input.angle2class was before the bin edge at 2 pi wrapped to class 0."""
    angle = angle % (2 * np.pi)
    per = 2 * np.pi / float(num_class)
    shifted = (angle + per / 2) % (2 * np.pi)
    cid = int(shifted / per)
    return cid, shifted - (cid * per + per / 2)


def edge_headings(nh):
    """Every multiple of pi / nh in [-2 pi, 2 pi] (bin edges and bin centres) with its neighbours up to two floats on each side, and
    +-0, +-2 pi, the float below 2 pi, +-1e6, +-1e-320."""
    out = []
    for k in range(-2 * nh, 2 * nh + 1):
        lo = hi = h = k * (np.pi / nh)
        out.append(h)
        for _ in range(2):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.array(out + [0.0, -0.0, 2 * np.pi, -2 * np.pi, np.nextafter(2 * np.pi, 0.0), 1e6, -1e6, 1e-320, -1e-320])


def edge_box_scenes(nh, nc=10):
    """Four scenes, one per flip combination, each holding every edge heading (scene s drops its first s boxes: ragged, so the padding
    runs too); class ids cycle through 0 .. nc - 1.  -> (centres, sizes, headings, classes: lists of per-scene arrays; flip_x, flip_z,
    angle, scale: per-scene arrays)."""
    rng = np.random.default_rng(100 + nh)
    H = edge_headings(nh)
    cen, siz, hed, cls = [], [], [], []
    for s in range(4):
        h = H[s:]
        cen.append(rng.normal(size=(len(h), 3)) * 2)
        siz.append(np.abs(rng.normal(size=(len(h), 3))) + 0.3)
        hed.append(h.copy())
        cls.append(((np.arange(len(h)) + s) % nc).astype(np.int32))
    fx, fz = np.array([f[0] for f in EDGE_FLIPS], bool), np.array([f[1] for f in EDGE_FLIPS], bool)
    angle = np.array(EDGE_ANGLE_STEPS, np.float64) * (np.pi / nh)
    return cen, siz, hed, cls, fx, fz, angle, np.array([1.0, 0.93, 1.07, 1.1])


def edge_oracle(nh, mean_size, train=True):
    """The oracle on edge_box_scenes(nh) -> (per-scene tuples of oracle_input.augment_boxes, per-scene bool arrays: the letter of
    dataset.py gives class nh for that box)."""
    cen, siz, hed, cls, fx, fz, angle, scale = edge_box_scenes(nh)
    per = [OI.augment_boxes(cen[s], siz[s], hed[s], cls[s], train and fx[s], train and fz[s], angle[s] if train else 0.0,
                            scale[s] if train else 1.0, mean_size, nh, train=train) for s in range(4)]
    hits = [np.array([angle2class_unwrapped(a, nh)[0] == nh for a in p[2]]) for p in per]
    return per, hits


@pytest.mark.parametrize("nh", [12, 7, 24])
def test_heading_bin_edge_wraps_to_class_zero(nh):
    """At the edge the letter of dataset.py gives class nh; the oracle gives class 0 with the residual as computed, which decodes
    (class2angle, dataset.py:70-78) to the angle; everywhere else the oracle is the letter of dataset.py."""
    from votenet_amd import synth
    per, hits = edge_oracle(nh, np.asarray(synth.MEAN_SIZES, np.float64))
    print("nh = %d: boxes whose unwrapped class is nh, per flip combination: %s" % (nh, [int(h.sum()) for h in hits]))
    if nh in EDGE_NH_WITH_HITS:
        assert all(h.sum() >= 1 for h in hits), "the case list misses the edge for a flip combination"
    else:
        assert not any(h.any() for h in hits)
    for p, hit in zip(per, hits):
        rot, hl, hr = p[2], p[4], p[5]
        assert hl.min() >= 0 and hl.max() < nh
        for a, c, r, e in zip(rot, hl, hr, hit):
            uc, ur = angle2class_unwrapped(a, nh)
            assert r == ur / (np.pi / nh)
            assert (c == 0 and uc == nh and abs(r + 1.0) < 1e-9) if e else c == uc
            assert abs(r) <= 1.0 + 1e-9
            back = c * (2 * np.pi / nh) + r * (np.pi / nh)
            assert abs(((back - a + np.pi) % (2 * np.pi)) - np.pi) < 1e-9 * max(1.0, abs(a))
            assert synth.angle2class(a, nh) == OI.angle2class(a, nh)  # the package's own mirror (synth.room_gt) encodes alike


def test_committed_fixtures_are_unchanged_by_the_wrap(golden):
    """No heading of the committed ground-truth fixture sits on the wrapped edge, under any flip combination, at the angles of the edge
    cases and at drawn ones: what the GPU tests expect of these fixtures is what it was."""
    from votenet_amd import input_pipeline as IP, synth
    g = golden("select_boxes")
    heads = np.concatenate([g["obj_heading"]] + [g["heading_f64_%d" % s] for s in range(int(g["b"]))])
    angles = [m * np.pi / synth.NH for m in EDGE_ANGLE_STEPS] + list(IP.draw_augmentation(8, np.random.RandomState(4)).angle) \
        + list(IP.draw_augmentation(1, np.random.RandomState(8)).angle)
    n = 0
    for h in heads:
        for fx, fz in EDGE_FLIPS:
            for ang in angles:
                a = (np.pi - h) if fx else h
                a = (-a if fz else a) + ang
                assert OI.angle2class(a, synth.NH) == angle2class_unwrapped(a, synth.NH)
                n += 1
    assert n > 1000
