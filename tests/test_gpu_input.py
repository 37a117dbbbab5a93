"""GPU: votenet_subsample_augment / votenet_augment_boxes (the step before the hot path) against oracle/oracle_input.py.
Bar: bit-exact -- float64 arithmetic in the reference's order, one rounding to float32; integer labels exact."""
import numpy as np
import pytest
import torch

from oracle import oracle_input as OI

pytestmark = pytest.mark.gpu


def _scenes(b, seed, lo=2500, hi=6000, cols=6):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(int(rng.integers(lo, hi)), cols)) * np.array([2.0, 3.0, 1.0] + [1.0] * (cols - 3)) for _ in range(b)]


@pytest.mark.parametrize("b,n_out,f64", [(3, 2048, True), (19, 1024, False), (1, 2500, True)])
def test_points_with_host_choice_bit_exact(hiplib, dev, b, n_out, f64):
    from votenet_amd import input_pipeline as IP
    scenes = _scenes(b, 10 + b)
    if not f64:
        scenes = [s.astype(np.float32) for s in scenes]
    raw, off = IP.pack_ragged(scenes, dev)
    aug = IP.draw_augmentation(b, np.random.RandomState(b))
    ch = IP.draw_choice(np.random.RandomState(1), [len(s) for s in scenes], n_out)
    got = IP.subsample_augment(raw, off, n_out, aug, ch).cpu().numpy()
    for s in range(b):
        exp = OI.augment_points(scenes[s], ch[s], aug.flip_x[s], aug.flip_z[s], aug.angle[s], aug.scale[s])
        assert np.array_equal(got[s], exp), s
    ev = IP.subsample_augment(raw, off, n_out, None, ch, depth_to_camera=False).cpu().numpy()
    for s in range(b):
        assert np.array_equal(ev[s], np.asarray(scenes[s], np.float64)[ch[s], :3].astype(np.float32))


def test_points_with_device_draw_bit_exact_and_without_replacement(hiplib, dev):
    from votenet_amd import input_pipeline as IP
    b, n_out = 18, 2048  # two launches of <= 16 scenes: scene numbers keep counting
    scenes = _scenes(b, 3, cols=3)
    raw, off = IP.pack_ragged(scenes, dev)
    aug = IP.draw_augmentation(b, np.random.RandomState(5))
    got = IP.subsample_augment(raw, off, n_out, aug, None, seed=0x1234567890AB, scene0=40).cpu().numpy()
    for s in range(b):
        ch = OI.feistel_choice(len(scenes[s]), n_out, 0x1234567890AB, 40 + s)
        assert len(np.unique(ch)) == n_out
        exp = OI.augment_points(scenes[s], ch, aug.flip_x[s], aug.flip_z[s], aug.angle[s], aug.scale[s])
        assert np.array_equal(got[s], exp), s
    again = IP.subsample_augment(raw, off, n_out, aug, None, seed=0x1234567890AB, scene0=40).cpu().numpy()
    other = IP.subsample_augment(raw, off, n_out, aug, None, seed=0x1234567890AC, scene0=40).cpu().numpy()
    assert np.array_equal(got, again) and not np.array_equal(got, other)


def test_points_full_size_properties(hiplib, dev):
    """BASELINE size: 8 scenes x 50 000 raw points -> 20 480 (config.POINT_NUM): every output row is a distinct raw row
    (replace=False), isometry up to the scale, evaluation = pure row selection."""
    from votenet_amd import input_pipeline as IP
    b, n_raw, n_out = 8, 50000, 20480
    rng = np.random.default_rng(0)
    rawn = rng.normal(size=(b * n_raw, 3)).astype(np.float32)
    raw = torch.from_numpy(rawn).to(dev)
    off = np.arange(b + 1) * n_raw
    ev = IP.subsample_augment(raw, off, n_out, None, None, seed=1).cpu().numpy()
    for s in range(b):
        sc = rawn[s * n_raw:(s + 1) * n_raw]
        cam = np.stack([sc[:, 0], -sc[:, 2], sc[:, 1]], 1)
        keys = {r.tobytes() for r in cam}
        rows = [r.tobytes() for r in ev[s]]
        assert len(set(rows)) == n_out and all(r in keys for r in rows)
    aug = IP.draw_augmentation(b, np.random.RandomState(0))
    tr = IP.subsample_augment(raw, off, n_out, aug, None, seed=1).cpu().numpy().astype(np.float64)
    assert np.allclose(np.linalg.norm(tr, axis=2), np.linalg.norm(ev.astype(np.float64), axis=2) * aug.scale[:, None], rtol=1e-6, atol=1e-6)
    assert np.allclose(tr[..., 1], ev[..., 1] * aug.scale[:, None], rtol=1e-6)


def test_points_argument_errors(hiplib, dev):
    from votenet_amd import input_pipeline as IP, _lib
    raw = torch.zeros(100, 3, device=dev)
    off = np.array([0, 60, 100])
    with pytest.raises(_lib.InvalidArgumentError):  # 40 points, 50 wanted: numpy raises for replace=False too
        IP.subsample_augment(raw, off, 50)
    with pytest.raises(_lib.InvalidArgumentError):
        IP.subsample_augment(raw, off, 10, choice=np.full((2, 10), 70))
    with pytest.raises(_lib.InvalidArgumentError):
        IP.subsample_augment(raw, off, 10, aug=IP.draw_augmentation(3))
    with pytest.raises(_lib.InvalidArgumentError):
        IP.subsample_augment(torch.zeros(100, 2, device=dev), off, 10)
    assert IP.subsample_augment(raw, off, 40).shape == (2, 40, 3)


@pytest.mark.parametrize("b,train", [(4, True), (17, True), (3, False)])
def test_boxes_bit_exact(hiplib, dev, b, train):
    from votenet_amd import input_pipeline as IP, synth
    rng = np.random.default_rng(b)
    cnt = rng.integers(1, 12, b)
    cen = [rng.normal(size=(c, 3)) * 2 for c in cnt]
    siz = [np.abs(rng.normal(size=(c, 3))) + 0.3 for c in cnt]
    hed = [rng.uniform(-2 * np.pi, 2 * np.pi, c) for c in cnt]
    hed[0][0] = 0.0
    cls = [rng.integers(0, 10, c).astype(np.int32) for c in cnt]
    aug = IP.draw_augmentation(b, np.random.RandomState(b)) if train else None
    dc, off = IP.pack_ragged(cen, dev)
    ds, _ = IP.pack_ragged(siz, dev)
    dh, _ = IP.pack_ragged(hed, dev)
    dk, _ = IP.pack_ragged(cls, dev)
    got = IP.augment_boxes(dc, ds, dh, dk, off, aug)
    per = [OI.augment_boxes(cen[s], siz[s], hed[s], cls[s], train and aug.flip_x[s], train and aug.flip_z[s],
                            aug.angle[s] if train else 0.0, aug.scale[s] if train else 1.0, synth.MEAN_SIZES, synth.NH, train=train)
           for s in range(b)]
    exp = OI.batch_boxes(per)
    assert set(got) == set(exp)
    for k in exp:
        g = got[k].cpu().numpy()
        assert g.dtype == exp[k].dtype and g.shape == exp[k].shape, k
        assert np.array_equal(g, exp[k]), k
    # the result feeds the loss graph directly
    assert got["bboxes_xyz"].shape[1] == cnt.max()


def test_boxes_argument_errors(hiplib, dev):
    from votenet_amd import input_pipeline as IP, _lib
    z3 = torch.zeros(4, 3, dtype=torch.float64, device=dev)
    z1 = torch.zeros(4, dtype=torch.float64, device=dev)
    k = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.InvalidArgumentError):  # a scene without boxes (dataset.py:300 skips it)
        IP.augment_boxes(z3, z3, z1, k, np.array([0, 2, 2, 4]))
    with pytest.raises(_lib.InvalidArgumentError):
        IP.augment_boxes(z3, z3, z1, k, np.array([0, 2, 6]))
    out = IP.augment_boxes(z3, z3 + 1, z1, k, np.array([0, 1, 4]))
    assert out["bboxes_lwh"].shape == (2, 3, 3) and torch.equal(out["bboxes_lwh"][0, 2], out["bboxes_lwh"][0, 0])


def test_pipeline_output_feeds_the_train_step(hiplib, dev):
    """raw clouds + ragged boxes -> subsample / augment / encode / pad on the device -> one train step on the result: the
    eight ground-truth tensors have the layout and dtypes the loss graph takes, the points the layout the backbone takes."""
    from votenet_amd import input_pipeline as IP, synth
    from votenet_amd.model import VoteNetHotPath
    b, n_raw, n_out = 2, 30000, 20480
    raws, cen, siz, hed, cls = [], [], [], [], []
    for s in range(b):
        pts, boxes = synth.room_scene(n_raw, 4000 + s)
        cam = pts.astype(np.float64)
        raws.append(np.stack([cam[:, 0], cam[:, 2], -cam[:, 1]], 1))  # camera -> upright depth axes (sunutils.py:79-84)
        bx = boxes.astype(np.float64)
        cen.append(bx[:, :3]), siz.append(bx[:, 3:6]), hed.append(bx[:, 6]), cls.append(bx[:, 7].astype(np.int32))
    raw, off = IP.pack_ragged(raws, dev)
    aug = IP.draw_augmentation(b, np.random.RandomState(3))
    x = IP.subsample_augment(raw, off, n_out, aug, None, seed=9)
    dc, boff = IP.pack_ragged(cen, dev)
    gt = IP.augment_boxes(dc, IP.pack_ragged(siz, dev)[0], IP.pack_ragged(hed, dev)[0], IP.pack_ragged(cls, dev)[0], boff, aug)
    assert x.shape == (b, n_out, 3) and gt["bboxes_xyz"].shape[0] == b
    # augmented points still lie on their augmented boxes: every box centre has points within half its diagonal
    d = (x[:, :, None, :] - gt["bboxes_xyz"][:, None, :, :]).norm(dim=-1)
    assert bool((d.min(1).values < gt["bboxes_lwh"].norm(dim=-1) * 0.75).all())
    net = VoteNetHotPath(dev, seed=1)
    net.train_step(x, gt=gt)
    assert bool(torch.isfinite(net.last_losses[:10]).all()) and float(net.last_losses[10]) > 0  # positives were assigned
    assert bool(torch.isfinite(net.store.flat).all())


# ---------------------------------------------------------------- heading-bin edges
@pytest.mark.parametrize("nh", [12, 7, 24])
def test_boxes_heading_bin_edges(hiplib, dev, nh):
    """votenet_augment_boxes on headings at and one / two floats beside every bin edge and bin centre (test_oracle_input.edge_headings),
    through all four flip combinations with augmentation angles that are multiples of pi / nh, and once without augmentation; class ids
    0 .. nc - 1.  For nh = 12 and 24 the list holds, for every flip combination, boxes for which the letter of dataset.py gives class nh
    (asserted); the kernel and the oracle give class 0 there.  Every output bit for bit, every heading label in [0, nh)."""
    from test_oracle_input import EDGE_NH_WITH_HITS, edge_box_scenes, edge_oracle
    from votenet_amd import input_pipeline as IP, synth
    cen, siz, hed, cls, fx, fz, angle, scale = edge_box_scenes(nh)
    assert {0, len(synth.MEAN_SIZES) - 1} <= set(np.concatenate(cls).tolist())
    dc, off = IP.pack_ragged(cen, dev)
    ds, dh, dk = IP.pack_ragged(siz, dev)[0], IP.pack_ragged(hed, dev)[0], IP.pack_ragged(cls, dev)[0]
    for train in (True, False):
        per, hits = edge_oracle(nh, synth.MEAN_SIZES, train=train)
        print("nh = %d train = %s: boxes whose unwrapped class is nh, per scene: %s" % (nh, train, [int(h.sum()) for h in hits]))
        if train and nh in EDGE_NH_WITH_HITS:
            assert all(h.sum() >= 1 for h in hits), "the case list misses the edge for a flip combination"
        exp = OI.batch_boxes(per)
        got = IP.augment_boxes(dc, ds, dh, dk, off, IP.Augmentation(fx, fz, angle, scale) if train else None, nh=nh)
        assert set(got) == set(exp)
        for k in exp:
            g = got[k].cpu().numpy()
            assert g.dtype == exp[k].dtype and g.shape == exp[k].shape, k
            assert np.array_equal(g, exp[k]), (k, train, np.argwhere(g != exp[k])[:4].tolist())
        hl = got["heading_labels"].cpu().numpy()
        assert hl.min() >= 0 and hl.max() < nh
        for s, h in enumerate(hits):
            assert (hl[s, :len(h)][h] == 0).all()


# ---------------------------------------------------------------- the device draw at the width boundaries of feistel_perm
DRAW_BATCHES = {                                    # name -> (scene sizes, n_out): ragged inside one launch; n_out <= the smallest scene
    "tiny-n1": ([1, 2, 3, 4, 5], 1),
    "whole-1": ([1] * 3, 1), "whole-2": ([2] * 3, 2), "whole-3": ([3] * 2, 3), "whole-4": ([4] * 2, 4), "whole-5": ([5] * 2, 5),
    "n15": ([15, 16, 17, 255, 256, 257, 15, 4095, 4096, 4097, 16, 16384, 16385, 17, 65536, 65537, 15, 16, 17, 255], 15),
    "n255": ([255, 256, 257, 4095, 4096, 4097, 16384, 16385, 65536, 65537, 255, 256, 257, 4095, 4096, 4097, 65537, 256], 255),
    "n256": ([256, 257, 4095, 4096, 4097, 16384, 16385, 65536, 65537, 256, 257, 4096, 4097, 16385, 65536, 65537, 256, 257], 256),
}
for _n in (15, 16, 17, 257):                       # n == n_out beside the widths 16 and 256 too
    DRAW_BATCHES["whole-%d" % _n] = ([_n] * 2, _n)
DRAW_SEEDS = (0x1234567890AB, 7)                    # one above 2^32 (both halves of the key), one below
DRAW_SCENE0 = 2 ** 32 - 3                           # scene0 + s + 1 crosses 2^32 inside the batch: the 32-bit wrap of scene_key


def draw_scenes(sizes):
    """Raw clouds whose x column is the row number (exact in float32 up to 2^24): the drawn row can be read off the output."""
    return [np.stack([np.arange(n), np.full(n, float(i)), np.zeros(n)], 1).astype(np.float32) for i, n in enumerate(sizes)]


def check_draw(rows, sizes, n_out, seed, scene0, what):
    """rows (b, n_out): the raw row numbers an entry drew -> equal to oracle_input.feistel_choice row for row; inside [0, n), distinct,
    and a whole permutation where n == n_out."""
    for s, n in enumerate(sizes):
        want = OI.feistel_choice(n, n_out, seed, scene0 + s)
        assert np.array_equal(rows[s], want), (what, s, n, rows[s][:8].tolist(), want[:8].tolist())
        assert rows[s].min() >= 0 and rows[s].max() < n and len(set(rows[s].tolist())) == n_out, (what, s, n)
        if n == n_out:
            assert sorted(rows[s].tolist()) == list(range(n)), (what, s, n)


@pytest.mark.parametrize("name", sorted(DRAW_BATCHES))
def test_device_draw_equals_its_restatement_at_the_width_boundaries(hiplib, dev, name):
    """subsample_augment with choice=None, aug=None against oracle_input.feistel_choice at scene sizes on both sides of every width of
    feistel_perm's loop `while ((1 << bits) < n) bits += 2` (4, 16, 256, 4096, 65536; 16384 is no boundary and must not be one), sizes
    1 .. 5, and n == n_out (the draw is then a whole permutation); scenes of different sizes in one launch and across the 16-scene
    chunk; two seeds; scene numbers that cross 2^32."""
    from votenet_amd import input_pipeline as IP
    sizes, n_out = DRAW_BATCHES[name]
    assert n_out <= min(sizes)
    raw, off = IP.pack_ragged(draw_scenes(sizes), dev)
    for seed in DRAW_SEEDS:
        got = IP.subsample_augment(raw, off, n_out, None, None, seed=seed, scene0=DRAW_SCENE0, depth_to_camera=False).cpu().numpy()
        assert np.array_equal(got[:, :, 1], np.repeat(np.arange(len(sizes), dtype=np.float32)[:, None], n_out, 1))  # rows of its own scene
        check_draw(got[:, :, 0].astype(np.int64), sizes, n_out, seed, DRAW_SCENE0, (name, seed))
