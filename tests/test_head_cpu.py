"""The detection head as a value (votenet_amd/head.py) on the CPU: HeadConfig's derived widths and slices, its rejections and
immutability, from_boxes; a CPU-device VoteNetHotPath(head=...) for each head of tests/head_cases.py (the last layer's shape and the
padded copy it runs on, the state_dict); checkpoints of a non-default head (round trip, the header, refusals that leave the net
untouched, load(path, device)); and the synthetic rooms under a head."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from head_cases import HEADS, WIDTH_PAD, head  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
SMALL = (64, 32, 16, 8)


# ---------------------------------------------------------------- HeadConfig
@pytest.mark.parametrize("name", sorted(HEADS))
def test_derived_widths_and_slices(name):
    nh, nc = HEADS[name]
    h = head(name)
    assert (h.nh, h.ns, h.nc) == (nh, nc, nc)
    assert h.width == 5 + 2 * nh + 4 * nc + nc == WIDTH_PAD[name][0]
    order = [h.obj, h.center, h.heading_cls, h.heading_res, h.size_cls, h.size_res, h.sem]
    assert [s.stop - s.start for s in order] == [2, 3, nh, nh, nc, 3 * nc, nc]
    assert order[0].start == 0 and order[-1].stop == h.width and all(a.stop == b.start for a, b in zip(order, order[1:]))
    row = np.arange(h.width)
    assert np.array_equal(row[h.sem], row[-nc:])
    assert h.mean_sizes_f64.shape == h.mean_sizes_f32.shape == (nc, 3)
    assert h.mean_sizes_f64.dtype == np.float64 and h.mean_sizes_f32.dtype == np.float32
    assert h.mean_sizes_f64.flags.c_contiguous and h.mean_sizes_f32.flags.c_contiguous
    assert np.array_equal(h.mean_sizes_f32, h.mean_sizes_f64.astype(np.float32))
    assert h.is_default == (name == "default")


def test_the_default_head_is_the_module_constants():
    from votenet_amd import model as VM
    from votenet_amd import synth
    from votenet_amd.head import HeadConfig
    d = HeadConfig.sunrgbd()
    assert (d.nh, d.ns, d.nc, d.width) == (VM.NH, VM.NS, VM.NC, VM.PROPOSAL_OUT) == (synth.NH, synth.NS, synth.NC, 79)
    assert np.array_equal(d.mean_sizes_f64, synth.MEAN_SIZES) and d.is_default
    assert d == HeadConfig(12, synth.MEAN_SIZES) and hash(d) == hash(HeadConfig(12, synth.MEAN_SIZES.tolist()))
    assert synth.room_head(12, 10) == d and synth.room_head(12, 10).is_default
    other = synth.MEAN_SIZES.copy()
    other[3, 1] = np.nextafter(other[3, 1], 2.0)
    assert HeadConfig(12, other) != d and not HeadConfig(12, other).is_default and HeadConfig(11, synth.MEAN_SIZES) != d


def test_room_head_templates():
    from votenet_amd import synth
    h = synth.room_head(1, 18)
    for c in range(18):
        assert np.array_equal(h.mean_sizes_f64[c], synth.MEAN_SIZES[c % 10] * (1 + 0.15 * (c // 10)))


@pytest.mark.parametrize("args,match", [
    ((0, np.ones((3, 3))), r"nh must be an integer in \[1, 32\] \(the kernels' cap"),
    ((33, np.ones((3, 3))), r"nh must be an integer in \[1, 32\] \(the kernels' cap"),
    ((2.0, np.ones((3, 3))), r"nh must be an integer"),
    ((True, np.ones((3, 3))), r"nh must be an integer"),
    ((2, np.ones((0, 3))), r"nc = len\(mean_sizes\) must be in \[1, 32\] \(the kernels' cap"),
    ((2, np.ones((33, 3))), r"nc = len\(mean_sizes\) must be in \[1, 32\] \(the kernels' cap"),
    ((2, np.ones((3, 2))), r"mean_sizes must have shape \(nc, 3\), got \(3, 2\)"),
    ((2, np.ones(3)), r"mean_sizes must have shape \(nc, 3\)"),
    ((2, np.ones((2, 3, 1))), r"mean_sizes must have shape \(nc, 3\)"),
    ((2, [[1, 1, 1], [1, 0.0, 1]]), r"finite and > 0; template 1"),
    ((2, [[1, -1, 1]]), r"finite and > 0; template 0"),
    ((2, [[1, 1, float("nan")]]), r"finite and > 0; template 0"),
    ((2, [[1, 1, 1], [1, 1, 1], [float("inf"), 1, 1]]), r"finite and > 0; template 2"),
    ((2, [["a", 1, 1]]), r"mean_sizes must be an \(nc, 3\) array of floats"),
])
def test_rejections_by_message(args, match):
    from votenet_amd import InvalidArgumentError
    from votenet_amd.head import HeadConfig
    with pytest.raises(InvalidArgumentError, match=match):
        HeadConfig(*args)


def test_class_names_of_another_length_are_rejected():
    from votenet_amd import InvalidArgumentError
    from votenet_amd.head import HeadConfig
    with pytest.raises(InvalidArgumentError, match=r"2 class_names for 3 classes"):
        HeadConfig(2, np.ones((3, 3)), class_names=["a", "b"])
    h = HeadConfig(2, np.ones((3, 3)), class_names=["a", "b", "c"])
    assert h.class_names == ("a", "b", "c") and HeadConfig.sunrgbd().class_names[0] == "bed"


def test_the_check_loads_no_library_and_touches_no_device():
    """A fresh interpreter: building and rejecting heads loads neither the product library nor a GPU context."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from votenet_amd.head import HeadConfig\nfrom votenet_amd import _lib, synth\nimport torch\n"
            "HeadConfig.sunrgbd(); synth.room_head(1, 18)\n"
            "try:\n    HeadConfig(40, [[1, 1, 1]])\nexcept ValueError:\n    pass\n"
            "assert 'libvotenet' not in open('/proc/self/maps').read()\n"
            "assert not torch.cuda.is_initialized()\nprint('ok')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_immutability():
    from votenet_amd.head import HeadConfig
    src = np.ones((3, 3))
    h = HeadConfig(2, src)
    src[0, 0] = 5.0                                   # the head holds a copy
    assert h.mean_sizes_f64[0, 0] == 1.0
    for name, value in (("nh", 3), ("nc", 4), ("class_names", ("x",)), ("anything", 1)):
        with pytest.raises(AttributeError):
            setattr(h, name, value)
    with pytest.raises(AttributeError):
        del h.nh
    with pytest.raises(ValueError):
        h.mean_sizes_f64[0, 0] = 2.0
    with pytest.raises(ValueError):
        h.mean_sizes_f32[0, 0] = 2.0
    assert not hasattr(h, "__dict__") and (h.nh, h.nc) == (2, 3)
    import votenet_amd.head as H
    assert not any(isinstance(v, (list, dict, set)) for k, v in vars(H).items() if not k.startswith("__")), "a module-level mutable"


def test_from_boxes_against_a_numpy_mean():
    from votenet_amd import InvalidArgumentError
    from votenet_amd.head import HeadConfig
    rng = np.random.default_rng(3)
    cls = np.concatenate([np.arange(5), rng.integers(0, 5, 95)]).astype(np.int32)
    size = rng.random((100, 3)) * 2 + 0.1
    h = HeadConfig.from_boxes(size, cls, 5, 1)
    want = np.stack([size[cls == c].mean(0) for c in range(5)])
    assert (h.nh, h.nc) == (1, 5) and np.array_equal(h.mean_sizes_f64, want)
    # tensors as select_boxes / boxes_from_labels return them (float64 sizes, int32 classes); float32 sizes are averaged in float64
    t = HeadConfig.from_boxes(torch.from_numpy(size), torch.from_numpy(cls), 5, 1)
    assert t == h
    f = HeadConfig.from_boxes(size.astype(np.float32), cls, 5, 3)
    assert np.array_equal(f.mean_sizes_f64, np.stack([size.astype(np.float32).astype(np.float64)[cls == c].mean(0) for c in range(5)]))
    with pytest.raises(InvalidArgumentError, match=r"class 5 has no box"):
        HeadConfig.from_boxes(size, cls, 6, 1)
    with pytest.raises(InvalidArgumentError, match=r"class 2 has no box"):
        HeadConfig.from_boxes(size[cls != 2], cls[cls != 2], 5, 1)
    with pytest.raises(InvalidArgumentError, match=r"nc must be an integer in \[1, 32\]"):
        HeadConfig.from_boxes(size, cls, 33, 1)


# ---------------------------------------------------------------- a net under each head
@pytest.mark.parametrize("name", sorted(HEADS))
def test_net_last_layer_and_state_dict(name):
    from votenet_amd import model as VM
    h = head(name)
    net = VM.VoteNetHotPath(CPU, seed=1, npoints=SMALL, head=h)
    assert net.head is h
    last = net.proposal.mlp2[-1]
    width, pad = WIDTH_PAD[name]
    assert (last.cin, last.cout, last.bn, last.relu) == (128, width, False, False) and last.cout_pad == pad
    assert tuple(net.store.views[last.name + "/W"].shape) == (128, width) and tuple(net.store.views[last.name + "/b"].shape) == (width,)
    assert net.make_cotangents(2)["proposals_output"].shape == (2, VM.PROPOSAL_NUM, width)
    sd = net.state_dict()
    base = VM.VoteNetHotPath(CPU, seed=1, npoints=SMALL).state_dict()
    assert list(sd) == list(base)
    ours = {k for k in sd if k.startswith("proposal/conv_post_2/")}
    assert ours == {"proposal/conv_post_2/" + s + t for s in ("W", "b") for t in ("", "/Adam", "/Adam_1")}
    for k in sd:
        if k in ours:
            assert sd[k].shape == ((1, 1, 128, width) if "/W" in k else (width,)), k
        else:
            assert sd[k].shape == base[k].shape, k


def test_head_must_be_a_head_config():
    from votenet_amd import InvalidArgumentError
    from votenet_amd import model as VM
    with pytest.raises(InvalidArgumentError, match="head must be a head.HeadConfig"):
        VM.VoteNetHotPath(CPU, npoints=SMALL, head=(1, 18))
    from votenet_amd.head import HeadConfig
    assert VM.VoteNetHotPath(CPU, npoints=SMALL).head is HeadConfig.sunrgbd()


# ---------------------------------------------------------------- checkpoints
def _golden_names():
    out = []
    with open(os.path.join(ROOT, "tests", "golden", "votenet_variable_names.txt")) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                key, shape = line.split(" ", 1)
                out.append((key, tuple(int(v) for v in shape.strip().strip("()").split(",") if v.strip())))
    return out


def _header(path):
    from votenet_amd import checkpoint as C
    with np.load(path, allow_pickle=False) as z:
        return json.loads(z[C.HEADER_KEY].tobytes().decode()), [k for k in z.files if k != C.HEADER_KEY]


def _scribble(net, seed):
    g = torch.Generator().manual_seed(seed)
    net.init_optimizer(2e-4)
    for t in net._ema_state().values():
        t[2].copy_(torch.randn(t.shape[1], generator=g))
        t[3].copy_(torch.rand(t.shape[1], generator=g) + 0.5)
    net._step = 9


def _bytes(net):
    net._ema_state()
    opt = (net._m.clone(), net._v.clone(), net._step, net._lr) if hasattr(net, "_seg") else None
    return net.store.flat.clone(), net._ema_flat.clone(), opt, net.store.generation, net._ema_version


def _unchanged(before, net):
    after = _bytes(net)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[3:] == after[3:]
    assert (before[2] is None) == (after[2] is None)
    if before[2] is not None:
        assert torch.equal(before[2][0], after[2][0]) and torch.equal(before[2][1], after[2][1]) and before[2][2:] == after[2][2:]


def test_default_head_file_is_what_it_was(tmp_path):
    """Key for key the golden variable list, field for field the header of a file from before heads existed: no mean_sizes."""
    from votenet_amd import mlp as M
    from votenet_amd import model as VM
    from votenet_amd.head import HeadConfig
    for kw in ({}, dict(head=HeadConfig.sunrgbd())):
        net = VM.VoteNetHotPath(CPU, seed=2, **kw)
        sd = net.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == _golden_names()
        p = tmp_path / "default.npz"
        net.save(p)
        hdr, keys = _header(p)
        assert hdr == dict(format="votenet_amd checkpoint", version=1, npoints=[2048, 1024, 512, 256], NH=12, NS=10, NC=10,
                           bn_momentum=net.BN_MOMENTUM, bn_epsilon=M.BN_EPS, optimizer=True)
        assert list(hdr) == ["format", "version", "npoints", "NH", "NS", "NC", "bn_momentum", "bn_epsilon", "optimizer"]
        assert keys == [k for k, _ in _golden_names()]


def test_scannet_round_trip_and_header(tmp_path):
    from votenet_amd import model as VM
    h = head("scannet")
    src = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL, head=h)
    _scribble(src, 1)
    p = tmp_path / "scannet.npz"
    src.save(p)
    hdr, _ = _header(p)
    assert (hdr["NH"], hdr["NS"], hdr["NC"]) == (1, 18, 18)
    assert isinstance(hdr["mean_sizes"], list) and np.array_equal(np.array(hdr["mean_sizes"], np.float64), h.mean_sizes_f64)  # exactly
    dst = VM.VoteNetHotPath(CPU, seed=4, npoints=SMALL, head=h)
    assert not torch.equal(dst.store.flat, src.store.flat)
    dst.load(p)
    a, b = src.state_dict(), dst.state_dict()
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert dst._step == 9 and dst._lr == 2e-4
    # load(path, device) rebuilds the head, the level sizes and the state
    made = VM.VoteNetHotPath.load(p, CPU)
    assert made.head == h and not made.head.is_default and [m.npoint for m in (made.sa1, made.sa2, made.sa3, made.sa4)] == list(SMALL)
    c = made.state_dict()
    assert list(a) == list(c) and all(np.array_equal(a[k], c[k]) for k in a)
    # ... and for a file without templates, the default head
    d = VM.VoteNetHotPath(CPU, seed=5, npoints=SMALL)
    d.save(tmp_path / "d.npz")
    assert VM.VoteNetHotPath.load(tmp_path / "d.npz", CPU).head.is_default


def test_loads_into_another_head_are_refused_and_write_nothing(tmp_path):
    from votenet_amd import model as VM
    from votenet_amd.head import HeadConfig
    h = head("scannet")
    scan = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL, head=h)
    dflt = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL)
    ulp = h.mean_sizes_f64.copy()
    ulp[7, 2] = np.nextafter(ulp[7, 2], 10.0)
    near = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL, head=HeadConfig(1, ulp))
    for net in (scan, dflt, near):
        _scribble(net, 2)
    scan.save(tmp_path / "scan.npz")
    dflt.save(tmp_path / "dflt.npz")
    for dst, file, fields in ((dflt, "scan.npz", ("header NH: file 1, model 12", "header NC: file 18, model 10", "header mean_sizes")),
                              (scan, "dflt.npz", ("header NH: file 12, model 1", "header NC: file 10, model 18", "header mean_sizes")),
                              (near, "scan.npz", ("header mean_sizes", "template 7"))):
        before = _bytes(dst)
        with pytest.raises(ValueError) as e:
            dst.load(tmp_path / file)
        for f in fields:
            assert f in str(e.value), (f, str(e.value))
        assert "nothing was loaded" in str(e.value)
        _unchanged(before, dst)
    with pytest.raises(ValueError) as e:  # the one-ulp file names no other field: shapes, NH and NC all fit
        near.load(tmp_path / "scan.npz")
    assert "header NH" not in str(e.value) and "header NC" not in str(e.value) and "expected float32" not in str(e.value)


# ---------------------------------------------------------------- the synthetic rooms under a head
@pytest.mark.parametrize("seed", [0, 7, 1000])
def test_default_rooms_are_unchanged(seed):
    """The default head, given or not, leaves every array what the recorded digests of the parent's generator say."""
    import hashlib
    from votenet_amd import synth
    from votenet_amd.head import HeadConfig

    def digest(arrays):
        m = hashlib.sha256()
        for a in arrays:
            m.update(np.ascontiguousarray(a).tobytes())
        return m.hexdigest()[:16]
    want = PARENT_DIGESTS[seed]
    for kw in ({}, dict(head=HeadConfig.sunrgbd()), dict(head=synth.room_head(12, 10))):
        pts, boxes = synth.room_scene(500, seed, **kw)
        inst, sem = synth.room_scene_labels(500, seed, **kw)
        gt = synth.room_gt(2, 500, seed, **kw)
        got = (digest([pts, boxes]), digest([inst, sem]), digest([gt[k] for k in sorted(gt)]))
        assert got == want, (seed, kw, got)


# sha256 prefixes of room_scene(500, seed), room_scene_labels(500, seed), room_gt(2, 500, seed) (keys sorted) at the parent commit
PARENT_DIGESTS = {
    0: ("e2616c942b4ffeab", "8cc91b4df38e3850", "928b44094f9719df"),
    7: ("17014994061458c6", "b33310e197bbe398", "369303d65c254f1c"),
    1000: ("6537c62ba6b847cd", "4b70da7a29486ae5", "c9f01042a53ef856"),
}


def test_rooms_under_the_scannet_head():
    from votenet_amd import synth
    h = synth.room_head(1, 18)
    T = h.mean_sizes_f64
    seen = set()
    for seed in range(40, 52):
        pts, boxes = synth.room_scene(600, seed, head=h)
        inst, sem = synth.room_scene_labels(600, seed, head=h)
        cls = boxes[:, 7].astype(int)
        assert pts.shape == (600, 3) and ((0 <= cls) & (cls < 18)).all() and (boxes[:, 6] == 0).all()
        assert ((sem >= -1) & (sem < 18)).all() and all((sem[inst == i] == cls[i]).all() for i in range(len(boxes)))
        seen |= set(cls.tolist())
        ratio = boxes[:, 3:6].astype(np.float64) / T[cls]
        assert (ratio > 0.8 - 1e-6).all() and (ratio < 1.2 + 1e-6).all()
    assert max(seen) >= 10, "no class beyond the ten SUN RGB-D ones was drawn"
    gt = synth.room_gt(2, 600, 40, head=h)
    assert (gt["heading_labels"] == 0).all() and (gt["heading_residuals"] == 0).all() and (gt["bboxes_roty"] == 0).all()
    assert np.array_equal(gt["size_labels"], gt["semantic_labels"]) and gt["semantic_labels"].max() < 18
    for s in range(2):
        boxes = synth.room_scene(600, 40 + s, head=h)[1].astype(np.float64)
        k = len(boxes)
        c = boxes[:, 7].astype(int)
        assert np.array_equal(gt["semantic_labels"][s, :k], c)
        assert np.array_equal(gt["size_residuals"][s, :k], ((boxes[:, 3:6] - T[c]) / T[c]).astype(np.float32))
    # two heading bins: the angles stay, the bins are angle2class's
    g2 = synth.room_gt(1, 600, 40, head=synth.room_head(2, 3))
    b2 = synth.room_scene(600, 40, head=synth.room_head(2, 3))[1].astype(np.float64)
    assert (b2[:, 6] != 0).any() and b2[:, 7].max() < 3
    for j, ang in enumerate(b2[:, 6]):
        hc, hr = synth.angle2class(ang, 2)
        assert g2["heading_labels"][0, j] == hc and g2["heading_residuals"][0, j] == np.float32(hr / (np.pi / 2))


# ---------------------------------------------------------------- the public functions' head= on the host
def test_eval_det_classes_follow_the_head():
    """eval_det_cls is host logic; the class loop's range is the head's (a label beyond it is counted nowhere) -- checked through
    finalize_records, which needs no device."""
    from votenet_amd import InvalidArgumentError
    from votenet_amd import evaluator as E
    rec = np.zeros((3, 4), np.int32)
    rec[:, 0] = np.array([0.9, 0.8, 0.7], np.float32).view(np.int32)
    rec[:, 1] = [17 | (1 << 8), 17, 3 | (1 << 8)]
    rec[:, 3] = [0, 1, 2]
    npos = np.zeros(18, np.int64)
    npos[17], npos[3] = 2, 1
    res = E.finalize_records(rec, npos, (0.25,), head=head("scannet"))
    assert sorted(res[0.25]["ap"]) == [3, 17] and res[0.25]["ap"][3] == 1.0 and res[0.25]["ap"][17] == 0.5
    with pytest.raises(InvalidArgumentError, match="npos holds 18 classes, the head has 10"):
        E.finalize_records(rec, npos, (0.25,), head=head("default"))
