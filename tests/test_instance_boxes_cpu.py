"""CPU: ground-truth boxes from instance-labelled points without a device -- the numpy restatement of
include/votenet_instance_boxes.h (tests/instance_boxes_ref.py) against a plain per-instance Python loop, and the C ABI entry points in
the header, their derived binding, the library's export list and its argument checks."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_boxes_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402

F = np.float32
NAMES = ["votenet_instance_boxes", "votenet_instance_boxes_last_error", "votenet_instance_boxes_workspace_bytes",
         "votenet_instance_point_box"]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def random_scene(seed, b=3, n=300, k=16, n_sem=12):
    """Instances as clumps with every kind of label and coordinate the rule names: unlabelled, ids at and beyond k, the int limits,
    NaN / Inf coordinates, -0.0, labels outside class_map, class_map values of -1 and beyond n_class."""
    rng = np.random.default_rng(seed)
    instance = rng.integers(-2, k + 3, (b, n)).astype(np.int32)
    instance[1][instance[1] == 7] = 8  # id 7 is absent from scene 1
    instance[:, ::37] = INT_MIN
    instance[:, 5::41] = INT_MAX
    points = (rng.normal(size=(b, n, 3)) * 2).astype(F)
    points[rng.random((b, n, 3)) < 0.02] = np.nan
    points[rng.random((b, n, 3)) < 0.01] = np.inf
    points[rng.random((b, n, 3)) < 0.01] = -np.inf
    points[rng.random((b, n, 3)) < 0.05] = -0.0
    semantic = np.broadcast_to(((np.arange(k + 3) * 5) % (n_sem + 2) - 1)[None], (b, k + 3))  # one label per id, some outside [0, n_sem)
    semantic = np.take_along_axis(semantic, np.clip(instance, 0, k + 2), 1).astype(np.int32)
    semantic[rng.random((b, n)) < 0.1] = 3  # points of an instance that disagree
    class_map = rng.integers(-1, 13, n_sem).astype(np.int32)  # n_class = 10: 10, 11, 12 are no object class
    return points, instance, semantic, class_map


def plain_loop(points, instance, semantic, class_map, k, n_class, min_points):
    """The rule, one point at a time in Python floats and ints: no numpy reduction shared with the restatement."""
    b, n = instance.shape
    out = dict(center=[], size=[], heading=[], cls=[], instance_id=[], n_points=[], offset=[0])
    status, count, slot = np.full((b, k), 3, np.int32), np.zeros((b, k), np.int32), np.full((b, k), -1, np.int32)
    ignored, point_box = np.zeros((b, 3), np.int32), np.full((b, n), -1, np.int32)
    for s in range(b):
        acc = {}
        for p in range(n):
            i, xyz = int(instance[s, p]), [float(v) for v in points[s, p]]
            if i < 0:
                ignored[s, 0] += 1
            elif i >= k:
                ignored[s, 1] += 1
            elif not all(math.isfinite(v) for v in xyz):
                ignored[s, 2] += 1
            else:
                xyz = [v + 0.0 for v in xyz]
                e = acc.setdefault(i, dict(lo=list(xyz), hi=list(xyz), n=0, first=p))
                e["lo"] = [a if a <= v else v for a, v in zip(e["lo"], xyz)]
                e["hi"] = [a if a >= v else v for a, v in zip(e["hi"], xyz)]
                e["n"] += 1
        rows = 0
        for i in sorted(acc):
            e = acc[i]
            count[s, i] = e["n"]
            sem = int(semantic[s, e["first"]])
            cls = int(class_map[sem]) if 0 <= sem < len(class_map) else -1
            if cls < 0 or cls >= n_class:
                status[s, i] = 1
            elif e["n"] < min_points:
                status[s, i] = 2
            else:
                status[s, i], slot[s, i] = 0, rows
                rows += 1
                out["center"].append([(lo + hi) * 0.5 for lo, hi in zip(e["lo"], e["hi"])])
                out["size"].append([hi - lo for lo, hi in zip(e["lo"], e["hi"])])
                out["heading"].append(0.0), out["cls"].append(cls), out["instance_id"].append(i), out["n_points"].append(e["n"])
        out["offset"].append(out["offset"][-1] + rows)
        for p in range(n):
            i = int(instance[s, p])
            if 0 <= i < k and all(math.isfinite(float(v)) for v in points[s, p]):
                point_box[s, p] = slot[s, i]
    nk = out["offset"][-1]
    res = {"center": np.array(out["center"], np.float64).reshape(nk, 3), "size": np.array(out["size"], np.float64).reshape(nk, 3),
           "heading": np.array(out["heading"], np.float64).reshape(nk), "box_offset": np.array(out["offset"], np.int64)}
    for key in ("cls", "instance_id", "n_points"):
        res[key] = np.array(out[key], np.int32).reshape(nk)
    res.update(status=status, inst_count=count, slot=slot, ignored=ignored, point_box=point_box)
    return res


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("seed,min_points", [(0, 1), (1, 13), (2, 16)])
def test_restatement_equals_a_plain_loop_over_the_points(seed, min_points):
    points, instance, semantic, class_map = random_scene(seed)
    got = R.boxes_from_labels(points, instance, semantic, class_map, k=16, n_class=10, min_points=min_points)
    exp = plain_loop(points, instance, semantic, class_map, 16, 10, min_points)
    assert R.same_bytes(got, exp) == [] and sorted(got) == sorted(exp)
    st = got["status"]
    print("status counts", np.bincount(st.ravel(), minlength=4), "ignored", got["ignored"].tolist(), "rows", got["box_offset"].tolist())
    assert (got["ignored"] > 0).all() and got["box_offset"][-1] >= 3
    assert {0, 1, 3}.issubset(set(st.ravel().tolist())) and (min_points == 1 or 2 in st) and st[1, 7] == 3


def test_restatement_on_a_case_worked_by_hand():
    pts = np.array([[[1, 2, 3], [-1, 5, -0.0], [np.nan, 0, 0], [7, 7, 7], [3, -2, 0.5], [9, 9, 9], [4, 4, np.inf]]], F)
    inst = np.array([[0, 0, 0, 1, 0, -1, 5]], np.int32)
    sem = np.array([[2, 0, 0, 1, 0, 0, 0]], np.int32)
    r = R.boxes_from_labels(pts, inst, sem, np.array([-1, 10, 4], np.int32), k=4, n_class=10, min_points=2)
    assert r["status"].tolist() == [[0, 1, 3, 3]] and r["inst_count"].tolist() == [[3, 1, 0, 0]] and r["slot"].tolist() == [[0, -1, -1, -1]]
    assert r["ignored"].tolist() == [[1, 1, 1]] and r["box_offset"].tolist() == [0, 1]
    assert r["center"].tolist() == [[1.0, 1.5, 1.5]] and r["size"].tolist() == [[4.0, 7.0, 3.0]] and r["heading"].tolist() == [0.0]
    assert not np.signbit(r["center"]).any() and not np.signbit(r["size"]).any()
    assert r["cls"].tolist() == [4] and r["instance_id"].tolist() == [0] and r["n_points"].tolist() == [3]
    assert r["point_box"].tolist() == [[0, 0, -1, -1, 0, -1, -1]]
    assert R.boxes_from_labels(pts, inst, sem, np.array([-1, 9, 4], np.int32), k=4, n_class=10, min_points=2)["status"][0, 1] == 2


# ------------------------------------------------------------------ the C ABI
def test_header_declares_the_entries_and_the_binding_follows_it():
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, L.SIDE_LIBS["instbox"])) as f:
        protos = L.parse_header(f.read(), {})
    I, V = ctypes.c_int, ctypes.c_void_p
    assert sorted(protos) == NAMES
    assert protos["votenet_instance_boxes_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_instance_boxes_workspace_bytes"] == (ctypes.c_size_t, [I, I])
    assert protos["votenet_instance_boxes"] == (I, [I, ctypes.c_long, I, I, I, I] + [V] * 16 + [ctypes.c_size_t, V])
    assert protos["votenet_instance_point_box"] == (I, [I, ctypes.c_long, I] + [V] * 5)
    lib = L.side_lib("instbox")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == (protos[name][0], protos[name][1])


def test_module_constants_follow_the_header():
    from votenet_amd import instance_boxes as IB
    with open(os.path.join(os.path.dirname(L.__file__), os.pardir, "include", "votenet_instance_boxes.h")) as f:
        text = f.read()
    assert "#define VOTENET_INSTANCE_BOXES_TILE %d\n" % IB.TILE in text and IB.TILE >= 64
    assert IB.MAX_K == 1024 and IB.STATUS == ("kept", "no_class", "few_points", "absent")


def defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in out.splitlines()]


def test_library_exports_exactly_its_header_and_the_others_export_what_they_did(hiplib):
    assert sorted(defined(L.side_path("instbox"))) == NAMES
    for name in L.SIDE_LIBS:
        if name == "instbox":
            continue
        with open(os.path.join(os.path.dirname(L.__file__), os.pardir, "include", L.SIDE_LIBS[name])) as f:
            assert sorted(defined(L.side_path(name))) == sorted(L.parse_header(f.read(), {})), name
    assert not [s for s in defined(L.lib_path()) if "instance_box" in s or "instance_point" in s]


def test_workspace_bytes_is_positive_and_monotone(hiplib):
    ws = L.side_lib("instbox").votenet_instance_boxes_workspace_bytes
    for k in (1, 2, 255, 256, 1024):
        seq = [ws(b, k) for b in (1, 2, 3, 8, 64, 65535)]
        assert seq[0] >= 32 * k and seq == sorted(seq) and seq[0] < seq[-1]
    for b in (1, 8, 65535):
        seq = [ws(b, k) for k in (1, 2, 63, 64, 65, 256, 1023, 1024)]
        assert seq[0] > 0 and seq == sorted(seq) and seq[0] < seq[-1]
        assert ws(b, 1024) >= b * 1024 * 32  # 32 bytes per id and scene
    assert [ws(0, 8), ws(65536, 8), ws(8, 0), ws(8, 1025), ws(-1, -1)] == [0] * 5


def test_every_limit_is_checked_before_any_buffer_or_device_is_touched(hiplib):
    """Status 1 with the text set, every pointer null: the limits come first, then the null checks; nothing reaches the device."""
    lib = L.side_lib("instbox")
    err = lambda: lib.votenet_instance_boxes_last_error().decode()

    def boxes(b=2, n=100, k=16, n_sem=4, n_class=10, min_points=1, ptr=None, ws=None, wsb=1 << 20):
        return lib.votenet_instance_boxes(b, n, k, n_sem, n_class, min_points, *[ptr] * 15, ws, wsb, None)

    def point_box(b=2, n=100, k=16, ptr=None):
        return lib.votenet_instance_point_box(b, n, k, *[ptr] * 4, None)
    limits = ((dict(b=0), "[1, 65535], got 0"), (dict(b=-1), "[1, 65535], got -1"), (dict(b=65536), "[1, 65535], got 65536"),
              (dict(n=0), "[1, 2^24), got n = 0"), (dict(n=-5), "[1, 2^24), got n = -5"), (dict(n=2 ** 24), "[1, 2^24), got n = 16777216"),
              (dict(n=2 ** 40), "[1, 2^24)"), (dict(k=0), "1 to 1024 entries, got k = 0"), (dict(k=1025), "1 to 1024 entries, got k = 1025"),
              (dict(k=INT_MIN), "1 to 1024 entries"))
    for kw, text in limits:
        assert boxes(**kw) == 1 and "instance_boxes: " in err() and text in err(), (kw, err())
        assert point_box(**kw) == 1 and "instance_point_box: " in err() and text in err(), (kw, err())
    for kw, text in ((dict(n_sem=0), "1 to 65536 labels, got n_sem = 0"), (dict(n_sem=65537), "1 to 65536 labels, got n_sem = 65537"),
                     (dict(min_points=0), "min_points must be >= 1, got 0"), (dict(min_points=-3), "min_points must be >= 1, got -3")):
        assert boxes(**kw) == 1 and text in err(), (kw, err())
    # within the limits: the null buffers are refused, still before anything is launched
    assert boxes() == 1 and "null" in err()
    assert point_box() == 1 and "null" in err()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert boxes(ptr=p, ws=None) == 1 and "workspace" in err()
    assert boxes(ptr=p, ws=p, wsb=lib.votenet_instance_boxes_workspace_bytes(2, 16) - 1) == 1 and "workspace of" in err()
    with pytest.raises(L.InvalidArgumentError, match=r"1 to 1024 entries, got k = 1025"):
        L.check(boxes(k=1025), side="instbox")


def test_python_entry_checks_its_arguments_without_a_device():
    import torch
    from votenet_amd import instance_boxes as IB
    z = torch.zeros((1, 4, 3))
    i = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(L.InvalidArgumentError, match="points must be a device tensor"):
        IB.boxes_from_labels(z, i, i, [0])
    with pytest.raises(L.InvalidArgumentError, match="points must be a device tensor"):
        IB.boxes_from_labels(z.numpy(), i, i, [0])
