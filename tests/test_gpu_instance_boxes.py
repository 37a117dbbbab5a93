"""GPU: ground-truth boxes from instance-labelled points (libvotenet_instbox.so: votenet_instance_boxes, votenet_instance_point_box;
votenet_amd/instance_boxes.py, input_pipeline.build_batch_from_labels) against the numpy restatement of
include/votenet_instance_boxes.h (tests/instance_boxes_ref.py).  Every combination of the rule is exact and the same in any order:
every output is compared by bit pattern (float64 viewed as int64, np.array_equal on the integers)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_boxes_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FLT_MAX = np.finfo(F).max
DENORM = np.array([1, 0x7FFFFF], np.uint32).view(F)  # the smallest and the largest denormal
CLASS_MAP = np.array([3, -1, 0, 9, 10, 7, 2, 12, 5, 1], np.int32)  # n_class = 10: labels 1 (-1), 4 (10) and 7 (12) have no object class
GOOD_SEM = np.array([0, 2, 3, 5, 6, 8, 9], np.int32)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def to_numpy(res):
    return {key: (v.cpu().numpy() if torch.is_tensor(v) else v) for key, v in res.items()}


def run(dev, points, instance, semantic, class_map=CLASS_MAP, **kw):
    from votenet_amd import instance_boxes as IB
    res = IB.boxes_from_labels(T(np.asarray(points, F), dev), T(np.asarray(instance, np.int32), dev), T(np.asarray(semantic, np.int32), dev),
                               T(class_map, dev), want_point_box=True, **kw)
    for key in ("center", "size", "heading", "cls", "instance_id", "n_points", "status", "inst_count", "slot", "ignored", "point_box"):
        assert res[key].is_cuda, key
    assert isinstance(res["box_offset"], np.ndarray) and res["box_offset"].dtype == np.int64
    return to_numpy(res)


def check(dev, points, instance, semantic, class_map=CLASS_MAP, **kw):
    """Run on the device, hold every output to the restatement by bit pattern; -> the (numpy) result."""
    got = run(dev, points, instance, semantic, class_map, **kw)
    exp = R.boxes_from_labels(points, instance, semantic, class_map, **{"k": 256, "n_class": 10, "min_points": 1, **kw})
    assert sorted(got) == sorted(exp)
    assert R.same_bytes(got, exp) == []
    return got


def cloud(rng, b, n):
    return (rng.normal(size=(b, n, 3)) * np.array([3.0, 1.0, 3.0])).astype(F)


def sem_of(instance):
    """A semantic label with an object class, one per id (so every point of an instance agrees)."""
    return GOOD_SEM[np.abs(instance.astype(np.int64)) % len(GOOD_SEM)].astype(np.int32)


# ------------------------------------------------------------------ sizes
def test_one_point(hiplib, dev):
    got = check(dev, np.array([[[1.5, -2.0, 0.25]]], F), [[2]], [[0]], k=4)
    assert got["box_offset"].tolist() == [0, 1] and got["center"].tolist() == [[1.5, -2.0, 0.25]] and got["size"].tolist() == [[0.0] * 3]
    assert got["cls"].tolist() == [3] and got["slot"].tolist() == [[-1, -1, 0, -1]] and got["point_box"].tolist() == [[0]]


def tile_sizes():
    from votenet_amd import instance_boxes as IB
    return [IB.TILE - 1, IB.TILE, IB.TILE + 1, 2 * IB.TILE + 3]


@pytest.mark.parametrize("which", range(4))
def test_tile_tails_with_instances_across_and_inside_tiles(hiplib, dev, which):
    """TILE - 1, TILE, TILE + 1, 2 TILE + 3 points: a last tile that is short, full, one point and three points.  Ids 0 .. 4 take
    stretches of 300 points that cross the tile boundaries (combined through the workspace); id 5 lies inside the first tile only, id 6
    is the last three points (alone in the last tile of 2 TILE + 3), id 7 is absent."""
    from votenet_amd import instance_boxes as IB
    n = tile_sizes()[which]
    rng = np.random.default_rng(n)
    pts = cloud(rng, 2, n)
    inst = np.broadcast_to(((np.arange(n) // 300) % 5)[None], (2, n)).astype(np.int32).copy()
    inst[:, 10:50] = 5
    inst[:, -3:] = 6
    inst[1] = rng.permutation(inst[1])  # the second scene: the same ids, scattered over every tile
    got = check(dev, pts, inst, sem_of(inst), k=8, min_points=2)
    assert got["box_offset"].tolist() == [0, 7, 14] and (got["status"][:, 7] == 3).all() and (got["status"][:, :7] == 0).all()
    assert got["inst_count"].sum() == 2 * n and (got["ignored"] == 0).all()
    assert IB.TILE == 2048


def test_three_scenes_keep_2_0_5_and_an_id_absent_from_one_scene(hiplib, dev):
    """The scene in the middle keeps nothing (its one instance has no object class): scene 2's rows start right behind scene 0's.  Id 3
    is kept in scene 0, absent from scene 1 and present in scene 2."""
    rng = np.random.default_rng(5)
    n = 300
    pts = cloud(rng, 3, n)
    inst = np.full((3, n), -1, np.int32)
    inst[0, :100], inst[0, 100:200] = 3, 9
    inst[1, 50:250] = 6
    for j, i in enumerate((0, 3, 4, 11, 15)):
        inst[2, 40 * j:40 * j + 40] = i
    sem = sem_of(inst)
    sem[1] = 4  # class_map[4] = 10 = n_class: no object class
    got = check(dev, pts, inst, sem, k=16)
    assert got["box_offset"].tolist() == [0, 2, 2, 7] and got["instance_id"].tolist() == [3, 9, 0, 3, 4, 11, 15]
    assert got["status"][:, 3].tolist() == [0, 3, 0] and got["status"][1, 6] == 1 and got["slot"][2, 15] == 4
    assert got["ignored"].tolist() == [[100, 0, 0], [100, 0, 0], [100, 0, 0]]
    assert (got["point_box"][1] == -1).all() and set(got["point_box"][2].tolist()) == {-1, 0, 1, 2, 3, 4}


def test_every_point_its_own_instance(hiplib, dev):
    rng = np.random.default_rng(6)
    pts = cloud(rng, 2, 1024)
    inst = np.stack([rng.permutation(1024), np.arange(1024)]).astype(np.int32)
    got = check(dev, pts, inst, sem_of(inst), k=1024)
    assert got["box_offset"].tolist() == [0, 1024, 2048] and (got["size"] == 0).all() and (got["n_points"] == 1).all()
    assert np.array_equal(got["center"][1024:], pts[1].astype(np.float64))


def test_one_instance_holds_every_point(hiplib, dev):
    """Every lane of every wave hits one LDS address, in three tiles."""
    n = tile_sizes()[3]
    pts = cloud(np.random.default_rng(7), 1, n)
    got = check(dev, pts, np.full((1, n), 2, np.int32), np.full((1, n), 5, np.int32), k=3)
    assert got["n_points"].tolist() == [n] and got["cls"].tolist() == [7]
    assert np.array_equal(got["size"][0], pts[0].max(0).astype(np.float64) - pts[0].min(0).astype(np.float64))


def test_table_of_one_entry_and_the_last_entry_of_the_largest_table(hiplib, dev):
    rng = np.random.default_rng(8)
    pts = cloud(rng, 2, 500)
    inst = rng.integers(-1, 3, (2, 500)).astype(np.int32)  # -1, 0, 1, 2 with k = 1: ids 1 and 2 are out of the table
    got = check(dev, pts, inst, sem_of(inst), k=1)
    assert got["box_offset"].tolist() == [0, 1, 2] and (got["ignored"][:, :2] > 0).all()
    inst = np.where(rng.random((2, 500)) < 0.5, 1023, -1).astype(np.int32)
    got = check(dev, pts, inst, sem_of(inst), k=1024)
    assert got["box_offset"].tolist() == [0, 1, 2] and got["instance_id"].tolist() == [1023, 1023] and (got["slot"][:, 1023] == 0).all()
    assert (got["status"][:, :1023] == 3).all()


# ------------------------------------------------------------------ labels and coordinates
def test_label_values_at_the_table_s_edges_and_the_int_limits_index_nothing(hiplib, dev):
    k, n = 16, 700
    rng = np.random.default_rng(9)
    pts = cloud(rng, 2, n)
    inst = rng.choice(np.array([-1, k - 1, k, INT_MIN, INT_MAX, 0, k + 1, -2, 2 ** 24, 2 ** 30], np.int64), (2, n)).astype(np.int32)
    sem = rng.choice(np.array([0, 2, INT_MIN, INT_MAX, -1, 10], np.int64), (2, n)).astype(np.int32)
    pts[0, ::7] = np.nan  # non-finite points under every kind of id: counted by the first test that holds
    got = check(dev, pts, inst, sem, k=k)
    exp_ign = [[int((inst[s] < 0).sum()), int((inst[s] >= k).sum()),
                int(((inst[s] >= 0) & (inst[s] < k) & ~np.isfinite(pts[s]).all(1)).sum())] for s in range(2)]
    assert got["ignored"].tolist() == exp_ign and all(v > 0 for v in exp_ign[0]) and exp_ign[1][2] == 0
    assert got["ignored"].sum() + got["inst_count"].sum() == 2 * n
    assert (got["status"][:, 1:k - 1] == 3).all() and (got["inst_count"][:, [0, k - 1]] > 0).all()


def test_signs_zeros_denormals_and_flt_max(hiplib, dev):
    """-0.0 takes part as +0.0 (a box of -0.0 points alone has centre and size +0.0, bit for bit); denormals are kept, not flushed;
    +-FLT_MAX in one instance: the size 2 FLT_MAX is finite in float64."""
    special = np.array([0.0, -0.0, DENORM[0], -DENORM[0], DENORM[1], -DENORM[1], np.finfo(F).tiny, FLT_MAX, -FLT_MAX, 1.0, -1.0, 1e-30, -3e38], F)
    rng = np.random.default_rng(10)
    n = 600
    pts = rng.choice(special, (1, n, 3)).astype(F)
    inst = rng.integers(0, 12, (1, n)).astype(np.int32)
    pts[0, inst[0] == 3] = -0.0                                      # only -0.0
    pts[0, inst[0] == 4] = rng.choice(DENORM, (int((inst[0] == 4).sum()), 3)) * F(-1)  # only negative denormals
    pts[0, inst[0] == 5] = rng.choice(np.array([-0.0, -DENORM[0]], F), (int((inst[0] == 5).sum()), 3))  # max is -0 -> +0
    got = check(dev, pts, inst, sem_of(inst), k=12)
    row = got["slot"][0]
    assert got["box_offset"].tolist() == [0, 12]
    assert (R.bits(got["center"][row[3]]) == 0).all() and (R.bits(got["size"][row[3]]) == 0).all()  # +0.0, bit for bit
    assert (got["center"][row[4]] < 0).all() and (np.abs(got["center"][row[4]]) < 1.2e-38).all()
    assert got["size"].max() == 2.0 * float(FLT_MAX) and np.isfinite(got["size"]).all()


def test_non_finite_points_are_ignored_and_leave_the_box_unchanged(hiplib, dev):
    rng = np.random.default_rng(11)
    n = 900
    pts = cloud(rng, 1, n)
    inst = rng.integers(0, 6, (1, n)).astype(np.int32)
    sem = sem_of(inst)
    clean = check(dev, pts, inst, sem, k=8)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.inf, -np.inf], [1e30, np.nan, -1e30]], F)
    extra_inst = np.repeat(np.arange(6), 5).astype(np.int32)
    pts2 = np.concatenate([np.tile(bad, (6, 1))[None], pts], 1)  # the non-finite points come FIRST: they do not become `first` either
    inst2 = np.concatenate([extra_inst[None], inst], 1)
    sem2 = np.concatenate([np.full((1, 30), 1, np.int32), sem], 1)  # their label has no object class: it must not decide
    inst2 = np.concatenate([inst2, np.full((1, 40), 7, np.int32)], 1)  # id 7: every point non-finite -> absent
    pts2 = np.concatenate([pts2, np.tile(bad, (8, 1))[None]], 1)
    sem2 = np.concatenate([sem2, np.zeros((1, 40), np.int32)], 1)
    got = check(dev, pts2, inst2, sem2, k=8)
    assert R.same_bytes(got, clean, ("center", "size", "heading", "cls", "instance_id", "n_points", "box_offset", "inst_count")) == []
    assert got["ignored"].tolist() == [[0, 0, 70]] and got["status"][0].tolist() == [0] * 6 + [3, 3] and got["inst_count"][0, 7] == 0
    assert (got["point_box"][0, :30] == -1).all() and (got["point_box"][0, -40:] == -1).all()


def test_the_lowest_index_point_s_label_decides_and_labels_without_a_class(hiplib, dev):
    """Ids 0 .. 2: points disagree, the first has / has not an object class.  Ids 3 .. 8: semantic below 0, at n_sem, INT_MIN, INT_MAX,
    class_map -1, class_map >= n_class: status 1 each."""
    rng = np.random.default_rng(12)
    per = 50
    inst = np.repeat(np.arange(9), per)[None].astype(np.int32)
    n = inst.shape[1]
    sem = np.zeros((1, n), np.int32)
    sem[0, 0 * per:1 * per] = 1      # id 0: all but the first have no class ...
    sem[0, 0] = 6                    # ... the first has class 2
    sem[0, 1 * per:2 * per] = 6      # id 1: the other way round
    sem[0, per] = 1
    sem[0, 2 * per:3 * per] = rng.choice(GOOD_SEM, per)  # id 2: classes disagree
    for i, v in zip(range(3, 9), (-1, len(CLASS_MAP), INT_MIN, INT_MAX, 1, 7)):
        sem[0, i * per:(i + 1) * per] = v
    perm = np.concatenate([[0, per, 2 * per], rng.permutation(np.setdiff1d(np.arange(n), [0, per, 2 * per]))])  # firsts stay first
    inst, sem = inst[:, perm], sem[:, perm]
    got = check(dev, cloud(rng, 1, n), inst, sem, k=9)
    assert got["status"][0].tolist() == [0, 1, 0, 1, 1, 1, 1, 1, 1]
    assert got["cls"].tolist() == [2, int(CLASS_MAP[sem[0, 2]])] and got["instance_id"].tolist() == [0, 2]
    assert check(dev, cloud(rng, 1, n), inst, sem, k=9, n_class=2)["status"][0, 0] == 1  # class 2 with n_class = 2


@pytest.mark.parametrize("min_points", [1, 5])
def test_min_points_threshold(hiplib, dev, min_points):
    """count = min_points - 1 (for min_points = 1: no point, absent) and count = min_points, in two tiles each."""
    from votenet_amd import instance_boxes as IB
    n = IB.TILE + 40
    rng = np.random.default_rng(13)
    inst = np.full((1, n), -1, np.int32)
    inst[0, 100:100 + min_points - 1] = 0
    at = [n - 1] + ([5] if min_points > 1 else []) + [300 + j for j in range(min_points - 2)]  # the first and the second tile
    inst[0, at] = 1
    got = check(dev, cloud(rng, 1, n), inst, sem_of(inst), k=2, min_points=min_points)
    assert got["inst_count"].tolist() == [[min_points - 1, min_points]]
    assert got["status"].tolist() == [[3 if min_points == 1 else 2, 0]] and got["n_points"].tolist() == [min_points]


def test_all_points_unlabelled(hiplib, dev):
    from votenet_amd import input_pipeline as IP
    rng = np.random.default_rng(14)
    n = 400
    pts = cloud(rng, 2, n)
    inst = np.full((2, n), -1, np.int32)
    got = check(dev, pts, inst, np.zeros((2, n), np.int32), k=4)
    assert got["box_offset"].tolist() == [0, 0, 0] and got["center"].shape == (0, 3) and got["cls"].shape == (0,)
    assert got["ignored"].tolist() == [[n, 0, 0]] * 2 and (got["status"] == 3).all() and (got["point_box"] == -1).all()
    raw, off = IP.pack_ragged([pts[0].astype(np.float64), pts[1].astype(np.float64)], dev)
    choice = np.stack([rng.permutation(n)[:64] for _ in range(2)]).astype(np.int32)
    points, gt, scene_index = IP.build_batch_from_labels(raw, off, inst.ravel(), np.zeros(2 * n, np.int32), CLASS_MAP, choice, n_out=64)
    assert points is None and gt is None and scene_index.dtype == np.int64 and scene_index.shape == (0,)


# ------------------------------------------------------------------ consistency
def mixed(seed, b=3, n=5000, k=40):
    """Everything at once: instances of very different sizes, unlabelled and out-of-table ids, holes, labels without a class."""
    rng = np.random.default_rng(seed)
    pts = cloud(rng, b, n)
    pts[rng.random((b, n)) < 0.01] = np.nan
    inst = np.minimum(rng.geometric(0.15, (b, n)) - 3, k + 2).astype(np.int32)
    sem = np.broadcast_to(np.arange(-2, k + 3)[None] % 11 - 1, (b, k + 5))
    sem = np.take_along_axis(sem, np.clip(inst, -2, k + 2) + 2, 1).astype(np.int32)
    return pts, inst, sem


def test_point_box_names_the_row_of_each_kept_instance(hiplib, dev):
    pts, inst, sem = mixed(20)
    got = check(dev, pts, inst, sem, k=40, min_points=4)
    pb = got["point_box"]
    part, _ = R.takes_part(pts, inst, 40)
    status_of_point = np.where(part, np.take_along_axis(got["status"], np.clip(inst, 0, 39), 1), -1)
    assert np.array_equal(pb >= 0, status_of_point == 0) and (pb >= 0).any() and (pb < 0).any()
    assert {1, 2, 3}.issubset(set(got["status"].ravel().tolist()))
    for s in range(3):  # ... and it names that instance's row
        rows = got["box_offset"][s] + pb[s][pb[s] >= 0]
        assert np.array_equal(got["instance_id"][rows], inst[s][pb[s] >= 0])


def test_two_calls_and_a_side_stream_write_the_same_bytes(hiplib, dev):
    pts, inst, sem = mixed(21)
    first = run(dev, pts, inst, sem, k=40, min_points=4)
    second = run(dev, pts, inst, sem, k=40, min_points=4)
    assert R.same_bytes(second, first) == [] and first["box_offset"][-1] > 10
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        third = run(dev, pts, inst, sem, k=40, min_points=4)
    side.synchronize()
    assert R.same_bytes(third, first) == []


class RawCall:
    """The two C entries on buffers of the caller: the workspace filled with garbage, every output between the words it was filled with."""
    GARBAGE = 0x5A5A5A5A

    def __init__(self, dev, pts, inst, sem, k, min_points):
        from votenet_amd import _lib as L
        self.L, self.lib = L, L.side_lib("instbox")
        self.b, self.n, self.k, self.min_points = inst.shape[0], inst.shape[1], k, min_points
        b, n = self.b, self.n
        self.inputs = [T(pts, dev), T(inst, dev), T(sem, dev), T(CLASS_MAP, dev)]
        filled = lambda words: torch.full((words,), self.GARBAGE, dtype=torch.int32, device=dev)
        self.words = {"center": 6 * b * k, "size": 6 * b * k, "heading": 2 * b * k, "cls": b * k, "instance_id": b * k, "n_points": b * k,
                      "kept": b, "slot": b * k, "status": b * k, "inst_count": b * k, "ignored": 3 * b, "point_box": b * n}
        self.out = {key: filled(w) for key, w in self.words.items()}
        self.wsb = int(self.lib.votenet_instance_boxes_workspace_bytes(b, k))
        self.ws = torch.full((self.wsb,), 0xA5, dtype=torch.uint8, device=dev)

    def launch(self):
        L, o = self.L, self.out
        L.check(self.lib.votenet_instance_boxes(self.b, self.n, self.k, len(CLASS_MAP), 10, self.min_points, *[L.ptr(t) for t in self.inputs],
                                                *[L.ptr(o[key]) for key in list(self.words)[:11]], L.ptr(self.ws), self.wsb, L.stream_ptr()),
                side="instbox")
        L.check(self.lib.votenet_instance_point_box(self.b, self.n, self.k, L.ptr(self.inputs[0]), L.ptr(self.inputs[1]), L.ptr(o["slot"]),
                                                    L.ptr(o["point_box"]), L.stream_ptr()), side="instbox")

    def result(self):
        """-> (dict laid out as boxes_from_labels', the words of the row outputs beyond the kept rows)."""
        o = {key: v.cpu().numpy() for key, v in self.out.items()}
        b, k = self.b, self.k
        off = np.concatenate([[0], np.cumsum(o["kept"])]).astype(np.int64)
        nk = int(off[-1])
        res = {"center": o["center"].view(np.float64).reshape(b * k, 3)[:nk], "size": o["size"].view(np.float64).reshape(b * k, 3)[:nk],
               "heading": o["heading"].view(np.float64)[:nk], "box_offset": off, "point_box": o["point_box"].reshape(b, self.n),
               "ignored": o["ignored"].reshape(b, 3)}
        res.update({key: o[key][:nk] for key in ("cls", "instance_id", "n_points")})
        res.update({key: o[key].reshape(b, k) for key in ("slot", "status", "inst_count")})
        beyond = np.concatenate([o["center"][6 * nk:], o["size"][6 * nk:], o["heading"][2 * nk:], o["cls"][nk:], o["instance_id"][nk:],
                                 o["n_points"][nk:]])
        return res, beyond


def test_garbage_in_the_workspace_does_not_matter_and_no_row_beyond_the_kept_is_written(hiplib, dev):
    pts, inst, sem = mixed(24)
    call = RawCall(dev, pts, inst, sem, 40, 4)
    call.launch()
    torch.cuda.synchronize()
    got, beyond = call.result()
    exp = R.boxes_from_labels(pts, inst, sem, CLASS_MAP, k=40, n_class=10, min_points=4)
    assert R.same_bytes(got, exp) == [] and 10 < exp["box_offset"][-1] < 3 * 40
    assert len(beyond) > 0 and (beyond == RawCall.GARBAGE).all()
    call.ws.fill_(0xFF)  # ... nor does what the call itself left there
    call.launch()
    torch.cuda.synchronize()
    assert R.same_bytes(call.result()[0], exp) == []


def test_both_entries_replay_from_a_captured_graph(hiplib, dev):
    """Nothing allocates, synchronises or is read back: the four launches are captured once and replayed on new labels."""
    pts, inst, sem = mixed(25)
    call = RawCall(dev, pts, inst, sem, 40, 4)
    call.launch()  # (loads the code object before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.launch()
    pts2, inst2, sem2 = mixed(26)
    for t, a in zip(call.inputs, (pts2, inst2, sem2)):
        t.copy_(T(a, dev))
    for v in call.out.values():
        v.fill_(RawCall.GARBAGE)
    graph.replay()
    torch.cuda.synchronize()
    exp = R.boxes_from_labels(pts2, inst2, sem2, CLASS_MAP, k=40, n_class=10, min_points=4)
    assert R.same_bytes(call.result()[0], exp) == []
    assert R.same_bytes(exp, R.boxes_from_labels(pts, inst, sem, CLASS_MAP, k=40, n_class=10, min_points=4)) != []


def test_argument_checks_on_the_device(hiplib, dev):
    from votenet_amd import _lib as L
    from votenet_amd import instance_boxes as IB
    p, i = torch.zeros((2, 8, 3), device=dev), torch.zeros((2, 8), dtype=torch.int32, device=dev)
    cm = T(CLASS_MAP, dev)
    for args, kw, text in (((p.double(), i, i, cm), {}, "points must be float32"), ((p[:, :, :2], i, i, cm), {}, r"shape \(b, n, 3\)"),
                           ((p.transpose(0, 1), i, i, cm), {}, "shape|contiguous"), ((p[:, ::2], i[:, ::2], i[:, ::2], cm), {}, "points must be contiguous"),
                           ((p, i.long(), i, cm), {}, "instance must be int32"), ((p, i, i[:, :4], cm), {}, "semantic must have shape"),
                           ((p, i.cpu(), i, cm), {}, "instance must be a tensor on points' device"), ((p, i, i, cm.reshape(2, 5)), {}, "class_map must hold"),
                           ((p, i, i, np.zeros(3)), {}, "1-D integer array"), ((p, i, i, cm), {"k": 0}, r"k must be in \[1, 1024\], got 0"),
                           ((p, i, i, cm), {"k": 1025}, r"k must be in \[1, 1024\], got 1025"), ((p, i, i, cm), {"min_points": 0}, "min_points must be >= 1"),
                           ((p, i, i, cm), {"k": 2.5}, "k must be an integer"), ((p[:0], i[:0], i[:0], cm), {}, "1 <= b"),
                           ((p, i.t().contiguous().t(), i, cm), {}, "instance must be contiguous")):
        with pytest.raises(L.InvalidArgumentError, match=text):
            IB.boxes_from_labels(*args, **kw)
    assert IB.boxes_from_labels(p, i, i, CLASS_MAP.tolist())["box_offset"].tolist() == [0, 1, 2]  # a host class_map is taken


# ------------------------------------------------------------------ the hand-over
def test_augment_boxes_takes_the_result(hiplib, dev):
    from votenet_amd import input_pipeline as IP
    from votenet_amd import instance_boxes as IB
    pts, inst, sem = mixed(22)
    res = IB.boxes_from_labels(T(pts, dev), T(inst, dev), T(sem, dev), T(CLASS_MAP, dev), k=40, min_points=4)
    off = res["box_offset"]
    cnt = np.diff(off)
    assert (cnt > 0).all() and len(set(cnt.tolist())) > 1  # ragged: the padding repeats a scene's last box
    gt = to_numpy(IP.augment_boxes(**{key: res[key] for key in ("center", "size", "heading", "cls", "box_offset")}, aug=None))
    center, size, cls = res["center"].cpu().numpy(), res["size"].cpu().numpy(), res["cls"].cpu().numpy()
    for s in range(3):
        rows = off[s] + np.minimum(np.arange(cnt.max()), cnt[s] - 1)
        assert np.array_equal(gt["bboxes_xyz"][s].view(np.int32), center[rows].astype(F).view(np.int32))
        assert np.array_equal(gt["bboxes_lwh"][s].view(np.int32), size[rows].astype(F).view(np.int32))
        assert np.array_equal(gt["semantic_labels"][s], cls[rows]) and np.array_equal(gt["size_labels"][s], cls[rows])
    assert (gt["bboxes_roty"].view(np.int32) == 0).all() and (gt["heading_labels"] == 0).all() and (gt["heading_residuals"] == 0).all()


def test_build_batch_from_labels_on_three_ragged_scenes(hiplib, dev):
    """An Augmentation and a host choice.  The points are subsample_augment's bit for bit; the gt is what the restatement forms from
    THOSE points and the labels gathered by choice; the scene whose labels have no object class is absent from scene_index."""
    from votenet_amd import input_pipeline as IP
    rng = np.random.default_rng(23)
    n_raw, n_out, k = (3000, 1700, 2400), 1024, 24
    scenes = [np.concatenate([rng.normal(size=(n, 3)) * [2.0, 2.0, 0.7] + [0, 3, 0], rng.random((n, 3))], 1) for n in n_raw]
    inst = [rng.integers(-1, k + 2, n).astype(np.int32) for n in n_raw]
    sem = [sem_of(i) for i in inst]
    sem[1][:] = 1  # scene 1: no label has an object class
    raw, off = IP.pack_ragged(scenes, dev)
    aug = IP.Augmentation([True, False, True], [False, True, True], [0.05, -0.08, 0.02], [1.05, 0.93, 1.0])
    choice = IP.draw_choice(np.random.RandomState(3), n_raw, n_out)
    inst_cat, sem_cat = np.concatenate(inst), np.concatenate(sem)
    points, gt, scene_index = IP.build_batch_from_labels(raw, off, inst_cat, T(sem_cat, dev), CLASS_MAP, choice, aug, n_out=n_out, k=k,
                                                         min_points=3)
    assert scene_index.tolist() == [0, 2]
    exp_points = IP.subsample_augment(raw, off, n_out, aug, choice)
    assert torch.equal(points.view(torch.int32), exp_points[[0, 2]].view(torch.int32))
    g_inst = np.stack([inst[s][choice[s]] for s in range(3)])
    g_sem = np.stack([sem[s][choice[s]] for s in range(3)])
    ref = R.boxes_from_labels(exp_points.cpu().numpy(), g_inst, g_sem, CLASS_MAP, k=k, n_class=10, min_points=3)
    cnt = np.diff(ref["box_offset"])
    assert cnt[1] == 0 and cnt[0] > 5 and cnt[2] > 5
    exp_gt = to_numpy(IP.augment_boxes(*[T(ref[key], dev) for key in ("center", "size", "heading", "cls")],
                                       np.concatenate([[0], np.cumsum(cnt[[0, 2]])]), None))
    got_gt = to_numpy(gt)
    assert sorted(got_gt) == sorted(exp_gt) == sorted(name for name, _, _ in IP.GT_FIELDS)
    for key in exp_gt:
        assert got_gt[key].dtype == exp_gt[key].dtype and np.array_equal(got_gt[key].view(np.int32), exp_gt[key].view(np.int32)), key
    assert np.array_equal(got_gt["bboxes_xyz"][0, :cnt[0]].view(np.int32), ref["center"][:cnt[0]].astype(F).view(np.int32))
    assert np.array_equal(got_gt["bboxes_lwh"][1, :cnt[2]].view(np.int32), ref["size"][cnt[0]:].astype(F).view(np.int32))
    # with features: the same points and boxes, the features of subsample_augment_features
    points_f, gt_f, idx_f = IP.build_batch_from_labels(raw, off, T(inst_cat, dev), sem_cat, T(CLASS_MAP, dev), T(choice, dev), aug,
                                                       n_out=n_out, k=k, min_points=3, height=True, extra_cols=3)
    assert idx_f.tolist() == [0, 2] and torch.equal(points_f.view(torch.int32), points.view(torch.int32))
    assert tuple(gt_f["features"].shape) == (2, n_out, 4)
    for key in exp_gt:
        assert torch.equal(gt_f[key], gt[key]), key


# ------------------------------------------------------------------ the library is loaded on request only
FRESH = """
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
import votenet_amd
from votenet_amd import _lib, input_pipeline as IP, sunrgbd
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
n = 4096
scene = np.concatenate([rng.random((n, 3)) * [2.0, 2.0, 1.0] + [-1.0, 1.0, -0.5], rng.random((n, 3))], 1)
raw, off = IP.pack_ragged([scene], dev)
Rt, K = np.eye(3), np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
objects = sunrgbd.pack_objects([{"cls": np.array([3], np.int32), "box2d": np.array([[-1e9, -1e9, 1e9, 1e9]]), "centroid": np.array([[0.0, 2.0, 0.0]]),
                                 "half_extent": np.array([[5.0, 5.0, 5.0]]), "heading": np.array([0.0])}])
choice = IP.draw_choice(np.random.RandomState(0), [n], 1024)
IP.build_batch(raw, off, [(Rt, K)], objects, IP.draw_augmentation(1, np.random.RandomState(1)), choice, n_out=1024)
torch.cuda.synchronize()
maps = open("/proc/self/maps").read()
assert "libvotenet_hip.so" in maps
assert not _lib.side_loaded("instbox") and "libvotenet_instbox" not in maps and "votenet_amd.instance_boxes" not in sys.modules
before = {name for name in _lib.SIDE_LIBS if _lib.side_loaded(name)}
from votenet_amd import instance_boxes as IB
assert not _lib.side_loaded("instbox") and "libvotenet_instbox" not in open("/proc/self/maps").read()
pts = IP.subsample_augment(raw, off, 1024, None, choice)
lab = torch.zeros((1, 1024), dtype=torch.int32, device=dev)
res = IB.boxes_from_labels(pts, lab, lab, [0])
assert res["box_offset"].tolist() == [0, 1]
assert _lib.side_loaded("instbox") and "libvotenet_instbox.so" in open("/proc/self/maps").read()
assert {name for name in _lib.SIDE_LIBS if _lib.side_loaded(name)} == before | {"instbox"}
print("fresh ok")
"""


def test_a_fresh_process_loads_the_library_with_the_first_call_only(hiplib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", FRESH % root], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fresh ok" in out.stdout, out.stdout + out.stderr
