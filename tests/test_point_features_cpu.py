"""CPU: the point-feature path without a device -- the numpy restatement of the floor (tests/point_features_ref.py) against
np.percentile, the C ABI entry in the header and its derived binding, and the model's sa1 width / checkpoint shape."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_features_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402
from votenet_amd import model as VM  # noqa: E402

CPU = torch.device("cpu")
SMALL = (64, 32, 16, 8)


def _clouds():
    rng = np.random.default_rng(11)
    out = [("random %d" % n, (rng.normal(size=n) * 1.5 - 0.4).astype(np.float32)) for n in (300, 1000, 5000, 20480)]
    flat = (rng.random(4000) * 2.5 - 1.2).astype(np.float32)
    flat[rng.permutation(4000)[:1200]] = np.float32(-1.2034)  # 30 % of the points on one plane: many equal values around the rank
    out.append(("flat floor", flat))
    for m in (1, 2, 102):  # m = 102: k = 0.9999, t just under 1
        out.append(("m = %d" % m, (rng.normal(size=m) * 2).astype(np.float32)))
    return out


@pytest.mark.parametrize("name,up", _clouds(), ids=[c[0] for c in _clouds()])
def test_floor_restatement_is_np_percentile(name, up):
    want = np.percentile(up.astype(np.float64), 0.99)
    got, a, b, m = R.floor_ref(up)
    assert m == len(up) and a <= b
    assert got.dtype == np.float32
    assert abs(float(got) - want) <= R.ulp32(want), (name, float(got), want)


def test_floor_restatement_leaves_non_finite_values_out():
    up = np.array([0.5, np.nan, -1.0, np.inf, 2.0, -np.inf, 0.25], np.float32)
    got, a, b, m = R.floor_ref(up)
    assert m == 4 and a == np.float32(-1.0) and b == np.float32(0.25)
    assert abs(float(got) - np.percentile(np.array([0.5, -1.0, 2.0, 0.25], np.float64), 0.99)) <= R.ulp32(got)
    pts = np.zeros((7, 3), np.float32)
    pts[:, 1] = -up
    h = R.heights_ref(pts)
    assert (h[[1, 3, 5]] == 0).all() and h[2] == np.float32(-1.0) - got
    assert R.floor_ref(np.array([np.nan, np.inf], np.float32)) == (0.0, 0.0, 0.0, 0)


def test_header_declares_the_entry_and_the_binding_follows_it():
    """include/votenet_point_features.h is the one statement of the entry: the ctypes prototype is read from it (parse_header), and it
    is votenet_subsample_augment's argument list up to the output, then want_height, extra_cols and the five pointers."""
    import ctypes
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, "votenet_point_features.h")) as f:
        protos = L.parse_header(f.read(), {})
    assert sorted(protos) == ["votenet_point_features_last_error", "votenet_subsample_augment_features"]
    ret, args = protos["votenet_subsample_augment_features"]
    base = L._abi()[0]["votenet_subsample_augment"][1]
    assert ret is ctypes.c_int and len(args) == 21
    assert args[:len(base) - 2] == base[:-2]
    assert args[len(base) - 2:] == [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5


def test_library_exports_exactly_its_header_and_binds_it(hiplib):
    import ctypes
    import subprocess
    F = L.side_lib("features")
    fn = F.votenet_subsample_augment_features
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 21
    assert F.votenet_point_features_last_error.restype is ctypes.c_char_p
    out = subprocess.run(["nm", "-D", "--defined-only", L.side_path("features")], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines()) == ["votenet_point_features_last_error", "votenet_subsample_augment_features"]
    # the argument checks need no device: every invalid-argument case returns 1 with a message before anything is launched
    import numpy as np
    off = np.array([0, 10], np.int64)
    P = lambda a: a.ctypes.data
    dummy = 4096  # (never dereferenced: the checks come first)

    def call(b=1, n_out=4, raw=dummy, stride=6, offp=None, want_height=1, extra=3, out=dummy, feats=dummy, floor=dummy):
        return fn(b, n_out, raw, 0, stride, P(off) if offp is None else offp, None, 0, 0, 1, None, None, None, None, want_height, extra, out, feats,
                  floor, None, None)
    for kw, text in ((dict(want_height=0, extra=0), "no feature"), (dict(extra=5), "extra_cols"), (dict(extra=-1), "extra_cols"),
                     (dict(want_height=2), "want_height"), (dict(stride=5), "raw_stride"), (dict(feats=None), "feats"),
                     (dict(floor=None), "floor"), (dict(out=None), "null"), (dict(raw=None), "null"), (dict(n_out=11), "without replacement"),
                     (dict(b=0), "positive")):
        assert call(**kw) == 1, kw
        assert text in F.votenet_point_features_last_error().decode(), (kw, F.votenet_point_features_last_error())


def test_point_features_widen_sa1_and_nothing_else():
    net = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL, point_features=4)
    base = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL)
    assert net.point_features == 4 and base.point_features == 0
    assert tuple(net.store.views["sa1/conv0/W"].shape) == (7, 64) and tuple(base.store.views["sa1/conv0/W"].shape) == (6, 64)
    assert net.sa1.leaf and net.sa1.cin == 4 and base.sa1.cin == 3
    for name, v in base.store.views.items():
        if name != "sa1/conv0/W":
            assert tuple(net.store.views[name].shape) == tuple(v.shape), name
    assert set(net.store.views) == set(base.store.views)
    sd = net.state_dict()
    assert sd["sa1/conv0/W"].shape == (1, 1, 7, 64) and sd["sa1/conv0/W/Adam"].shape == (1, 1, 7, 64)


def test_state_dict_round_trips_with_point_features(tmp_path):
    net = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL, point_features=4)
    net.init_optimizer(2e-3)
    net._m.normal_()
    net._v.uniform_()
    net._step = 7
    other = VM.VoteNetHotPath(CPU, seed=9, npoints=SMALL, point_features=4)
    assert not torch.equal(other.store.flat, net.store.flat)
    other.load_state_dict(net.state_dict())
    a, b = net.state_dict(), other.state_dict()  # (the buckets' alignment padding is no part of the state)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert torch.equal(other.store.views["sa1/conv0/W"], net.store.views["sa1/conv0/W"]) and float(a["sa1/conv0/W/Adam"].std()) > 0
    assert other._step == 7 and other._lr == 2e-3
    path = tmp_path / "pf.npz"
    net.save(path)
    third = VM.VoteNetHotPath(CPU, seed=5, npoints=SMALL, point_features=4)
    third.load(path)
    assert torch.equal(third.store.flat, net.store.flat)
    a, b = net.state_dict(), third.state_dict()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("have,want", [(4, 0), (0, 4), (1, 4)])
def test_a_checkpoint_of_another_sa1_width_is_refused_naming_both(tmp_path, have, want):
    src = VM.VoteNetHotPath(CPU, seed=3, npoints=SMALL, point_features=have)
    dst = VM.VoteNetHotPath(CPU, seed=4, npoints=SMALL, point_features=want)
    before = dst.store.flat.clone()
    rows = lambda c: 3 + (c if c else 3)
    with pytest.raises(ValueError, match=r"sa1/conv0/W.*%d input rows.*%d" % (rows(have), rows(want))):
        dst.load_state_dict(src.state_dict())
    path = tmp_path / "w.npz"
    src.save(path)
    with pytest.raises(ValueError, match=r"%d input rows.*%d" % (rows(have), rows(want))):
        dst.load(path)
    assert torch.equal(dst.store.flat, before)  # nothing was written


def test_more_than_five_point_features_are_refused():
    for c in (6, 9, -1):
        with pytest.raises(L.InvalidArgumentError, match="point_features"):
            VM.VoteNetHotPath(CPU, npoints=SMALL, point_features=c)


def test_feats_are_checked_before_anything_runs():
    net = VM.VoteNetHotPath(CPU, npoints=SMALL, point_features=2)
    base = VM.VoteNetHotPath(CPU, npoints=SMALL)
    x = torch.zeros(2, 128, 3)
    with pytest.raises(L.InvalidArgumentError, match="point_features=2"):
        net.forward(x)
    with pytest.raises(L.InvalidArgumentError, match="point_features=2"):
        net.predict(x)
    with pytest.raises(L.InvalidArgumentError, match="point_features=2"):
        net.train_step(x)
    for bad in (torch.zeros(2, 128, 3), torch.zeros(2, 100, 2), torch.zeros(2, 128, 2, dtype=torch.float64), torch.zeros(2, 128, 4)[..., :2]):
        with pytest.raises(L.InvalidArgumentError, match="feats"):
            net.forward(x, feats=bad)
    with pytest.raises(L.InvalidArgumentError, match="without point features"):
        base.forward(x, feats=torch.zeros(2, 128, 2))
    with pytest.raises(L.InvalidArgumentError, match="without point features"):
        base.train_step(x, feats=torch.zeros(2, 128, 2))
    with pytest.raises(L.InvalidArgumentError, match="next_feats"):
        VM.VoteNetHotPath._pair_next([x, x], [torch.zeros(2, 128, 2)])


def test_prefetched_geometry_is_trusted_only_for_the_same_feature_tensor():
    net = VM.GeometryPrefetch(chain=lambda *a: None, side_stream=lambda: None, device=CPU, prop_npoint=256)
    x, f = torch.zeros(2, 8, 3), torch.zeros(2, 8, 2)

    def entry():
        net.pool[id(x)] = VM.PrefetchEntry(x, x._version, {"sa1": 1}, {"sa1": 2}, None, 0, f, f._version)
    entry()
    assert net.take(x, f) == ({"sa1": 1}, {"sa1": 2})
    entry()
    assert net.take(x, f.clone()) is None  # another tensor
    entry()
    assert net.take(x, None) is None
    entry()
    f.add_(1)  # changed in place after the prefetch
    assert net.take(x, f) is None
