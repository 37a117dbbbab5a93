"""CPU: proposals sampled on the votes without a device -- the numpy float32 restatement of include/votenet_vote_sampling.h
(tests/vote_sampling_ref.py) against the oracle's composition farthest_point_sample -> gather_point -> query_ball_point on every case
of tests/vote_sampling_cases.py (integers equal, floats equal in bits), each case's own property, and the interface: the header's
entries, the switch of VoteNetHotPath, SAModule.geometry's new argument, the library's argument checks."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_sampling_cases as C  # noqa: E402
import vote_sampling_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402

F = np.float32
NAMES = ["votenet_cluster_votes", "votenet_votesamp_last_error"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


# ------------------------------------------------------------------ the restatement against the oracle's composition
@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_restatement_equals_the_oracles_composition(O, case):
    name, votes, m, radius, k, _ = case
    got = C.results(case)
    fps = O.farthest_point_sample(m, votes)
    centres = O.gather_point(votes, fps)
    idx, cnt = O.query_ball_point(radius, k, votes, centres)
    assert np.array_equal(got["fps_idx"], fps), "fps_idx"
    assert np.array_equal(bits(got["new_xyz"]), bits(centres)), "new_xyz"
    assert np.array_equal(got["idx"], idx), "idx"
    assert np.array_equal(got["pts_cnt"], cnt), "pts_cnt"
    n = votes.shape[1]
    assert got["fps_idx"].min() >= 0 and got["fps_idx"].max() < n and got["idx"].min() >= 0 and got["idx"].max() < n


def test_threshold_is_the_librarys(hiplib):
    for r in (0.3, 0.2, 0.5, 1.2, 1e-3, 1.5, 0.30000001192092896, 7.0, 1e-19):
        want = hiplib.votenet_ball_threshold(ctypes.c_float(F(r)))
        assert R.ball_threshold(r) == F(want), r
    assert R.threshold(0.5) == F(0.25) and R.threshold(1e-21) == F(-1)


# ------------------------------------------------------------------ each case has the property it was built for
def by_kind(kind):
    return [c for c in C.CASES if c[5] == kind]


def test_clustered_balls_overflow_and_fall_short():
    for case in by_kind("clustered"):
        name, votes, m, radius, k, _ = case
        b, n, _ = votes.shape
        r = C.results(case)
        if n >= 1000 or (n >= 63 and k <= 3):
            assert (r["hits"] > k).any(), name                       # a row with more than nsample hits: it is cut at nsample
            assert (r["pts_cnt"][r["hits"] > k] == k).all(), name
        if n >= 256:
            assert ((r["hits"] < k) & (r["hits"] > 0)).any(), name   # and a row with fewer: it is padded with its first hit
        short = r["pts_cnt"] < k
        assert (r["idx"][short][:, -1] == r["idx"][short][:, 0]).all(), name
        if m > n:
            assert (r["fps_idx"][:, n:] == 0).all(), name            # every distance is 0: index 0 repeats
    assert C.results(by_kind("clustered")[1])["fps_idx"].tolist() == [[0, 0, 0, 0]]


def test_lonely_balls_hold_their_centre_only():
    for case in by_kind("lonely"):
        name, votes, m, radius, k, _ = case
        r = C.results(case)
        assert (r["hits"] == 1).all() and (r["pts_cnt"] == 1).all(), name
        assert (r["idx"] == r["fps_idx"][..., None]).all(), name


def test_lattice_rounds_are_exact_ties():
    for case in by_kind("lattice"):
        r = C.results(case)
        assert r["ties"] > 0, case[0]
        print(case[0], "rounds with a tie", r["ties"], "decided against index order", r["against"])


def test_the_mod_512_key_decides_not_the_index():
    case, = by_kind("mod512")
    r = C.results(case)
    f = r["fps_idx"][0].tolist()
    assert f[:5] == [0, 522, 300, 100, 700]  # 522 beats 300 (10 < 300 mod 512) against index order; 100 beats 700 (100 < 188) with it
    assert r["against"] >= 1 and 812 not in f and 612 not in f  # of a duplicate pair only the smaller index is ever sampled


def test_an_all_duplicate_cloud_repeats_index_0():
    for case in by_kind("duplicates"):
        name, votes, m, radius, k, _ = case
        r = C.results(case)
        assert not r["fps_idx"].any() and (r["pts_cnt"] == k).all() and (r["idx"] == np.arange(k)).all(), name
        assert r["ties"] == 0  # (every distance is 0: the all-zero tie is index 0's by rule, not counted)


def test_the_boundary_pair_falls_on_each_side():
    case, = by_kind("boundary")
    name, votes, m, radius, k, _ = case
    T = R.threshold(radius)
    assert T == F(0.25)
    p = votes[0]
    s = lambda a: (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    assert s(p[0] - p[1]) == T and s(p[0] - p[2]) == np.nextafter(T, F(0))
    r = C.results(case)
    assert (r["fps_idx"][:, 0] == 0).all() and r["idx"][:, 0].tolist() == [[0, 2, 0]] * 3 and (r["pts_cnt"][:, 0] == 2).all()


def test_squares_overflow_and_nothing_is_nan():
    for case in by_kind("huge"):
        name, votes, m, radius, k, _ = case
        with np.errstate(over="ignore"):
            assert np.isinf(votes * votes).all() and np.isfinite(votes).all()
        r = C.results(case)
        n = votes.shape[1]
        # every running distance stays at the cap, so the picks follow the tie key alone: 0, 1, 513, 2, 514, ...
        order = np.array(sorted(range(n), key=lambda i: (i % 512, i)), np.int32)[:m]
        assert (r["fps_idx"] == order).all(), name
        assert (r["hits"] == 1).all() and (r["idx"] == r["fps_idx"][..., None]).all(), name


def test_nonfinite_votes_are_never_sampled_and_a_nonfinite_centre_has_no_hit():
    for case in [c for c in C.CASES if c[5].startswith("nonfinite")]:
        name, votes, m, radius, k, kind = case
        r = C.results(case)
        bad = ~np.isfinite(votes).all(axis=2)
        assert bad.any(), name
        for s in range(len(votes)):
            picked = r["fps_idx"][s]
            assert not bad[s][picked[picked > 0]].any(), name         # only index 0 may be a non-finite point
            zero = ~np.isfinite(r["new_xyz"][s]).all(axis=1)          # a non-finite centre: the raw point 0
            assert (r["pts_cnt"][s][zero] == 0).all() and not r["idx"][s][zero].any(), name
            assert (r["pts_cnt"][s][~zero] >= 1).all(), name          # a finite centre hits itself
            assert (zero == (bad[s][picked])).all(), name
        if kind == "nonfinite-point0":
            assert (r["pts_cnt"][:, 0] == 0).all() and not np.isfinite(r["new_xyz"][:, 0]).all(axis=1).any(), name
            assert (r["pts_cnt"][:, 1:] >= 1).all()
        if kind == "nonfinite-scene":
            assert not r["fps_idx"].any() and not r["pts_cnt"].any() and not r["idx"].any(), name
        if kind == "nonfinite-one_scene":
            assert not r["fps_idx"][1].any() and not r["pts_cnt"][1].any() and (r["pts_cnt"][0] >= 1).all(), name
            assert len(set(r["fps_idx"][0].tolist())) > 1


# ------------------------------------------------------------------ the interface
def test_header_declares_the_two_entries_and_the_binding_follows_it(hiplib):
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, L.SIDE_LIBS["votesamp"])) as f:
        protos = L.parse_header(f.read(), {})
    I, V, Fl = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert sorted(protos) == NAMES
    assert protos["votenet_votesamp_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_cluster_votes"] == (I, [I, I, I, Fl, I, V, V, V, V, V, V])
    lib = L.side_lib("votesamp")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == protos[name]


def test_the_mode_is_off_by_default_and_what_the_kernel_refuses_is_refused_at_enable_time():
    from votenet_amd import vote_sampling as VS
    from votenet_amd.model import VoteNetHotPath
    assert VS.MODES == ("seed_fps", "vote_fps")
    assert VS.supported(1024, 256, 64) and VS.supported(1, 1, 1) and VS.supported(2048, 1024, 64)
    assert not VS.supported(2049, 256, 64) and not VS.supported(1024, 1025, 64) and not VS.supported(1024, 256, 65)
    assert not VS.supported(0, 1, 1) and not VS.supported(1, 0, 1) and not VS.supported(1, 1, 0)
    assert VoteNetHotPath.proposal_sampling is None
    net = object.__new__(VoteNetHotPath)  # the switch needs no device

    def shape(n, m, k, knn=False):
        net.sa2 = types.SimpleNamespace(npoint=n)
        net.proposal = types.SimpleNamespace(npoint=m, nsample=k, radius=0.3, knn=knn, group_all=False)
    shape(1024, 256, 64)
    with pytest.raises(L.InvalidArgumentError, match="nonsense"):
        net.enable_proposal_sampling("nonsense")
    assert net.proposal_sampling is None
    net.enable_proposal_sampling()
    assert net.proposal_sampling == "vote_fps" and net.vote_supervision is None and net.proposal_supervision is None
    net.enable_proposal_sampling("seed_fps")
    assert net.proposal_sampling == "seed_fps"
    net.disable_proposal_sampling()
    assert net.proposal_sampling is None
    for bad, text in (((4096, 256, 64), "4096 seeds"), ((1024, 2048, 64), "npoint 2048"), ((1024, 256, 128), "nsample 128")):
        shape(*bad)
        with pytest.raises(L.InvalidArgumentError, match=text):
            net.enable_proposal_sampling("vote_fps")
        assert net.proposal_sampling is None
        net.enable_proposal_sampling("seed_fps")  # the default's name adds no launch and asks nothing of the shape
        net.disable_proposal_sampling()
    shape(1024, 256, 64, knn=True)
    with pytest.raises(L.InvalidArgumentError, match="knn True"):
        net.enable_proposal_sampling("vote_fps")


def test_geometry_takes_the_grouped_argument():
    import inspect
    from votenet_amd.pointnet2 import SAModule
    sig = inspect.signature(SAModule.geometry)
    assert list(sig.parameters)[-1] == "grouped" and sig.parameters["grouped"].default is None
    assert list(inspect.signature(__import__("votenet_amd.model", fromlist=["x"]).VoteNetHotPath.propose).parameters) == \
        ["self", "votes_xyz", "votes_points", "seeds_xyz", "tape", "prop_fps"]  # propose keeps its signature


def test_the_library_checks_its_arguments_before_anything_is_launched(hiplib):
    """Every refused shape and null pointer returns 1 with the limit in the text: no device is needed."""
    lib = L.side_lib("votesamp")
    buf = np.zeros(1 << 12, F)
    p0 = buf.ctypes.data
    err = lambda: lib.votenet_votesamp_last_error().decode()

    def cv(b=2, n=64, m=16, radius=0.3, k=8, votes=p0, fps=p0, xyz=p0, idx=p0, cnt=p0):
        return lib.votenet_cluster_votes(b, n, m, radius, k, votes, fps, xyz, idx, cnt, None)
    for kw, text in ((dict(n=2049), "1 to 2048 votes per scene, got n = 2049"), (dict(n=0), "1 to 2048 votes per scene, got n = 0"),
                     (dict(m=1025), "1 to 1024 clusters per scene, got m = 1025"), (dict(m=0), "1 to 1024 clusters per scene, got m = 0"),
                     (dict(k=65), "1 to 64 votes per cluster, got nsample = 65"), (dict(k=0), "1 to 64 votes per cluster, got nsample = 0"),
                     (dict(radius=0.0), "positive radius"), (dict(radius=-1.0), "positive radius"), (dict(radius=float("nan")), "positive radius"),
                     (dict(b=-1), "b >= 0"), (dict(votes=None), "null"), (dict(fps=None), "null"), (dict(xyz=None), "null"),
                     (dict(idx=None), "null"), (dict(cnt=None), "null"), (dict(b=0, n=4096), "got n = 4096")):
        assert cv(**kw) == 1, kw
        assert text in err(), (kw, err())
    assert cv(b=0) == 0 and cv(b=0, votes=None, fps=None, xyz=None, idx=None, cnt=None) == 0  # no scene: ok, nothing is launched
    with pytest.raises(L.InvalidArgumentError, match=r"1 to 1024 clusters per scene, got m = 1025"):
        L.check(cv(m=1025), side="votesamp")
