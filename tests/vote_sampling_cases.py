"""The case table of the vote-sampling tests (tests/test_vote_sampling_cpu.py, tests/test_gpu_vote_sampling.py): every shape at which
votenet_cluster_votes takes another path, and the clouds that reach every rule of include/votenet_vote_sampling.h.  A case is
(name, votes (b,n,3) float32, m, radius, nsample, kind); the references' results are computed once per case and shared (results())."""
import numpy as np

import vote_sampling_ref as R

F = np.float32
# (b, n, m, nsample): the smallest shape; m > n; round the wave boundary; the suite's small net (m == n); the first index whose k mod 512
# wraps; n no multiple of 64; the training shape; both limits
SHAPES = [(1, 1, 1, 1), (1, 1, 4, 3), (3, 63, 16, 3), (1, 64, 64, 64), (1, 65, 8, 1), (2, 256, 256, 64), (1, 513, 32, 64),
          (3, 1000, 256, 64), (8, 1024, 256, 64), (1, 2048, 1024, 64)]
RADIUS = 0.3  # the proposal module's


def clustered(seed, b, n):
    """Votes piled up about a few centres (sigma 0.1 against the radius 0.3): the balls overflow nsample as soon as n allows."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-2, 2, (b, 5, 3))
    pick = rng.integers(0, 5, (b, n))
    return (np.take_along_axis(centres, pick[..., None].repeat(3, -1), 1) + rng.normal(0, 0.1, (b, n, 3))).astype(F)


def uniform(seed, b, n):
    return np.random.default_rng(seed).uniform(-3, 3, (b, n, 3)).astype(F)


def lattice(seed, b, n):
    """Integer coordinates in a 5 x 5 x 5 grid with spacing 1 (repetitions once n > 125): exact distance ties in every round."""
    return np.random.default_rng(seed).integers(0, 5, (b, n, 3)).astype(F)


def mod512_duplicates(seed, n=1000):
    """One scene.  A small cloud about point 0 = the origin, and two exact ties of the first rounds:
    (+10,0,0) at k = 300 and its duplicate at k + 512 = 812 against (-10,0,0) at 522 (522 mod 512 = 10 < 300: the LARGER index wins);
    (0,+8,0) at k = 100 and its duplicate at 612 against (0,-8,0) at 700 (700 mod 512 = 188 > 100: the smaller index wins).
    Of a duplicate pair the smaller k is sampled and the other never is."""
    v = np.random.default_rng(seed).uniform(-0.5, 0.5, (1, n, 3)).astype(F)
    v[0, 0] = 0
    v[0, 300] = v[0, 812] = (10, 0, 0)
    v[0, 522] = (-10, 0, 0)
    v[0, 100] = v[0, 612] = (0, 8, 0)
    v[0, 700] = (0, -8, 0)
    return v


BOUNDARY_RADIUS = 0.5  # T(0.5) = 0.25 exactly


def boundary(seed, b, n):
    """Point 0 (always the first centre) at the origin; point 1 at squared distance exactly T(0.5) = 0.25: no hit; point 2 at the float
    below it: (0.5 - 2^-25)^2 rounds to 0.25 - 2^-25, plus (2^-13)^2 = 2^-26: a hit.  Everything else lies far away."""
    v = np.random.default_rng(seed).uniform(10, 20, (b, n, 3)).astype(F)
    v[:, 0] = 0
    v[:, 1] = (0.5, 0, 0)
    v[:, 2] = (0, F(0.5) - F(2.0 ** -25), F(2.0 ** -13))
    return v


def huge(seed, b, n):
    """Magnitudes 3e19 .. 1e30, either sign: every square overflows float32."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(np.log10(3e19), 30, (b, n, 3))
    return (mag * rng.choice([-1.0, 1.0], (b, n, 3))).astype(F)


BAD = np.array([np.nan, np.inf, -np.inf], F)


def with_nonfinite(votes, seed, where):
    """NaN and +-Inf in a position: `point0` (one coordinate of point 0 in every scene), `tenth` (a scattered tenth of the points, one to
    three coordinates each), `scene` (every coordinate), `one_scene` (every coordinate of the batch's second scene only)."""
    rng = np.random.default_rng(seed)
    v = votes.copy()
    b, n, _ = v.shape
    if where == "point0":
        for s in range(b):
            v[s, 0, s % 3] = BAD[s % 3]
    elif where == "tenth":
        mask = (rng.random((b, n, 1)) < 0.1) & (rng.random((b, n, 3)) < 0.6)
        v[mask] = BAD[rng.integers(0, 3, int(mask.sum()))]
    elif where == "scene":
        v[:] = BAD[rng.integers(0, 3, v.shape)]
    elif where == "one_scene":
        v[1] = BAD[rng.integers(0, 3, v[1].shape)]
    return v


def _table():
    cases = []
    for i, (b, n, m, k) in enumerate(SHAPES):
        cases.append(("clustered-b%d-n%d-m%d-k%d" % (b, n, m, k), clustered(100 + i, b, n), m, RADIUS, k, "clustered"))
    cases += [
        ("lonely-b3-n1000-m256-k64", uniform(1, 3, 1000), 256, 1e-3, 64, "lonely"),      # every ball holds only its centre
        ("lonely-b1-n65-m8-k1", uniform(2, 1, 65), 8, 1e-3, 1, "lonely"),
        ("lattice-b2-n256-m256-k64", lattice(3, 2, 256), 256, 1.5, 64, "lattice"),
        ("lattice-b1-n513-m32-k64", lattice(4, 1, 513), 32, 1.5, 64, "lattice"),
        ("mod512-b1-n1000-m32-k64", mod512_duplicates(5), 32, RADIUS, 64, "mod512"),
        ("duplicates-b2-n256-m256-k64", np.full((2, 256, 3), 0.75, F), 256, RADIUS, 64, "duplicates"),
        ("duplicates-b1-n2048-m1024-k64", np.full((1, 2048, 3), -1.5, F), 1024, RADIUS, 64, "duplicates"),
        ("boundary-b3-n63-m16-k3", boundary(6, 3, 63), 16, BOUNDARY_RADIUS, 3, "boundary"),
        ("huge-b3-n1000-m256-k64", huge(7, 3, 1000), 256, RADIUS, 64, "huge"),
        ("huge-b1-n64-m64-k64", huge(8, 1, 64), 64, RADIUS, 64, "huge"),
    ]
    for where, (b, n, m, k) in (("point0", (3, 63, 16, 3)), ("point0", (8, 1024, 256, 64)), ("tenth", (3, 1000, 256, 64)),
                                ("tenth", (1, 2048, 1024, 64)), ("scene", (1, 64, 64, 64)), ("scene", (1, 513, 32, 64)),
                                ("one_scene", (2, 256, 256, 64)), ("one_scene", (3, 1000, 256, 64))):
        cases.append(("nonfinite-%s-b%d-n%d-m%d-k%d" % (where, b, n, m, k), with_nonfinite(clustered(200 + n + m, b, n), 9 + n, where),
                      m, RADIUS, k, "nonfinite-" + where))
    return cases


CASES = _table()
IDS = [c[0] for c in CASES]
_results = {}


def results(case):
    """The restatement's result of a case, computed once and shared by the tests that need it; nobody changes it."""
    name, votes, m, radius, k, _ = case
    if name not in _results:
        _results[name] = R.cluster_votes(votes, m, R.threshold(radius), k)
    return _results[name]
