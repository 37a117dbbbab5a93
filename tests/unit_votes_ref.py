"""The rule of include/votenet_unit_votes.h twice over, without a device.

forward / backward: a numpy float32 restatement, operation for operation -- the row as (c / 64, 64): lane l owns channels l, l + 64,
...; the per-lane partial accumulated in ascending chunk order; the 64 partials combined by the six-step xor butterfly 32, 16, 8, 4,
2, 1 as p + p[perm]; np.sqrt and / in float32 (both correctly rounded).  The kernels are compared with it by bit pattern.
forward64 / backward64: the independent float64 form, u / |u| and (g - y (y . g)) / |u|, which the restatement is held to on the CPU."""
import numpy as np

F = np.float32
LANES = np.arange(64)
STEPS = (32, 16, 8, 4, 2, 1)


def _quiet():
    return np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def butterfly(p):
    """p (rows, 64) float32 -> (rows,): p + p[partner] over the xor butterfly; every lane ends with the same bits (checked)."""
    assert p.dtype == F and p.shape[1] == 64
    with _quiet():
        for s in STEPS:
            p = p + p[:, LANES ^ s]
    same = (p.view(np.int32) == p.view(np.int32)[:, :1]) | np.isnan(p)
    assert same.all(), "the butterfly leaves different bits in the lanes of a row"
    return p[:, 0].copy()


def lane_sum(a, b):
    """sum_k a_k * b_k per row as the kernels form it.  a, b (rows, c) float32, c % 64 == 0."""
    rows, c = a.shape
    a3, b3 = a.reshape(rows, c // 64, 64), b.reshape(rows, c // 64, 64)
    with _quiet():
        p = a3[:, 0] * b3[:, 0]
        for i in range(1, c // 64):
            p = p + a3[:, i] * b3[:, i]
    return butterfly(p)


def normalise(u):
    """u (rows, c) float32, the un-normalised vote features -> u / |u| (rows, c), |u| (rows), as the kernel forms them."""
    u = np.ascontiguousarray(u, F)
    with _quiet():
        norm = np.sqrt(lane_sum(u, u))
        y = u / norm[:, None]
    assert y.dtype == F and norm.dtype == F
    return y, norm


def forward(x, off):
    """x, off (rows, 3 + c) float32 -> votes_xyz (rows, 3), votes_points (rows, c), norm (rows), all float32."""
    x, off = np.asarray(x, F), np.asarray(off, F)
    with _quiet():
        v_xyz = x[:, :3] + off[:, :3]
        u = x[:, 3:] + off[:, 3:]
    y, norm = normalise(u)
    assert v_xyz.dtype == F
    return v_xyz, y, norm


def backward(d_xyz, cot_xyz, d_points, votes_points, norm, d_width):
    """-> d_votes (rows, d_width) float32: [d_xyz (+ cot_xyz) | (g - y (y . g)) / norm | 0]."""
    g, y, norm = np.asarray(d_points, F), np.asarray(votes_points, F), np.asarray(norm, F)
    rows, c = y.shape
    out = np.zeros((rows, d_width), F)
    with _quiet():
        dot = lane_sum(y, g)
        out[:, 3:3 + c] = (g - y * dot[:, None]) / norm[:, None]
        out[:, :3] = np.asarray(d_xyz, F) if cot_xyz is None else np.asarray(d_xyz, F) + np.asarray(cot_xyz, F)
    return out


def forward64(x, off):
    """The same in float64, independently: -> votes_xyz, u / |u|, |u|."""
    s = np.asarray(x, np.float64) + np.asarray(off, np.float64)
    u = s[:, 3:]
    n = np.sqrt((u * u).sum(1))
    return s[:, :3], u / n[:, None], n


def backward64(d_points, y, norm):
    """(g - y (y . g)) / |u| in float64 (the feature columns only)."""
    g, y = np.asarray(d_points, np.float64), np.asarray(y, np.float64)
    return (g - y * (y * g).sum(1)[:, None]) / np.asarray(norm, np.float64)[:, None]


def backward_bound(d_points, y, norm):
    """2e-6 (|g_k| + |y_k| sum_j |y_j g_j|) / norm, in float64: the condition of (g - y (y . g)) / norm times twenty float32 roundings."""
    g, y = np.abs(np.asarray(d_points, np.float64)), np.abs(np.asarray(y, np.float64))
    return 2e-6 * (g + y * (y * g).sum(1)[:, None]) / np.asarray(norm, np.float64)[:, None]


# ---- the rows every test of the rule uses -------------------------------------------------------------------------------------------
def random_rows(rows, c, seed, scale=1.0):
    """x, off (rows, 3 + c) float32 with entries 0.25 N(0, 1) * scale: at scale 1e18 the squares of c = 512 channels sum to ~6e37,
    inside float32; at 1e-18 the squares are ~1e-38 .. 1e-36, around the smallest normal number."""
    rng = np.random.default_rng(seed)
    x = (0.25 * rng.standard_normal((rows, 3 + c)) * scale).astype(F)
    off = (0.25 * rng.standard_normal((rows, 3 + c)) * scale).astype(F)
    return x, off


SPECIAL = ("plain", "zero", "overflow", "denormal", "nan", "plain")  # row kinds of special_rows, in order


def special_rows(c, seed=3):
    """Six rows: an ordinary one, a row whose features sum to zero, a row whose squares overflow, a row of denormal features, a row
    with one NaN channel, an ordinary one.  The coordinates are ordinary everywhere."""
    x, off = random_rows(len(SPECIAL), c, seed)
    off[1, 3:] = -x[1, 3:]                       # u = 0 exactly
    x[2, 3:] *= F(1e20)                          # u ~ 1e19: squares overflow
    off[2, 3:] *= F(1e20)
    x[3, 3:] *= F(1e-40)                         # denormal operands and sums; every square underflows to zero
    off[3, 3:] *= F(1e-40)
    x[4, 3 + c // 2 + 1] = np.nan
    return x, off
