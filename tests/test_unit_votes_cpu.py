"""CPU: unit-length vote features without a device -- the numpy float32 restatement of include/votenet_unit_votes.h
(tests/unit_votes_ref.py) against its independent float64 form inside derived bounds, the properties of the rule (unit norm, a gradient
orthogonal to the features, the zero / overflowing / NaN rows), and the interface: the header's entries, the library's argument checks
(host pointers: nothing is launched), the switch of VoteNetHotPath.

The bounds.  With d = 2^-24: u_k = x + off is one rounding.  The sum of squares has no cancellation; each product is one rounding and
the sum takes c / 64 - 1 + 6 additions, so |u|^2 is within (2 + 1 + c / 64 + 5) d <= 16 d of the true one at c = 512, |u| within
8 d + d for the root, and y = u / |u| within (1 + 9 + 1) d = 6.6e-7 of the float64 y: the bar is 1e-6 |y64|.  The backward's
(g_k - y_k dot) / norm has the condition (|g_k| + |y_k| sum_j |y_j g_j|) / norm; the roundings on it -- y's 11 d twice, the products,
the c / 64 + 5 additions of dot, the difference, the quotient, the norm's 9 d -- are first-order terms of mixed sign, and their sum
stays below 2e-6 = 34 d of that condition on every row tried here, which this file checks before the GPU tests rely on it."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_votes_ref as R  # noqa: E402

from votenet_amd import _lib as L  # noqa: E402

F = np.float32
NAMES = ["votenet_unit_votes", "votenet_unit_votes_backward", "votenet_unitvote_last_error"]
SHAPES = [(64, 37), (256, 129), (512, 65)]  # (c, rows)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _gradient(rows, c, seed, scale=1.0):
    rng = np.random.default_rng(seed + 100)
    return (rng.standard_normal((rows, c)) * scale).astype(F)


# ------------------------------------------------------------------ the restatement against float64
@pytest.mark.parametrize("scale", [1.0, 1e-18, 1e18], ids=["unit-scale", "scaled-1e-18", "scaled-1e18"])
@pytest.mark.parametrize("c,rows", SHAPES)
def test_restatement_stays_inside_the_derived_bounds_of_the_float64_form(c, rows, scale):
    x, off = R.random_rows(rows, c, 10 + c, scale)
    v_xyz, y, norm = R.forward(x, off)
    x64, y64, n64 = R.forward64(x, off)
    assert np.isfinite(y).all() and np.isfinite(norm).all() and (norm > 0).all()
    assert np.array_equal(bits(v_xyz), bits((x64).astype(F)))  # one rounding of the exact sum
    err = np.abs(y.astype(np.float64) - y64)
    print("forward: worst |y - y64| / |y64| = %.3g (bar 1e-6), norm %.3g" % (float((err / np.abs(y64)).max()), float(np.abs(norm / n64 - 1).max())))
    assert (err <= 1e-6 * np.abs(y64)).all()
    assert (np.abs(norm.astype(np.float64) - n64) <= 1e-6 * n64).all()
    # the backward on the restatement's own y and norm, against float64 on the float64 ones (y is of unit scale whatever u's is)
    g = _gradient(rows, c, c)
    d = R.backward(np.zeros((rows, 3), F), None, g, y, norm, 3 + c)[:, 3:]
    d64 = R.backward64(g, y64, n64)
    bound = R.backward_bound(g, y64, n64)
    derr = np.abs(d.astype(np.float64) - d64)
    print("backward: worst |d - d64| / bound = %.3g of the 2e-6 bar" % float((derr / bound).max()))
    assert np.isfinite(d).all() and (derr <= bound).all()


# ------------------------------------------------------------------ the properties of the rule
@pytest.mark.parametrize("c,rows", SHAPES)
def test_features_have_unit_norm_and_the_gradient_is_orthogonal_to_them(c, rows):
    x, off = R.random_rows(rows, c, 20 + c)
    _, y, norm = R.forward(x, off)
    y64 = y.astype(np.float64)
    assert (np.abs(np.sqrt((y64 * y64).sum(1)) - 1.0) <= 1e-6).all()
    g = _gradient(rows, c, c)
    d = R.backward(np.zeros((rows, 3), F), None, g, y, norm, 3 + c)[:, 3:].astype(np.float64)
    bound = R.backward_bound(g, y64, norm)
    assert (np.abs((y64 * d).sum(1)) <= (np.abs(y64) * bound).sum(1)).all()  # the projection removed the component along y
    assert (np.abs((y64 * g).sum(1)) > 100 * (np.abs(y64) * bound).sum(1) * norm).any()  # ... which the raw gradient has


def test_backward_writes_the_coordinates_the_cotangent_and_a_zero_tail():
    c, rows = 64, 5
    x, off = R.random_rows(rows, c, 31)
    _, y, norm = R.forward(x, off)
    g = _gradient(rows, c, 1)
    dx, cot = _gradient(rows, 3, 2), _gradient(rows, 3, 3)
    dx[0, 0] = F(-0.0)
    plain = R.backward(dx, None, g, y, norm, 3 + c + 29)
    both = R.backward(dx, cot, g, y, norm, 3 + c + 29)
    assert np.array_equal(bits(plain[:, :3]), bits(dx)) and np.signbit(plain[0, 0])  # no cotangent: d_xyz itself, not d_xyz + 0
    assert np.array_equal(bits(both[:, :3]), bits(dx + cot))
    assert np.array_equal(bits(plain[:, 3:]), bits(both[:, 3:])) and not plain[:, 3 + c:].any() and plain.shape == (rows, 96)


@pytest.mark.parametrize("c", [64, 256, 512])
def test_zero_overflowing_denormal_and_nan_rows_behave_as_the_rule_says_and_touch_no_other_row(c):
    x, off = R.special_rows(c)
    v_xyz, y, norm = R.forward(x, off)
    kinds = list(R.SPECIAL)
    zero, over, den, nan = (kinds.index(k) for k in ("zero", "overflow", "denormal", "nan"))
    assert np.isnan(y[zero]).all() and norm[zero] == 0            # 0 / 0; the norm itself is sqrtf(0)
    assert np.isposinf(norm[over]) and not y[over].any() and np.isfinite(x[over]).all()
    u = x[den, 3:] + off[den, 3:]
    assert (np.abs(u[u != 0]) < np.finfo(F).tiny).all() and u.any() and norm[den] == 0 and np.isinf(y[den][u != 0]).all()
    assert np.isnan(y[nan]).all() and np.isnan(norm[nan])
    assert np.isfinite(v_xyz).all()
    # the ordinary rows are, bit for bit, what they are without the special rows beside them
    px, poff = R.random_rows(len(kinds), c, 3)
    _, py, pn = R.forward(px, poff)
    for r in (0, len(kinds) - 1):
        assert np.array_equal(bits(y[r]), bits(py[r])) and bits(norm[r:r + 1]) == bits(pn[r:r + 1])
        assert abs(float(np.sqrt((y[r].astype(np.float64) ** 2).sum())) - 1) <= 1e-6
    g = _gradient(len(kinds), c, 5)
    d = R.backward(np.zeros((len(kinds), 3), F), None, g, y, norm, 3 + c)
    pd = R.backward(np.zeros((len(kinds), 3), F), None, g, py, pn, 3 + c)
    for r in (0, len(kinds) - 1):
        assert np.array_equal(bits(d[r]), bits(pd[r])) and np.isfinite(d[r]).all()
    assert np.isnan(d[zero, 3:]).all() and np.isnan(d[nan, 3:]).all() and not d[over, 3:].any()


# ------------------------------------------------------------------ the interface
def test_header_declares_the_three_entries_and_the_binding_follows_it(hiplib):
    inc = os.path.join(os.path.dirname(L.__file__), os.pardir, "include")
    with open(os.path.join(inc, L.SIDE_LIBS["unitvote"])) as f:
        protos = L.parse_header(f.read(), {})
    I, V, Lg = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert sorted(protos) == NAMES
    assert protos["votenet_unitvote_last_error"] == (ctypes.c_char_p, [])
    assert protos["votenet_unit_votes"] == (I, [Lg, I, V, Lg, V, Lg, V, V, V, V])
    assert protos["votenet_unit_votes_backward"] == (I, [Lg, I, V, V, V, V, V, V, Lg, I, V])
    lib = L.side_lib("unitvote")
    for name in NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes or [])) == protos[name]
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", L.side_path("unitvote")], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[2] for line in out.splitlines()) == NAMES


def test_the_library_checks_its_arguments_before_anything_is_launched(hiplib):
    """Every refused shape and null pointer returns 1 with the limit in the text, from host pointers: no device is needed."""
    lib = L.side_lib("unitvote")
    buf = np.zeros(1 << 14, F)
    p0 = buf.ctypes.data
    err = lambda: lib.votenet_unitvote_last_error().decode()

    def fwd(rows=4, c=256, x=p0, xp=259, off=p0, op=288, vx=p0, vp=p0, norm=p0):
        return lib.votenet_unit_votes(rows, c, x, xp, off, op, vx, vp, norm, None)

    def bwd(rows=4, c=256, dx=p0, cot=None, g=p0, y=p0, norm=p0, d=p0, dp=288, dw=288):
        return lib.votenet_unit_votes_backward(rows, c, dx, cot, g, y, norm, d, dp, dw, None)
    channels = "64 to 512 channels in multiples of 64 expected, got c = %d"
    for kw, text in ((dict(c=0), channels % 0), (dict(c=96), channels % 96), (dict(c=576), channels % 576), (dict(c=-64), channels % -64),
                     (dict(xp=258), "at least 3 + c = 259 elements expected, got x_pitch = 258"),
                     (dict(op=258), "at least 3 + c = 259 elements expected, got x_pitch = 259, off_pitch = 258"),
                     (dict(c=64, xp=66, op=67), "at least 3 + c = 67 elements expected, got x_pitch = 66"),
                     (dict(rows=-1), "rows expected, got rows = -1"), (dict(x=None), "null"), (dict(off=None), "null"), (dict(vx=None), "null"),
                     (dict(vp=None), "null"), (dict(norm=None), "null"), (dict(rows=0, c=96), channels % 96)):
        assert fwd(**kw) == 1, kw
        assert "unit_votes:" in err() and text in err(), (kw, err())
    for kw, text in ((dict(c=0), channels % 0), (dict(c=96), channels % 96), (dict(c=576), channels % 576),
                     (dict(dw=258, dp=288), "d_width of at least 3 + c = 259 columns expected, got d_width = 258"),
                     (dict(dw=288, dp=287), "d_pitch >= d_width = 288 elements expected, got d_pitch = 287"),
                     (dict(dw=259, dp=258), "d_pitch >= d_width = 259 elements expected, got d_pitch = 258"),
                     (dict(rows=-1), "rows expected, got rows = -1"), (dict(dx=None), "null"), (dict(g=None), "null"), (dict(y=None), "null"),
                     (dict(norm=None), "null"), (dict(d=None), "null"), (dict(rows=0, dw=10, dp=10), "got d_width = 10")):
        assert bwd(**kw) == 1, kw
        assert "unit_votes_backward:" in err() and text in err(), (kw, err())
    # no row: ok, nothing is launched, whatever the buffers
    assert fwd(rows=0) == 0 and fwd(rows=0, x=None, off=None, vx=None, vp=None, norm=None) == 0
    assert bwd(rows=0) == 0 and bwd(rows=0, dx=None, g=None, y=None, norm=None, d=None) == 0
    assert fwd(rows=0, c=64, xp=67, op=67) == 0 and fwd(rows=0, c=512, xp=515, op=515) == 0 and bwd(rows=0, c=512, dp=515, dw=515) == 0
    with pytest.raises(L.InvalidArgumentError, match=r"multiples of 64 expected, got c = 96"):
        L.check(fwd(c=96), side="unitvote")


def test_the_mode_is_off_by_default_and_an_unknown_mode_is_refused():
    from votenet_amd import unit_votes as UV
    from votenet_amd.model import VoteNetHotPath
    assert UV.MODES == ("unit",)
    assert UV.supported(64) and UV.supported(256) and UV.supported(512)
    assert not UV.supported(0) and not UV.supported(96) and not UV.supported(576)
    assert VoteNetHotPath.vote_features is None
    net = object.__new__(VoteNetHotPath)  # the switch needs no device
    with pytest.raises(L.InvalidArgumentError, match=r"mode must be one of unit, got 'nonsense'"):
        net.enable_vote_features("nonsense")
    assert net.vote_features is None
    net.enable_vote_features()
    assert net.vote_features == "unit" and "vote_features" in net.__dict__
    assert net.proposal_sampling is None and net.vote_supervision is None and net.proposal_supervision is None  # the other modes stay
    net.disable_vote_features()
    assert net.vote_features is None
    net.enable_vote_features("unit")
    assert net.vote_features == "unit" and VoteNetHotPath.vote_features is None


def test_python_entries_refuse_host_tensors_and_wrong_shapes():
    import torch
    from votenet_amd import unit_votes as UV
    x = torch.zeros(4, 259)
    with pytest.raises(L.VotenetError, match="no CPU fallback"):
        UV.unit_votes(x, x)
    with pytest.raises(L.InvalidArgumentError, match="2-D row-major view"):
        UV.unit_votes(x.view(2, 2, 259), x)
    with pytest.raises(L.InvalidArgumentError, match="2-D row-major view"):
        UV.unit_votes(x.t(), x.t())
