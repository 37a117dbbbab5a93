"""GPU: the Gram-form backward of a pooled last layer (votenet_amd/csrc/pool_bwd.hip) against tests/pool_bwd_ref.py, the float64
statement of the operation -- every launch on its own (votenet_bn_backward_reduce_pool; votenet_pool_dgrad_prepare + the dense GEMM +
votenet_pool_dgrad_scatter[_half] with and without the reduce of the layer below; votenet_mlp_gram[_half];
votenet_pool_wgrad_sparse[_half][_centres] + votenet_pool_wgrad_finish), every compiled form behind a debug hook, the list edges of the
scatter kernel (tests/pool_bwd_ref.py: PATTERNS), the piece layout, and the early stop at a count only the device knows.

Criterion: |got - ref| <= T * S for EVERY element, S = the reference's expression with every term replaced by its absolute value.
T = 4 x the figure of the project's direct form of the same quantity -- mlp.dgrad_bn / mlp.wgrad_dense_bn on a stored z,
mlp.bn_backward_reduce with argmax, on the fp32 MFMA kernels (test_direct_form_meets_the_tolerance_derived_from_it runs them on the
inputs of this module) -- plus 2e-6 where a split-operand GEMM takes part (tests/test_gpu_bf3.py grants one GEMM that much of its
product magnitude):

    launch   direct form, largest |got - ref| / S (MI355X)             T fp32     T with a split-operand GEMM
    sums     1.48e-7  (128 -> 128,   8 groups, empty_alternating)      5.92e-7    --       (no GEMM)
    da       1.17e-7  ( 64 -> 128, 300 groups, empty_alternating)      4.68e-7    2.47e-6  (gemm_form 2: W diag(C) W^T as fp16 x 2)
    dW       5.82e-7  (128 -> 256, 300 groups, random)                 2.33e-6    --       (the finish reads a float64-made Gram matrix here)
    below    1.22e-8  ( 64 -> 128,   8 groups, random)                 4.88e-8    2.05e-6  (sums of the da above)
    gram     no direct form: dW's figure (a contraction over           2.33e-6    4.33e-6  (gemm_form 1, 2; the piece layout under every
    colsum   the same rows in the same arithmetic)                     2.33e-6    --        form: gram_bf3_kernel is all it has)

The figures are the maxima over the three shapes, G in {8, 300} and the patterns random / one_row_random / empty_alternating / plain
(tests/pool_bwd_ref.py: DIRECT) and over two runs -- dW is summed with fp32 atomics, 5.72e-7 and 5.82e-7.  The largest figures of
the Gram-form launches in the same runs, every form and case of this module: sums 1.86e-7, da 8.6e-8, below 4.1e-8 (pieces,
64 -> 128, one_row_random: the closest to its T), dW 1.59e-6 and colsum 1.57e-6 (the full-layout sparse pass under
votenet_debug_sparse_workgroups(1), 37 groups), gram 8.8e-7 at the default grid and 1.81e-6 for the 960 rows of the piece layout
under votenet_debug_gram_workgroups(1).  One wrong input (test_one_wrong_input_misses_the_criterion) is 11 T in dW at the least.

What bounds the cases under a workgroup cap: T is calibrated on launches whose fp32 accumulators see some 128 rows each before an
atomic combines them.  A cap of ONE workgroup puts every row of the case into one fp32 accumulator, and the rounding of such a chain of
same-signed terms (x >= 0 behind a ReLU, x^2 on the Gram diagonal) grows like sqrt(rows): measured 2.45e-6 (colsum, element 115) and
2.38e-6 (dW, element (115, 46)) for the piece-walking sparse pass of 128 -> 128 over 260 pieces = 4160 rows in one workgroup, 3.07e-6
on the Gram diagonal for 2368 rows in one workgroup -- accumulated rounding, no lost term (a dropped channel of a row is 1e-3 and more,
tests/test_pool_bwd_ref_cpu.py), and no grid the model launches.  So the capped cases are as small as their loops allow: 37 groups
(the walks of the scatter and the sparse pass), 24 centres = 60 pieces (the piece layout), 9 groups = 36 slabs (the Gram matrix).

Two forms of one launch agree with each other within 2 T; bit for bit where the order of the sums is the same (da over the grids of the
scatter pass, the deterministic dW over two runs).  While a test of this module runs torch.empty hands out NaN-filled device memory:
an element no launch wrote cannot pass."""
import contextlib
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_bwd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(128, 256), (128, 128), (64, 128)]  # what votenet_pool_backward_supported serves (k = 64)
shapes = pytest.mark.parametrize("cin,cout", SHAPES, ids=["%dto%d" % s for s in SHAPES])
GROUPS = [1, 7, 8, 9, 17, 33, 300]  # one group; one short of, exactly, one over the 8 wavefronts of a workgroup; ...; a real size
FIGURES = {}  # (launch, what ran) -> the largest |got - ref| / S seen in this process, where, in which case (the record behind the docstring)

# the debug hooks of pool_bwd.hip and their defaults
DEFAULTS = {"votenet_debug_scatter_form": (1,), "votenet_debug_scatter_waves": (16,), "votenet_debug_scatter_workgroups": (0,),
            "votenet_debug_scatter_reverse": (0,), "votenet_debug_sparse_workgroups": (0,), "votenet_debug_sparse_teams": (2, 256),
            "votenet_debug_sparse_centre_workgroups": (0,), "votenet_debug_sparse_centre_teams": (2,), "votenet_debug_zsel_grid": (0, 0),
            "votenet_debug_gram_workgroups": (0,)}


@contextlib.contextmanager
def hooks(M, **kw):
    """with hooks(M, votenet_debug_scatter_form=(0,)): ... -- set through mlp.debug_switch (as tests/test_gpu_tile_walk.py), put back to
    the defaults on the way out."""
    try:
        for name, args in kw.items():
            M.debug_switch(name[len("votenet_debug_"):], *args)
        yield
    finally:
        for name in kw:
            M.debug_switch(name[len("votenet_debug_"):], *DEFAULTS[name])


@contextlib.contextmanager
def setting(obj, name, value):
    prev = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, prev)


@pytest.fixture(autouse=True)
def poisoned_empty(monkeypatch):
    real_empty = torch.empty

    def empty(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        if t.is_cuda and t.numel() and t.dtype.is_floating_point:
            t.fill_(float("nan"))
        return t
    monkeypatch.setattr(torch, "empty", empty)


@pytest.fixture()
def M(hiplib, dev):
    from votenet_amd import mlp
    assert all(mlp.pool_backward_supported(cin, cout, 64) for cin, cout in SHAPES)
    return mlp


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- cases

_memo = {}

COUNTS = {  # the neighbour counts a piece layout is made from
    "full": lambda G, rng: np.full(G, 64),
    "empty": lambda G, rng: np.zeros(G, np.int64),
    "mixed": lambda G, rng: rng.randint(0, 65, G),
    "one": lambda G, rng: np.where(np.arange(G) == 7, 40, 3),  # one ball of 40 among balls of 3
}


def slim(r):
    """Drop what only the margins needed: the (rows, cout) intermediates of a reference are tens of MB at G = 300."""
    for name in ("x", "z", "dz", "S_dz", "below_mask", "below_margin", "below_terms", "gate_margin", "gate_terms", "full_da", "full_S_da"):
        if hasattr(r, name):
            delattr(r, name)
    return r


def case(M, dev, cin, cout, pattern, G, counts=None, device_count=False):
    """-> (inputs on the host, the same on the device, the float64 reference); made once per process.  counts: a piece layout from
    mlp.half_groups on that kind of neighbour counts; device_count: the host holds only the upper bound 4 G of its pieces, the rows past
    the true count are NaN."""
    key = (cin, cout, pattern, G, counts, device_count)
    if key in _memo:
        return _memo[key]
    half = layout = None
    if counts is not None:
        cnt = torch.from_numpy(COUNTS[counts](G, np.random.RandomState(G)).astype(np.int32)).to(dev).view(1, G)
        half = M.half_groups(cnt, device_count=device_count).resolve()
        layout = R.PieceLayout.of(half)
        assert layout.nh % 8 == 0 and (device_count or layout.nh == half.nh)
    c = R.make_case(cin, cout, pattern, G=G, layout=layout, seed=3, extra_rows=(half.nh * R.PIECE - layout.rows) if half is not None else 0)
    r = slim(R.case_reference(c))  # (asserts the margins: before any kernel runs)
    r.tag = "%d -> %d, %d groups, %s" % (cin, cout, G, pattern)
    d = type("Device", (), {})()
    for name in ("xz", "in_scale", "in_shift", "w", "bias", "coef", "gout", "argmax", "zsel", "mean", "var", "bmean", "bvar"):
        setattr(d, name, getattr(c, name).to(dev).contiguous())
    d.wT = d.w.t().contiguous()
    d.aff = torch.stack([d.in_scale, d.in_shift]).contiguous()
    d.scale, d.shift = d.coef[3 * cout:4 * cout], d.coef[4 * cout:]
    d.below = (d.in_scale, d.in_shift, d.bmean, d.bvar, c.in_relu)
    d.half = half
    d.gram_ref = torch.cat([r.gram.float(), torch.zeros(1, cin)]).to(dev)  # what the finish of pool_wgrad reads beside the column sums
    _memo[key] = (c, d, r)
    return _memo[key]


# ---------------------------------------------------------------------------------------------------------------- launches

def sums(M, c, d):
    return M.bn_backward_reduce_pool(d.gout, d.zsel, d.scale, d.shift, d.mean, d.var, c.relu)


def dgrad(M, c, d, below=False):
    """-> da, or (da, sums of the layer below)"""
    return M.pool_dgrad(d.xz, d.in_scale, d.in_shift, c.in_relu, d.w, d.bias, d.wT, d.coef, c.relu, d.gout, d.argmax, d.zsel, c.k,
                        below=d.below if below else None, half=d.half)


def gram(M, c, d):
    return M.gram(d.xz, d.aff, c.in_relu, half=d.half)[:c.cin]


def wgrad(M, c, d):
    """-> dW, column sums.  The Gram matrix the finish multiplies is the reference's (fp32): dW is not judged through votenet_mlp_gram."""
    g = d.gram_ref.clone()
    dw = torch.zeros(c.cin, c.cout, device=d.xz.device)
    M.pool_wgrad(d.xz, d.in_scale, d.in_shift, c.in_relu, g, d.w, d.bias, d.coef, c.relu, d.gout, d.argmax, d.zsel, c.k, dw, half=d.half)
    assert same_bits(g[:c.cin], d.gram_ref[:c.cin])
    return dw, g[c.cin].clone()


# ---------------------------------------------------------------------------------------------------------------- the criterion

def check(launch, got, r, T, what, rows=None):
    """|got - ref| <= T * S element by element; the figure is printed (and kept in FIGURES) before it is judged."""
    ref, S = getattr(r, launch), getattr(r, "S_" + launch)
    got = got.detach().cpu()
    if rows is not None:
        got, ref, S = got[:rows], ref[:rows], S[:rows]
    assert got.shape == ref.shape, (launch, what, tuple(got.shape), tuple(ref.shape))
    q, at = R.excess(got, ref, S)
    print("%-6s %-40s %.3g of S at %s (T = %.3g)" % (launch, what, q, at, T))
    if q > FIGURES.get((launch, what), (-1.0,))[0]:
        FIGURES[(launch, what)] = (q, at, r.tag)
    assert q <= T, "%s, %s (%s): |got - ref| = %.3g S at element %s (got %r, reference %r), T = %.3g" % (
        launch, what, r.tag, q, at, float(got[at]), float(ref[at]), T)


def agree(launch, a, b, r, T, what, rows=None):
    """Two forms of one launch: within 2 T of each other (in units of the reference's S)."""
    S = getattr(r, "S_" + launch)
    a, b = a.detach().cpu(), b.detach().cpu()
    if rows is not None:
        a, b, S = a[:rows], b[:rows], S[:rows]
    q, at = R.excess(a, b, S)
    assert q <= 2 * T, "%s, %s: the two forms differ by %.3g S at element %s" % (launch, what, q, at)


def tol(launch, gemm_form, d, deterministic=False):
    """T of a launch as it runs under the fixture's GEMM form (the table in the module docstring)."""
    if launch in ("da", "below"):
        return R.tolerance(launch, split=gemm_form == 2)
    if launch == "gram":
        return R.tolerance(launch, split=d.half is not None or (gemm_form != 0 and not deterministic))
    return R.tolerance(launch)


def check_all(M, c, d, r, gemm_form, what, rows=None):
    """Every launch in its default form against the reference -> da (for comparisons with other forms)."""
    check("sums", sums(M, c, d), r, tol("sums", gemm_form, d), what)
    da = dgrad(M, c, d)
    check("da", da, r, tol("da", gemm_form, d), what, rows)
    da2, bs = dgrad(M, c, d, below=True)
    assert same_bits(da2[:rows], da[:rows]), what
    check("below", bs, r, tol("below", gemm_form, d), what)
    check("gram", gram(M, c, d), r, tol("gram", gemm_form, d), what)
    dw, cs = wgrad(M, c, d)
    check("dW", dw, r, tol("dW", gemm_form, d), what)
    check("colsum", cs, r, tol("colsum", gemm_form, d), what)
    return da


# ---------------------------------------------------------------------------------------------------------------- full layout

@shapes
@pytest.mark.parametrize("G", GROUPS)
def test_every_launch_at_the_group_counts(M, dev, gemm_form, cin, cout, G):
    """(the dense GEMM inside pool_dgrad serves every row count: rows = 64 included)"""
    c, d, r = case(M, dev, cin, cout, "random", G)
    check_all(M, c, d, r, gemm_form, "full layout")
    with setting(M, "DETERMINISTIC", True):  # the scratch and ordered-reduce path of the sparse pass, the fp32 Gram kernel
        dw, cs = wgrad(M, c, d)
        check("dW", dw, r, tol("dW", gemm_form, d), "full layout, deterministic")
        check("colsum", cs, r, tol("colsum", gemm_form, d), "full layout, deterministic")
        check("gram", gram(M, c, d), r, tol("gram", gemm_form, d, True), "full layout, deterministic")
        dw2, cs2 = wgrad(M, c, d)
        assert same_bits(dw2, dw) and same_bits(cs2, cs)


@shapes
@pytest.mark.parametrize("pattern", [p for p in R.PATTERNS if p != "random"])
def test_every_launch_at_the_list_edges(M, dev, gemm_form, cin, cout, pattern):
    """17 groups: two workgroups of the scatter pass and a lone wavefront in a third."""
    c, d, r = case(M, dev, cin, cout, pattern, 17)
    check_all(M, c, d, r, gemm_form, "full layout, " + pattern)


@shapes
@pytest.mark.parametrize("pattern", ["empty_alternating", "worst_padding"])
def test_scatter_forms_and_walks(M, dev, gemm_form, cin, cout, pattern):
    """37 groups: under votenet_debug_scatter_workgroups(1) a wavefront walks 4 or 5 of them, under (2) 2 or 3, and the walk ends on a
    tail; the workgroup-per-group form takes 19 workgroups of 2 groups, front to back and back to front."""
    c, d, r = case(M, dev, cin, cout, pattern, 37)
    T, Tb = tol("da", gemm_form, d), tol("below", gemm_form, d)
    da = dgrad(M, c, d)
    check("da", da, r, T, "wave form")
    for wgs in (1, 2):
        with hooks(M, votenet_debug_scatter_workgroups=(wgs,)):
            for below in (False, True):
                got = dgrad(M, c, d, below)
                if below:
                    check("below", got[1], r, Tb, "wave form, %d workgroups" % wgs)
                    got = got[0]
                check("da", got, r, T, "wave form, %d workgroups" % wgs)
                assert same_bits(got, da), "da differs between the grids of the scatter pass"
    for reverse in (0, 1):
        with hooks(M, votenet_debug_scatter_form=(0,), votenet_debug_scatter_reverse=(reverse,)):
            for below in (False, True):
                got = dgrad(M, c, d, below)
                if below:
                    check("below", got[1], r, Tb, "workgroup form, reverse %d" % reverse)
                    got = got[0]
                check("da", got, r, T, "workgroup form, reverse %d" % reverse)
                agree("da", got, da, r, T, "workgroup form against wave form")
                if reverse == 0 and not below:
                    front = got
                assert same_bits(got, front), "da differs between the walks of the workgroup form"
    with hooks(M, votenet_debug_scatter_form=(1,), votenet_debug_scatter_reverse=(1,)):  # (the wave form has no reversed walk)
        assert same_bits(dgrad(M, c, d), da)


@shapes
def test_sparse_pass_grids(M, dev, gemm_form, cin, cout):
    """votenet_debug_sparse_workgroups(1): one workgroup stages all 37 groups, (3): 13, 12 and 12; atomics and the deterministic
    scratch path."""
    c, d, r = case(M, dev, cin, cout, "empty_alternating", 37)
    T, Tc = tol("dW", gemm_form, d), tol("colsum", gemm_form, d)
    dw0, cs0 = wgrad(M, c, d)
    check("dW", dw0, r, T, "sparse pass")
    for wgs in (1, 3):
        for det in (False, True):
            with hooks(M, votenet_debug_sparse_workgroups=(wgs,)), setting(M, "DETERMINISTIC", det):
                what = "sparse pass, %d workgroups%s" % (wgs, ", deterministic" if det else "")
                dw, cs = wgrad(M, c, d)
                check("dW", dw, r, T, what)
                check("colsum", cs, r, Tc, what)
                agree("dW", dw, dw0, r, T, what)
                agree("colsum", cs, cs0, r, Tc, what)
                if det:
                    dw2, cs2 = wgrad(M, c, d)
                    assert same_bits(dw2, dw) and same_bits(cs2, cs), what


@shapes
def test_reduction_grids(M, dev, gemm_form, cin, cout):
    """votenet_debug_zsel_grid(groups per workgroup, cap): (1, 1) one workgroup for all 37 groups -- an 8-fold unrolled trip and the
    tail --, (4, 2), (32, 256); votenet_debug_gram_workgroups(1) and (5) over 9 groups = 36 slabs: one row range; four of 8 slabs and
    one of 4."""
    c, d, r = case(M, dev, cin, cout, "empty_alternating", 37)
    T = tol("sums", gemm_form, d)
    s0 = sums(M, c, d)
    for grid in ((1, 1), (4, 2), (32, 256)):
        with hooks(M, votenet_debug_zsel_grid=grid):
            s = sums(M, c, d)
            check("sums", s, r, T, "zsel grid %d, %d" % grid)
            agree("sums", s, s0, r, T, "zsel grid %d, %d" % grid)
    c, d, r = case(M, dev, cin, cout, "random", 9)
    for det in (False, True):
        with setting(M, "DETERMINISTIC", det):
            Tg = tol("gram", gemm_form, d, det)
            g0 = gram(M, c, d)
            for wgs in (1, 5):
                with hooks(M, votenet_debug_gram_workgroups=(wgs,)):
                    g = gram(M, c, d)
                    check("gram", g, r, Tg, "gram, %d workgroups%s" % (wgs, ", deterministic" if det else ""))
                    agree("gram", g, g0, r, Tg, "gram, %d workgroups" % wgs)


# ---------------------------------------------------------------------------------------------------------------- piece layout

LAYOUTS = [("full", 8), ("empty", 16), ("mixed", 8), ("mixed", 24), ("mixed", 104), ("one", 24)]  # (votenet_half_groups: centres in multiples of 8)


def check_pieces(M, c, d, r, gemm_form, what, rows=None):
    da = check_all(M, c, d, r, gemm_form, what, rows)  # (pool_wgrad: the centre-walking form)
    assert M.POOL_WGRAD_CENTRES
    dwc, csc = wgrad(M, c, d)
    with setting(M, "POOL_WGRAD_CENTRES", False):  # the piece-walking form
        dw, cs = wgrad(M, c, d)
    check("dW", dw, r, tol("dW", gemm_form, d), what + ", walking pieces")
    check("colsum", cs, r, tol("colsum", gemm_form, d), what + ", walking pieces")
    agree("dW", dw, dwc, r, tol("dW", gemm_form, d), what + ", pieces against centres")
    agree("colsum", cs, csc, r, tol("colsum", gemm_form, d), what + ", pieces against centres")
    return da


@shapes
@pytest.mark.parametrize("counts,G", LAYOUTS, ids=["%s%d" % l for l in LAYOUTS])
def test_every_launch_on_the_piece_layouts(M, dev, gemm_form, cin, cout, counts, G):
    c, d, r = case(M, dev, cin, cout, "random", G, counts)
    if counts == "full":
        assert d.half.nh == 4 * G
    if counts == "empty":
        assert d.half.nh == G and bool((d.half.wh == 49).all())
    check_pieces(M, c, d, r, gemm_form, "pieces, %s %d" % (counts, G))


@shapes
@pytest.mark.parametrize("pattern", [p for p in R.PATTERNS if p != "random"])
def test_list_edges_on_the_piece_layout(M, dev, gemm_form, cin, cout, pattern):
    """The patterns over the slots of the pieces a ball kept (a ball of one piece under worst_padding: cout + 3 * 16 list entries, the
    capacity of a wavefront's lists)."""
    c, d, r = case(M, dev, cin, cout, pattern, 24, "mixed")
    check_pieces(M, c, d, r, gemm_form, "pieces, " + pattern)


@shapes
def test_forms_and_walks_on_the_piece_layout(M, dev, gemm_form, cin, cout):
    """24 centres, 60 pieces: 16 (12, 8) wavefronts of ONE or TWO scatter workgroups walk them all, 3 to 8 pieces each; the sparse
    passes with one and two teams under their smallest grids: one workgroup stages all 60 pieces (all 24 centres), three a third each."""
    c, d, r = case(M, dev, cin, cout, "empty_alternating", 24, "mixed")
    T, Tb, Tw, Tc = (tol(l, gemm_form, d) for l in ("da", "below", "dW", "colsum"))
    da = dgrad(M, c, d)
    check("da", da, r, T, "pieces")
    for waves in (16, 12):  # (another kernel text at 128 -> 256 only)
        for wgs in (0, 1, 2):
            with hooks(M, votenet_debug_scatter_waves=(waves,), votenet_debug_scatter_workgroups=(wgs,)):
                what = "pieces, %d wavefronts, %d workgroups" % (waves, wgs)
                got, bs = dgrad(M, c, d, below=True)
                check("da", got, r, T, what)
                check("below", bs, r, Tb, what)
                agree("da", got, da, r, T, what)
                if waves == 16:
                    assert same_bits(got, da), "da differs between the grids of the scatter pass"
    dwc, csc = wgrad(M, c, d)
    for teams in (1, 2):
        for wgs in (0, 1, 3):
            with hooks(M, votenet_debug_sparse_centre_teams=(teams,), votenet_debug_sparse_centre_workgroups=(wgs,)):
                what = "centres, %d teams, %d workgroups" % (teams, wgs)
                dw, cs = wgrad(M, c, d)
                check("dW", dw, r, Tw, what)
                check("colsum", cs, r, Tc, what)
                agree("dW", dw, dwc, r, Tw, what)
    with setting(M, "POOL_WGRAD_CENTRES", False):
        for teams, wgs2, wgs in ((1, 0, 0), (1, 0, 1), (1, 0, 3), (2, 1, 0), (2, 3, 0), (2, 256, 0)):
            with hooks(M, votenet_debug_sparse_teams=(teams, wgs2), votenet_debug_sparse_workgroups=(wgs,)):
                what = "pieces, %d teams, caps %d / %d" % (teams, wgs2, wgs)
                dw, cs = wgrad(M, c, d)
                check("dW", dw, r, Tw, what)
                check("colsum", cs, r, Tc, what)
                agree("dW", dw, dwc, r, Tw, what)
    for wgs in (1, 5):
        with hooks(M, votenet_debug_gram_workgroups=(wgs,)):
            check("gram", gram(M, c, d), r, tol("gram", gemm_form, d), "pieces, gram, %d workgroups" % wgs)


@shapes
@pytest.mark.parametrize("pattern", ["random", "empty_alternating"])
def test_launches_stop_at_the_count_on_the_device(M, dev, gemm_form, cin, cout, pattern):
    """A layout whose count only the device knows: every launch is sized for 4 G pieces and stops at nh_dev[0].  The compact rows
    past the count are NaN -- read, they would poison every sum -- and da past the count keeps the NaN torch.empty put there."""
    c, d, r = case(M, dev, cin, cout, pattern, 24, "mixed", device_count=True)
    half, n = d.half, c.layout.nh
    assert half.nh_limit is not None and half.nh == 4 * c.G and c.G <= n < half.nh and n % 8 == 0 and int(half.nh_dev.item()) == n
    assert d.xz.shape[0] == 64 * c.G and bool(torch.isnan(d.xz[16 * n:]).all()) and not bool(torch.isnan(d.xz[:16 * n]).any())
    da = check_pieces(M, c, d, r, gemm_form, "pieces, count on the device", rows=16 * n)
    assert same_bits(da[16 * n:], torch.full_like(da[16 * n:], float("nan"))), "rows past the device's count were written"
    for wgs in (1, 2):
        with hooks(M, votenet_debug_scatter_workgroups=(wgs,)):
            got, bs = dgrad(M, c, d, below=True)
            assert same_bits(got, da)
            check("below", bs, r, tol("below", gemm_form, d), "pieces, count on the device, %d workgroups" % wgs)


@shapes
def test_one_wrong_input_misses_the_criterion(M, dev, gemm_form, cin, cout):
    """The criterion on the device (tests/test_pool_bwd_ref_cpu.py has it on the CPU): the launches run on inputs that differ from the
    reference's in ONE place -- a channel of one group without its gradient; the weight of slot 0 of one ball with dropped pieces set
    to 1 -- and the criterion rejects every launch that place reaches, while the launches it does not reach still pass.  (Not
    asserted of the sums of the layer below: they are judged in units of S summed over ALL rows, where one row's error is small; da
    is where it shows.)"""
    c, d, r = case(M, dev, cin, cout, "random", 24, "mixed")

    def misses(launch, got):
        q, T = R.excess(got.detach().cpu(), getattr(r, launch), getattr(r, "S_" + launch))[0], tol(launch, gemm_form, d)
        print("%-6s wrong input: %.3g of S, %.3g T" % (launch, q, q / T))
        return q > T
    g, ch = [int(v) for v in (r.gated_gout != 0).nonzero()[5]]
    d1 = copy.copy(d)
    d1.gout = d.gout.clone()
    d1.gout[g, ch] = 0.0
    da, _ = dgrad(M, c, d1, below=True)
    dw, cs = wgrad(M, c, d1)
    assert misses("sums", sums(M, c, d1)) and misses("da", da) and misses("dW", dw) and not misses("colsum", cs)
    ball = int((d.half.wh[:c.G] > 1).nonzero()[0])
    d2 = copy.copy(d)
    d2.half = copy.copy(d.half)
    d2.half.wh = d.half.wh.clone()
    d2.half.wh[ball] = 1.0
    da, _ = dgrad(M, c, d2, below=True)
    dw, cs = wgrad(M, c, d2)
    assert misses("da", da) and misses("dW", dw) and misses("colsum", cs) and misses("gram", gram(M, c, d2))
    assert not misses("sums", sums(M, c, d2))
    with setting(M, "POOL_WGRAD_CENTRES", False):
        dw, cs = wgrad(M, c, d2)
    assert misses("dW", dw) and misses("colsum", cs)


# ---------------------------------------------------------------------------------------------------------------- the direct form

@shapes
@pytest.mark.parametrize("G", [8, 300])
@pytest.mark.parametrize("pattern", ["random", "one_row_random", "empty_alternating", "plain"])
def test_direct_form_meets_the_tolerance_derived_from_it(M, dev, cin, cout, G, pattern):
    """The project's other computation of the same quantities, from a stored z on the fp32 MFMA kernels: where the figures of the
    module docstring come from (FIGURES[(launch, 'direct form')] after a run of this test)."""
    c, d, r = case(M, dev, cin, cout, pattern, G)
    z = c.z.to(dev)
    try:
        for name in ("fast_bf3", "wgrad_bf3"):
            M.debug_switch(name, 0)
        s = M.bn_backward_reduce(z, d.scale, d.shift, d.mean, d.var, c.relu, d.gout, argmax=d.argmax, k=c.k)
        dw = torch.zeros(cin, cout, device=dev)
        M.wgrad_dense_bn(d.xz, z, d.coef, c.relu, dw, gout=d.gout, argmax=d.argmax, k=c.k, in_scale=d.in_scale, in_shift=d.in_shift,
                         in_relu=c.in_relu)
        da = M.dgrad_bn(z, d.coef, c.relu, d.wT, gout=d.gout, argmax=d.argmax, k=c.k)
        bs = M.bn_backward_reduce(d.xz, *d.below, da)
    finally:
        for name in ("fast_bf3", "wgrad_bf3"):
            M.debug_switch(name, 1)
    for launch, got in (("sums", s), ("dW", dw), ("da", da), ("below", bs)):
        check(launch, got, r, R.tolerance(launch), "direct form")
