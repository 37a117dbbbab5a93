"""The backward of a pooled last layer (votenet_amd/csrc/pool_bwd.hip: conv + BatchNorm + ReLU + max over the k rows of a group)
restated in float64 on the CPU (torch).  No device code, no kernel-shaped tricks: the Gram-form launches compute

    x   = act(xz * in_scale + in_shift)                         the layer's input activation
    z   = x W + b
    da' = gout at row g*k + argmax[g,c], gated by [zsel*scale + shift > 0] when relu, zero elsewhere
    dz  = A da' + B + C z                                        coef = [A | B | C | scale | shift] (csrc/mlp_bwd.hip, bn_bwd_apply)

and from them sums = [sum da' | sum da' zhat(zsel)], dW = x^T dz, da = dz W^T, the Gram matrix x^T x with its column sums, and --
with the layer below given -- the BatchNorm-backward sums of that layer over (da, xz).

reference()         the full layout; every result with its magnitude S: the same expression with every term replaced by its absolute
                    value.  Tolerances are in units of S, element by element (excess()).
reference_pieces()  the piece layout (csrc/half.hip): expand the compact rows, run reference(), fold da back as totals per compact row.
PieceLayout         a piece layout on the host (what mlp.HalfLayout holds on the device), layout_from_counts() builds one without a device.
make_case()         inputs of a test: a shape, a layout, an arg-max pattern; gates and the ReLU of the layer below kept off their thresholds.

The gates are comparisons: a value within rounding of zero may flip in fp32.  reference() returns the margins |zsel*scale + shift|
and |xz*bscale + bshift| with their term magnitudes; assert_margins() is what every test calls before a kernel runs."""
import types

import numpy as np
import torch

BN_EPS = 1e-5  # votenet_amd.mlp.BN_EPS
PIECE, BALL_PIECES, TILE_PIECES = 16, 4, 8  # rows per piece, pieces per ball, pieces per 128-row GEMM tile (csrc/half.hip)
MARGIN = 1e-4  # no gate closer to its threshold than this share of its terms' magnitudes

# |got - ref| <= T * S per element.  DIRECT: the largest |got - ref| / S of the project's direct form of the same quantity (mlp.dgrad_bn,
# mlp.wgrad_dense_bn on a stored z, mlp.bn_backward_reduce with argmax; fp32 MFMA kernels) on the inputs of tests/test_gpu_pool_bwd.py
# against reference(), as measured on an MI355X (the figures and what was measured: that module's docstring).  T = 4 * DIRECT -- the
# margin covers another association of the sums, not a lost term -- plus, where a split-operand GEMM takes part, the 2e-6 of product
# magnitude the project grants one (tests/test_gpu_bf3.py).
DIRECT = {"sums": 1.48e-7, "da": 1.17e-7, "dW": 5.82e-7, "below": 1.22e-8}
SPLIT = 2e-6


def tolerance(launch, split=False):
    """launch: sums | da | dW | below | gram | colsum.  The Gram matrix and its column sums have no direct form: they are contractions
    over the same rows as dW in the same arithmetic, and take dW's figure."""
    base = DIRECT["dW" if launch in ("gram", "colsum") else launch]
    return 4 * base + (SPLIT if split else 0.0)


def f64(a):
    if torch.is_tensor(a):
        return a.detach().to("cpu", torch.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def i64(a):
    if torch.is_tensor(a):
        return a.detach().to("cpu", torch.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.int64)


def reference(xz, in_scale, in_shift, in_relu, w, bias, coef, relu, gout, argmax, zsel, k, mean=None, var=None, eps=BN_EPS, below=None,
              dtype=torch.float64):
    """The arguments of the entry points (mean / var: what votenet_bn_backward_reduce_pool takes for zhat; below = (scale, shift, mean,
    var, relu) of the layer that produced xz).  -> a namespace: sums, dW, da, gram, colsum, below (when given), each with S_<name>;
    gate_margin / gate_terms (G, cout) and below_margin / below_terms (rows, cin).  dtype: float32 evaluates the same expressions in
    fp32 (the stand-in 'kernel' of tests/test_pool_bwd_ref_cpu.py)."""
    cv = (lambda a: None if a is None else f64(a).to(dtype))
    xz, w, gout, zsel, coef = cv(xz), cv(w), cv(gout), cv(zsel), cv(coef)
    in_scale, in_shift, bias, mean, var = cv(in_scale), cv(in_shift), cv(bias), cv(mean), cv(var)
    argmax = i64(argmax)
    rows, cin = xz.shape
    cout = w.shape[1]
    G = gout.shape[0]
    assert rows == G * k and argmax.shape == (G, cout) and zsel.shape == (G, cout) and coef.numel() == 5 * cout
    assert int(argmax.min()) >= 0 and int(argmax.max()) < k
    A, B, C, scale, shift = coef.view(5, cout)
    b = bias if bias is not None else torch.zeros(cout, dtype=dtype)
    r = types.SimpleNamespace()
    x = xz
    if in_scale is not None:
        x = xz * in_scale + in_shift
        if in_relu:
            x = torch.relu(x)
    z = x @ w + b
    r.x, r.z = x, z
    # the pooled gradient at its rows
    pre = zsel * scale + shift
    r.gate_margin, r.gate_terms = (pre.abs(), (zsel * scale).abs() + shift.abs()) if relu else (None, None)
    gate = (pre > 0).to(dtype) if relu else torch.ones_like(pre)
    gp = gout * gate
    r.gated_gout = gp
    dap = torch.zeros(G, k, cout, dtype=dtype)
    dap.scatter_(1, argmax[:, None, :], gp[:, None, :])
    dap = dap.reshape(rows, cout)
    dz = A * dap + B + C * z
    S_dz = (A * dap).abs() + B.abs() + C.abs() * (x.abs() @ w.abs() + b.abs())
    r.dz, r.S_dz = dz, S_dz
    if mean is not None:
        inv = 1.0 / torch.sqrt(var + eps)
        r.sums = torch.cat([gp.sum(0), (gp * ((zsel - mean) * inv)).sum(0)])
        r.S_sums = torch.cat([gp.abs().sum(0), (gp.abs() * ((zsel.abs() + mean.abs()) * inv)).sum(0)])
    r.dW, r.S_dW = x.t() @ dz, x.abs().t() @ S_dz
    r.da, r.S_da = dz @ w.t(), S_dz @ w.abs().t()
    r.gram, r.S_gram = x.t() @ x, x.abs().t() @ x.abs()
    r.colsum, r.S_colsum = x.sum(0), x.abs().sum(0)
    if below is not None:
        bs, bh, bm, bv, brelu = below
        bs, bh, bm, bv = cv(bs), cv(bh), cv(bm), cv(bv)
        pre = xz * bs + bh
        r.below_margin, r.below_terms = (pre.abs(), (xz * bs).abs() + bh.abs()) if brelu else (None, None)
        m = (pre > 0).to(dtype) if brelu else torch.ones_like(pre)
        binv = 1.0 / torch.sqrt(bv + eps)
        r.below = torch.cat([(r.da * m).sum(0), (r.da * m * ((xz - bm) * binv)).sum(0)])
        r.S_below = torch.cat([(r.S_da * m).sum(0), (r.S_da * m * ((xz.abs() + bm.abs()) * binv)).sum(0)])
        r.below_mask = m
    return r


class PieceLayout:
    """A piece layout on the host: G centres, nh pieces.  pos (G, 3): where pieces 1..3 of a centre sit among the pieces past the first
    G (-1: dropped), hc (nh,): piece q is piece hc[q] % 4 of centre hc[q] / 4, wh (nh,): what row 0 of a piece stands for."""

    def __init__(self, G, pos, hc, wh, nh=None):
        self.G = int(G)
        self.nh = int(nh if nh is not None else len(hc))
        self.pos = i64(pos).reshape(self.G, BALL_PIECES - 1)
        self.hc = i64(hc)[:self.nh]
        self.wh = f64(wh)[:self.nh]
        assert self.G <= self.nh <= BALL_PIECES * self.G and int(self.pos.max()) < self.nh - self.G
        self.rows = self.nh * PIECE

    @classmethod
    def of(cls, half):
        """From a resolved mlp.HalfLayout (true_count(): the device's count where the host holds only the upper bound)."""
        return cls(half.G, half.pos, half._hc, half._wh, half.true_count())

    def full_index(self):
        """(64 G,) the compact row that holds each slot of the full layout; a slot of a dropped piece -> the ball's slot 0
        (mlp.HalfLayout.full_index)."""
        G = self.G
        c = torch.arange(G)[:, None]
        s = torch.arange(64)[None, :]
        j = s // PIECE
        posx = torch.cat([torch.zeros(G, 1, dtype=torch.long), self.pos], 1)
        p = torch.gather(posx, 1, j.expand(G, 64))
        return torch.where(j == 0, c * PIECE + s, torch.where(p >= 0, (G + p) * PIECE + s % PIECE, c * PIECE)).reshape(-1)

    def kept_slots(self):
        """(G,) a ball's slots 0 .. kept_slots - 1 lie in pieces it kept."""
        return PIECE * (1 + (self.pos >= 0).sum(1))

    def row_weights(self):
        w = torch.ones(self.nh, PIECE, dtype=torch.float64)
        w[:, 0] = self.wh
        return w.reshape(-1)


def layout_from_counts(cnt):
    """votenet_half_groups restated (as tests/test_gpu_half.py:layout_reference): a ball keeps pieces 0 .. ceil(cnt / 16) - 1; the first
    pieces of all centres, then the others centre by centre, then all-copy pieces until the count is a multiple of 8."""
    cnt = np.asarray(cnt)
    G = cnt.size
    kc = np.clip((np.maximum(cnt, 1) + PIECE - 1) // PIECE, 1, BALL_PIECES)
    pos = np.full((G, BALL_PIECES - 1), -1, np.int64)
    hc = [c * BALL_PIECES for c in range(G)]
    for c in range(G):
        for j in range(1, kc[c]):
            pos[c, j - 1] = len(hc) - G
            hc.append(c * BALL_PIECES + j)
    c = 0
    while len(hc) % TILE_PIECES:
        for j in range(1, BALL_PIECES):
            if len(hc) % TILE_PIECES and pos[c, j - 1] < 0:
                pos[c, j - 1] = len(hc) - G
                hc.append(c * BALL_PIECES + j)
        c += 1
    wh = np.ones(len(hc))
    wh[:G] = 1 + PIECE * (BALL_PIECES - 1 - (pos >= 0).sum(1))
    return PieceLayout(G, pos, np.array(hc), wh)


def reference_pieces(layout, xz_h, in_scale, in_shift, in_relu, w, bias, coef, relu, gout, argmax, zsel, mean=None, var=None, eps=BN_EPS,
                     below=None, dtype=torch.float64):
    """The piece-layout expectation from the full-layout one.  xz_h: compact rows (the first layout.rows are read).  da, S_da, the
    margins of the layer below: per compact row (da: the sum over the full rows a compact row stands for); everything else is
    unchanged by the layout."""
    fi = layout.full_index()
    assert int(i64(argmax).max(1).values.sub(layout.kept_slots()).max()) < 0, "an arg-max in a piece its ball dropped"
    xz = f64(xz_h)[:layout.rows][fi]
    r = reference(xz, in_scale, in_shift, in_relu, w, bias, coef, relu, gout, argmax, zsel, 64, mean, var, eps, below, dtype)
    r.full_da, r.full_S_da = r.da, r.S_da
    for name in ("da", "S_da"):
        t = torch.zeros(layout.rows, xz.shape[1], dtype=dtype)
        t.index_add_(0, fi, getattr(r, name))
        setattr(r, name, t)
    if below is not None:  # (a compact row's copies carry the same value: any of them states its margin)
        for name in ("below_margin", "below_terms") if below[4] else ():
            t = torch.zeros(layout.rows, xz.shape[1], dtype=dtype)
            t[fi] = getattr(r, name)
            setattr(r, name, t)
    return r


def assert_margins(r, margin=MARGIN):
    """No gated entry within `margin` of its threshold (relative to its terms).  Exact zeros excluded: 0 > 0 is false in every arithmetic."""
    for m, t, what in ((r.gate_margin, r.gate_terms, "gate"), (getattr(r, "below_margin", None), getattr(r, "below_terms", None), "layer below")):  # (None: no gate)
        if m is None:
            continue
        bad = (m < margin * t) & (t > 0)
        assert not bool(bad.any()), "%s: %d entries within %g of the ReLU threshold" % (what, int(bad.sum()), margin)


def excess(got, ref, S):
    """max over the elements of |got - ref| / S (0 / 0 = 0, x / 0 = inf) and the index where it is attained."""
    d = (f64(got) - f64(ref)).abs()
    S = f64(S)
    q = torch.where(S > 0, d / S.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    i = int(q.reshape(-1).argmax())
    return float(q.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(q.shape)))


# ---------------------------------------------------------------------------------------------------------------- test inputs

PATTERNS = ("random", "one_row_first", "one_row_last", "one_row_random", "worst_padding", "multiples_of_four", "empty_gout", "empty_gated",
            "empty_alternating", "plain")


def _split_counts(gen, total, n, unit, base):
    """n counts of the form base + unit * a, a >= 0, summing to `total` (spread at random)."""
    extra = (total - base * n) // unit
    assert extra >= 0 and base * n + unit * extra == total
    a = torch.bincount(torch.randint(0, n, (extra,), generator=gen), minlength=n)
    return base + unit * a


def pattern_argmax(pattern, gen, cout, slots, pre):
    """(G, cout) arg-max slots and a (G, cout) mask of the entries whose gout is to be zero.  slots (G,): a group's usable slots are
    0 .. slots - 1; pre (G, 64, cout): the gate's pre-activation of every row (for the patterns that pick gated-off rows)."""
    G = slots.numel()
    arg = torch.zeros(G, cout, dtype=torch.int64)
    zero = torch.zeros(G, cout, dtype=torch.bool)
    u = lambda *s: torch.rand(*s, generator=gen)
    for g in range(G):
        n = int(slots[g])
        if pattern in ("random", "plain", "empty_gout"):
            arg[g] = torch.randint(0, n, (cout,), generator=gen)
        elif pattern == "one_row_first":
            arg[g] = 0
        elif pattern == "one_row_last":
            arg[g] = n - 1
        elif pattern == "one_row_random":
            arg[g] = int(torch.randint(0, n, (1,), generator=gen))
        elif pattern in ("worst_padding", "multiples_of_four"):
            # worst_padding: every usable row holds 1 mod 4 channels (full layout: cout + 3 k list entries after padding, the capacity;
            # piece layout: that for a ball of one piece).  multiples_of_four: no padding at all; four per row where the rows suffice
            if pattern == "worst_padding":
                counts = _split_counts(gen, cout, n, 4, 1)
            elif cout // 4 <= n:
                counts = torch.zeros(n, dtype=torch.int64)
                counts[torch.randperm(n, generator=gen)[:cout // 4]] = 4
            else:
                counts = _split_counts(gen, cout, n, 4, 4)
            arg[g, torch.randperm(cout, generator=gen)] = torch.repeat_interleave(torch.arange(n), counts)
        elif pattern in ("empty_gated", "empty_alternating"):
            arg[g] = torch.randint(0, n, (cout,), generator=gen)
    if pattern == "empty_gout":
        zero[torch.rand(G, generator=gen) < 0.5] = True
        zero[0] = True
        zero[-1] = False if G > 1 else True
    if pattern in ("empty_gated", "empty_alternating"):
        # an empty group: every channel on a row whose pre-activation is negative (gated off); where a channel has none, gout = 0
        empty = torch.ones(G, dtype=torch.bool) if pattern == "empty_gated" else torch.rand(G, generator=gen) < 0.5
        if pattern == "empty_alternating" and G > 1:
            empty[0], empty[1] = False, True
        usable = torch.arange(64)[None, :, None] < slots[:, None, None]
        neg = (pre < -0.05) & usable  # (far enough that the nudge off the threshold in make_case never meets it)
        pick = (u(G, 64, cout) * neg).argmax(1)
        none = ~neg.any(1)
        arg = torch.where(empty[:, None] & ~none, pick, arg)
        zero = empty[:, None] & none
        if pattern == "empty_alternating":  # every other empty group is empty by its gradient instead
            by_gout = empty & (torch.cumsum(empty.long(), 0) % 2 == 0)
            zero = zero | by_gout[:, None]
    return arg, zero


def make_case(cin, cout, pattern="random", G=None, layout=None, seed=0, extra_rows=0):
    """Inputs (CPU float32 / int32 tensors in a namespace) of a pooled layer of G groups of 64 rows -- or, with a PieceLayout, of its
    compact rows (plus extra_rows rows of NaN behind them: what a launch must not read).  pattern: one of PATTERNS; 'plain' is 'random'
    with relu = in_relu = False.  Some BatchNorm scales are negative in every case."""
    assert pattern in PATTERNS
    k = 64
    G = layout.G if layout is not None else G
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * G + 31 * cin + cout + 101 * PATTERNS.index(pattern))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    c = types.SimpleNamespace(cin=cin, cout=cout, G=G, k=k, pattern=pattern, layout=layout)
    c.relu = pattern not in ("plain", "worst_padding", "multiples_of_four")  # (the padding patterns need every channel listed)
    c.in_relu = pattern != "plain"
    rows = layout.rows if layout is not None else G * k
    c.in_scale = (rnd(cin) * 0.3 + 1.0) * torch.where(torch.arange(cin) % 5 == 3, -1.0, 1.0)
    c.in_shift = rnd(cin) * 0.2
    c.bmean, c.bvar = rnd(cin) * 0.1, torch.rand(cin, generator=gen) + 0.5
    xz = rnd(rows, cin)
    c.w, c.bias = rnd(cin, cout) * 0.15, rnd(cout) * 0.1
    c.coef = rnd(5 * cout) * 0.3
    c.coef[3 * cout:4 * cout] = (rnd(cout) * 0.3 + 0.9) * torch.where(torch.arange(cout) % 4 == 1, -1.0, 1.0)  # scale: every fourth negative
    c.coef[4 * cout:] = rnd(cout) * 0.3 - 0.2
    assert int((c.coef[3 * cout:4 * cout] < 0).sum()) > 0 and int((c.in_scale < 0).sum()) > 0
    c.mean, c.var = rnd(cout) * 0.1, torch.rand(cout, generator=gen) + 0.5
    c.gout = rnd(G, cout)
    c.below = (c.in_scale, c.in_shift, c.bmean, c.bvar, c.in_relu)
    # the arg-max rows by the pattern; zsel and the stored z of the direct form: the float32 of the float64 z.  No gate may sit within
    # 10 MARGIN of its threshold, and nothing may be inconsistent for it -- zsel IS z at the arg-max row -- so the INPUTS move: an
    # element of xz off the threshold of the layer below, a channel to the next row, or (a pattern that fixes the rows) the whole
    # xz row of the group by 1/16
    scale, shift = c.coef[3 * cout:4 * cout].double(), c.coef[4 * cout:].double()
    near = lambda v, s, h: (v.double() * s.double() + h.double()).abs() <= 10 * MARGIN * ((v.double() * s.double()).abs() + h.double().abs())
    slots = layout.kept_slots() if layout is not None else torch.full((G,), k)
    fi = layout.full_index() if layout is not None else torch.arange(G * k)
    arg = None
    for attempt in range(50):
        if c.in_relu:
            xz = torch.where(near(xz, c.in_scale, c.in_shift), xz + 0.0625, xz)
        x = xz[fi].double() * c.in_scale.double() + c.in_shift.double()
        z = ((torch.relu(x) if c.in_relu else x) @ c.w.double() + c.bias.double()).view(G, k, cout)
        if arg is None:
            arg, zero = pattern_argmax(pattern, gen, cout, slots, z * scale + shift)
            c.gout[zero] = 0.0
        zsel = z.float().gather(1, arg[:, None, :])[:, 0, :]
        bad = near(zsel, scale, shift) if c.relu else torch.zeros(G, cout, dtype=torch.bool)
        if not bool(bad.any()):
            break
        if pattern.startswith("one_row"):
            g = bad.any(1).nonzero()[:, 0]
            xz[fi[g * k + arg[g, 0]]] += 0.0625
        else:
            arg = torch.where(bad, (arg + 1) % slots[:, None], arg)
    else:
        raise AssertionError("no inputs off the thresholds after 50 attempts")
    c.z, c.zsel, c.argmax = z.float().reshape(G * k, cout), zsel.contiguous(), arg.to(torch.int32)
    xz_full = xz[fi]
    c.xz_full = xz_full
    c.xz = xz if not extra_rows else torch.cat([xz, torch.full((extra_rows, cin), float("nan"))])
    return c


def case_reference(c, dtype=torch.float64):
    """reference() / reference_pieces() on a case of make_case, margins asserted."""
    if c.layout is None:
        r = reference(c.xz, c.in_scale, c.in_shift, c.in_relu, c.w, c.bias, c.coef, c.relu, c.gout, c.argmax, c.zsel, c.k, c.mean, c.var,
                      below=c.below, dtype=dtype)
    else:
        r = reference_pieces(c.layout, c.xz, c.in_scale, c.in_shift, c.in_relu, c.w, c.bias, c.coef, c.relu, c.gout, c.argmax, c.zsel, c.mean,
                             c.var, below=c.below, dtype=dtype)
    assert_margins(r)
    return r
