"""CPU: tests/pool_bwd_ref.py IS the derivative of the pooled layer -- against torch autograd in float64 over the real layer,
max_k relu(BN_train(act(xz s + h) W + b)) -- its piece-layout fold against an evaluation on the compact rows, its magnitudes bound
its values, and the per-element criterion |got - ref| <= T * S of tests/test_gpu_pool_bwd.py rejects the errors a kernel of
csrc/pool_bwd.hip could make while it accepts the same expressions evaluated in float32."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_bwd_ref as R  # noqa: E402

LAUNCHES = ("sums", "da", "dW", "below", "gram", "colsum")


def coef_from_sums(rows, gamma, mean, var, sums, scale, shift, eps):
    """bn_bwd_coef_kernel (csrc/mlp_bwd.hip) in float64."""
    c = gamma.numel()
    inv = 1.0 / torch.sqrt(var + eps)
    m1, m2 = sums[:c] / rows, sums[c:] / rows
    A = gamma * inv
    C = -A * inv * m2
    return torch.cat([A, -A * m1 - C * mean, C, scale, shift])


@pytest.mark.parametrize("G,k,cin,cout", [(3, 4, 5, 7), (6, 64, 16, 24)])
def test_reference_is_the_derivative_of_the_layer(G, k, cin, cout):
    gen = torch.Generator().manual_seed(G + cout)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    rows, eps = G * k, R.BN_EPS
    xz, s, h = rnd(rows, cin), rnd(cin) * 0.3 + 1.0, rnd(cin) * 0.2
    w = (rnd(cin, cout) * 0.3).requires_grad_(True)
    b = rnd(cout) * 0.1
    gamma = ((rnd(cout) * 0.3 + 0.8) * torch.where(torch.arange(cout) % 3 == 1, -1.0, 1.0)).requires_grad_(True)  # every third negative
    beta = (rnd(cout) * 0.3).requires_grad_(True)
    assert int((gamma < 0).sum()) > 0 and int((gamma > 0).sum()) > 0
    gout = rnd(G, cout)
    x = torch.relu(xz * s + h).detach().requires_grad_(True)  # d/dx: the gradient with respect to xz without its act'
    z = x @ w + b
    mean, var = z.mean(0), z.var(0, unbiased=False)
    y = gamma * (z - mean) / torch.sqrt(var + eps) + beta
    out = torch.relu(y).view(G, k, cout).max(1).values
    (out * gout).sum().backward()
    # what the forward pass hands to the backward pass
    with torch.no_grad():
        mean, var = mean.detach(), var.detach()
        scale = gamma.detach() / torch.sqrt(var + eps)
        shift = beta.detach() - mean * scale
        argmax = y.view(G, k, cout).argmax(1)
        zsel = z.view(G, k, cout).gather(1, argmax[:, None, :])[:, 0, :]
        args = (xz, s, h, True, w.detach(), b)
        coef0 = torch.cat([torch.zeros(3 * cout, dtype=torch.float64), scale, shift])
        sums = R.reference(*args, coef0, True, gout, argmax, zsel, k, mean, var).sums
        coef = coef_from_sums(rows, gamma.detach(), mean, var, sums, scale, shift, eps)
        r = R.reference(*args, coef, True, gout, argmax, zsel, k, mean, var)
        R.assert_margins(r)
        assert int((r.gated_gout != 0).sum()) > 0 and (k > 4 or int((r.gated_gout == 0).sum()) > 0)  # (a maximum over 64 rows is never gated off)
        for got, want, S in ((r.dW, w.grad, r.S_dW), (r.da, x.grad, r.S_da), (r.sums[:cout], beta.grad, r.S_sums[:cout]),
                             (r.sums[cout:], gamma.grad, r.S_sums[cout:])):
            assert R.excess(got, want, S)[0] < 1e-10


CNT = [0, 64, 17, 3, 40, 16, 33, 64, 1, 48, 5]  # an empty ball, full balls, a 17-neighbour ball, ...


def compact_eval(c, n, wh, dtype=torch.float64, omit_cb=False, gout=None):
    """The quantities of a case on the piece layout computed ON the compact rows, the way the kernels do: pieces 0 .. n - 1, row 0 of
    piece q counted wh[q] times in the dense part, dW in Gram form.  Independent of reference_pieces' expand-and-fold; in float32 the
    stand-in 'kernel' of the mutation test."""
    cv = lambda a: R.f64(a).to(dtype)
    cout, rows = c.cout, n * R.PIECE
    xz = cv(c.xz)[:rows]
    W, b = cv(c.w), cv(c.bias)
    A, B, C, scale, shift = cv(c.coef).view(5, cout)
    x = xz * cv(c.in_scale) + cv(c.in_shift)
    x = torch.relu(x) if c.in_relu else x
    z = x @ W + b
    rw = torch.ones(n, R.PIECE, dtype=dtype)
    rw[:, 0] = cv(wh)[:n]
    rw = rw.reshape(-1, 1)
    zsel, g = cv(c.zsel), cv(c.gout if gout is None else gout)
    gp = g * (zsel * scale + shift > 0) if c.relu else g
    tgt = c.layout.full_index().view(c.G, 64).gather(1, c.argmax.long())  # the compact row of every channel's arg-max slot
    ok = tgt < rows
    dap = torch.zeros(rows, cout, dtype=dtype)
    dap.index_put_((tgt[ok], torch.arange(cout).expand(c.G, cout)[ok]), gp[ok], accumulate=True)
    out = {}
    out["da"] = rw * ((B + C * z) @ W.t()) + (A * dap) @ W.t()
    out["gram"], out["colsum"] = x.t() @ (rw * x), (rw * x).sum(0)
    out["dW"] = (out["gram"] @ W) * C + torch.outer(out["colsum"], B + (0 if omit_cb else C * b)) + x.t() @ (A * dap)
    inv = 1.0 / torch.sqrt(cv(c.var) + R.BN_EPS)
    out["sums"] = torch.cat([gp.sum(0), (gp * ((zsel - cv(c.mean)) * inv)).sum(0)])
    bs, bh, bm, bv, brelu = c.below
    m = (xz * cv(bs) + cv(bh) > 0) if brelu else torch.ones_like(xz)
    out["below"] = torch.cat([(out["da"] * m).sum(0), (out["da"] * m * ((xz - cv(bm)) / torch.sqrt(cv(bv) + R.BN_EPS))).sum(0)])
    return out


def worst(out, r, rows=None):
    w = {}
    for name in LAUNCHES:
        ref, S = getattr(r, name), getattr(r, "S_" + name)
        got = out[name]
        if name == "da" and rows is not None:
            got, ref, S = got[:rows], ref[:rows], S[:rows]
        w[name] = R.excess(got, ref, S)[0]
    return w


@pytest.fixture(scope="module")
def piece_case():
    layout = R.layout_from_counts(CNT)
    c = R.make_case(16, 24, "random", layout=layout, seed=5, extra_rows=R.PIECE)
    c.xz[layout.rows:] = torch.randn(R.PIECE, 16, generator=torch.Generator().manual_seed(1))  # a piece past the count: real numbers, not the layout's
    return c, R.case_reference(c)


def test_piece_layout_fold(piece_case):
    c, r = piece_case
    L = c.layout
    assert L.nh % 8 == 0 and L.wh[0] > 1 and L.wh[1] == 1 and float(L.wh[2]) == 1 + 16 * 2  # empty (a padding piece or more), full, 17 neighbours
    assert torch.equal(torch.bincount(L.full_index(), minlength=L.rows).double(), L.row_weights())
    out = compact_eval(c, L.nh, L.wh)
    for name, q in worst(out, r).items():
        assert q < 1e-10, name
    # the fold keeps the totals, and the ball without neighbours carries all its 64 rows' gradient in its kept rows
    assert R.excess(r.da.sum(0), r.full_da.sum(0), r.S_da.sum(0))[0] < 1e-12
    own = torch.bincount(L.full_index()[:64], minlength=L.rows) > 0
    assert R.excess(r.da[own].sum(0), r.full_da[:64].sum(0), r.S_da[own].sum(0))[0] < 1e-12


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_magnitudes_bound_the_values(pattern):
    for layout in (None, R.layout_from_counts(CNT)):
        c = R.make_case(16, 128, pattern, G=5, layout=layout, seed=2)
        r = R.case_reference(c)
        for name in LAUNCHES:
            v, S = getattr(r, name), getattr(r, "S_" + name)
            assert bool((S >= v.abs() * (1 - 1e-12)).all()), name
        listed = (r.gated_gout != 0)
        if pattern.startswith("empty"):
            assert bool((~listed).all(1).any())
        if pattern == "empty_gated":
            assert not bool(listed.any())
        if pattern in ("worst_padding", "multiples_of_four"):
            assert bool(listed.all())
            per_row = torch.zeros(c.G, 64, dtype=torch.long).scatter_add_(1, c.argmax.long(), torch.ones(c.G, c.cout, dtype=torch.long))
            if pattern == "multiples_of_four":
                assert bool((per_row % 4 == 0).all())
            else:
                slots = layout.kept_slots() if layout is not None else torch.full((c.G,), 64)
                used = torch.arange(64)[None, :] < slots[:, None]
                assert bool((per_row[used] % 4 == 1).all()) and bool((per_row[~used] == 0).all())
                if layout is None:  # the padded lists fill the capacity cout + 3 k exactly
                    assert bool((((per_row + 3) // 4 * 4).sum(1) == c.cout + 3 * 64).all())


def test_criterion_rejects_what_a_kernel_could_get_wrong(piece_case):
    """The float32 evaluation passes the loosest tolerance of tests/test_gpu_pool_bwd.py (a split-operand launch); each mutation fails
    the same tolerance in the launches it touches."""
    c, r = piece_case
    L = c.layout
    T = {name: R.tolerance(name, split=True) for name in LAUNCHES}
    n = L.nh
    wh = torch.cat([L.wh, torch.ones(1, dtype=torch.float64)])
    fails = lambda out, rows=None: {name for name, q in worst(out, r, rows).items() if not q <= T[name]}
    assert fails(compact_eval(c, n, wh, torch.float32)) == set()
    # one channel of one row dropped from the scatter
    g, ch = [int(v) for v in (r.gated_gout != 0).nonzero()[7]]
    gout = c.gout.clone()
    gout[g, ch] = 0.0
    assert fails(compact_eval(c, n, wh, torch.float32, gout=gout)) == {"sums", "da", "dW", "below"}
    # a ball with dropped pieces whose slot 0 counts once
    ball = int((L.wh[:L.G] > 1).nonzero()[1])
    wh1 = wh.clone()
    wh1[ball] = 1.0
    assert fails(compact_eval(c, n, wh1, torch.float32)) == {"da", "dW", "below", "gram", "colsum"}
    # the column-sum part without C b
    assert fails(compact_eval(c, n, wh, torch.float32, omit_cb=True)) == {"dW"}
    # one piece early / late at the device's count (da: the rows of the count; the rows behind it are the sentinel's business)
    early = compact_eval(c, n - 1, wh, torch.float32)
    early["da"] = torch.cat([early["da"], torch.zeros(R.PIECE, c.cin)])
    assert fails(early) >= {"da", "dW", "below", "gram", "colsum"}
    assert fails(compact_eval(c, n + 1, wh, torch.float32), rows=L.rows) == {"dW", "below", "gram", "colsum"}
