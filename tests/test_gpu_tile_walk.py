"""GPU: the persistent tile walk of the fused GEMMs (votenet_amd/csrc/mlp_fast.hip).  Every family of tests/tile_walk_ref.py is launched
twice -- one row tile per workgroup (the default caps: what every other unit test runs) and WALKED (votenet_debug_fast_workgroups caps the
grid, so that a workgroup takes tile0, tile0 + tstride, ...: the pointer jumps at a tile boundary, the LDS buffers by tile parity, the
prefetch across tiles, the statistics carried over a walk, the coefficient tail's ticket, workgroups that get no tile at all):

* what plain stores write (z / da_prev, the pooled extremes and their rows, the narrow layer's mask) must be BIT-EQUAL in both
  launches: an element is computed by one workgroup in one fixed k order whichever workgroup owns its tile;
* the walked launch against float64 at the tolerances the one-tile launch is held to elsewhere (tests/test_gpu_h2.py for the forward
  layers, tests/test_gpu_backward.py for input gradients, BatchNorm-backward sums and the coefficient tail); what atomics reduce
  (statistics, sums, ug) is compared this way only.

An unwritten tile must not pass: while a test of this module runs, torch.empty hands out device memory filled with NaN (integers:
0x7f7f...), so an output block that the caching allocator recycles from the first launch cannot carry its values into the second."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_stats_ref as S  # noqa: E402
import tile_walk_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_INT = 0x7f7f7f7f


def case_id(c):
    return "%dx%dx%d-gx%d%s%s%s" % (c.rows // 128, c.cin, c.cout, c.gx, "c" if c.chunked else "", "" if c.dev_tiles is None else "-dev%d" % c.dev_tiles,
                                    "-k%d" % c.k if c.k else "")


def cases(family):
    return pytest.mark.parametrize("case", [c for c in R.CASES if c.family == family], ids=case_id)


class Walk:
    def __init__(self, M):
        self.M = M

    def caps(self, cap22=512, cap41=1024, chunk=1):
        # through mlp.debug_switch: graphs captured under other caps are not reused
        self.M.debug_switch("fast_workgroups", cap22, cap41)
        self.M.debug_switch("fast_xcd_chunk", 1 if chunk else 0)

    def one_tile(self, fn):
        self.caps()
        return fn()

    def walked(self, case, fn):
        cap22, cap41 = R.caps_of(case)
        self.caps(cap22, cap41, case.chunked)
        try:
            return fn()
        finally:
            self.caps()

    def runner(self, case):
        """The `run` hook of the stage helpers (test_gpu_narrow / test_gpu_assembled / test_gpu_half): every launch they hand over runs
        walked and with one tile per workgroup, the plain stores of both are compared bit for bit, the helper goes on with the WALKED
        launch's results.  (Walked first: a PendingBN's first consumer derives the BatchNorm from the raw sums in its prologue.)"""
        def run(tag, fn):
            assert tag in R.FAMILIES
            walked = self.walked(case, fn)
            one = self.one_tile(fn)
            for a, b in zip(walked if isinstance(walked, tuple) else (walked,), one if isinstance(one, tuple) else (one,)):
                if a.dim() == 2 and a.dtype != torch.float64:  # (float64: what atomics reduce; one dimension: a tail's coefficient vector)
                    assert same_bits(a, b), tag
                    run.compared += 1
            run.launches += 1
            return walked
        run.launches = run.compared = 0
        return run


@pytest.fixture()
def walk(hiplib, dev, monkeypatch):
    from votenet_amd import mlp as M
    real_empty = torch.empty

    def poisoned_empty(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        if t.is_cuda and t.numel():
            if t.dtype.is_floating_point:
                t.fill_(float("nan"))
            elif t.is_contiguous():
                t.view(torch.uint8).fill_(0x7f)
        return t
    monkeypatch.setattr(torch, "empty", poisoned_empty)
    w = Walk(M)
    w.caps()
    yield w
    w.caps(512, 1024, 1)


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / max(1e-12, float(b.double().abs().max())))


_memo = {}


def memo(key, make):
    """Inputs and float64 references are made once per shape and shared by the cases (and GEMM forms) that use it; nothing writes them."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def images(M, mats, gemm_form, forward):
    """Split-operand images as the model registers them: forward matrices fp16 x 2 under gemm_form 2, everything else bf16 x 3."""
    img = M.SplitImages(mats, pieces=2 if (forward and gemm_form == 2) else 3)
    img.refresh()
    return img


# ---------------------------------------------------------------------------------------------------------------- forward layers


def forward_inputs(dev, rows, cin, cout):
    g = torch.Generator().manual_seed(rows + 3 * cin + 7 * cout)
    f = types.SimpleNamespace()
    f.x = (torch.randn(rows, cin, generator=g) * 2 + 0.3).to(dev)
    f.w = (torch.randn(cin, cout, generator=g) * (2.0 / cin) ** 0.5).to(dev)
    f.b = torch.randn(cout, generator=g).to(dev)
    f.sc = (torch.rand(cin, generator=g) + 0.5).to(dev)
    f.sh = (torch.randn(cin, generator=g) * 0.2).to(dev)
    f.gamma = (torch.randn(cout, generator=g) * 0.3 + 0.2).to(dev)  # mixed signs (the piece layout's pool)
    a = torch.relu(f.x * f.sc + f.sh)  # the loader's two fp32 roundings
    f.ref = a.double() @ f.w.double() + f.b.double()
    f.bound = max(1.0, float((a.abs() @ f.w.abs()).max()))
    return f


def check_forward(f, z, stats, rows=None, weights=None):
    """tests/test_gpu_h2.py, test_h2_gemm_vs_oracle_float64_bf16x3_and_the_fp32_mfma_kernel: 2e-6 of the product magnitude; the
    statistics to rtol 1e-5, atol 1e-3 of it."""
    rows = f.ref.shape[0] if rows is None else rows
    ref = f.ref[:rows]
    if rows:
        e = float((z[:rows].double() - ref).abs().max()) / f.bound
        assert e <= 2e-6, e
    if stats is not None:
        wt = torch.ones(rows, 1, dtype=torch.float64, device=ref.device) if weights is None else weights.double()[:, None]
        sref = torch.cat([(ref * wt).sum(0), (ref * ref * wt).sum(0)])
        assert np.allclose(stats.cpu().numpy(), sref.cpu().numpy(), rtol=1e-5, atol=1e-3 * f.bound)
        # ... and what BatchNorm makes of them: the scale and shift the device derives from these sums against the float64 BatchNorm of
        # the float64 product, 1e-5 of the normalised output (tests/bn_stats_ref.py: metric)
        from votenet_amd import mlp as M
        n = int(round(float(wt.sum())))
        beta = torch.zeros_like(f.gamma)
        sc, sh, _, _ = M.bn_finalize(n, stats, f.gamma, beta)
        m = S.metric(ref.cpu().numpy(), sc.cpu().numpy(), sh.cpu().numpy(), f.gamma.cpu().numpy(), beta.cpu().numpy(), wt[:, 0].cpu().numpy())
        assert float(m["e"].max()) <= S.BAR, float(m["e"].max())


@cases("dense")
def test_dense_forward(walk, dev, gemm_form, case):
    M = walk.M
    f = memo(("fwd", case.rows, case.cin, case.cout), lambda: forward_inputs(dev, case.rows, case.cin, case.cout))
    img = images(M, [f.w], gemm_form, True)
    try:
        for want_stats in (True, False):  # EPI 0 / EPI 1
            fn = lambda: M.linear_dense(f.x, f.w, f.b, f.sc, f.sh, True, want_stats=want_stats)
            z1, _ = walk.one_tile(fn)
            zw, stw = walk.walked(case, fn)
            assert same_bits(zw, z1)
            assert (stw is not None) == want_stats
            check_forward(f, zw, stw)
    finally:
        img.close()


@cases("pool")
def test_pooled_forward(walk, dev, gemm_form, case):
    M = walk.M
    f = memo(("fwd", case.rows, case.cin, case.cout), lambda: forward_inputs(dev, case.rows, case.cin, case.cout))
    img = images(M, [f.w], gemm_form, True)
    try:
        fn = lambda: M.linear_dense_pool(f.x, f.w, 64, f.b, f.sc, f.sh, True, keep_z=True)
        z1, _, pool1 = walk.one_tile(fn)
        zw, stw, poolw = walk.walked(case, fn)
        assert same_bits(zw, z1)
        for a, b in zip(poolw, pool1):  # zmax, zmin and the rows where they are attained
            assert same_bits(a, b)
        check_forward(f, zw, stw)
        grp = zw.cpu().numpy().reshape(case.rows // 64, 64, case.cout)
        zmax, zmin, amax, amin = (p.cpu().numpy() for p in poolw)
        assert (zmax == grp.max(1)).all() and (zmin == grp.min(1)).all()
        assert (amax == grp.argmax(1)).all() and (amin == grp.argmin(1)).all()
    finally:
        img.close()


def piece_counts(G, pieces):
    """pts_cnt of G balls that keep `pieces` pieces in all (a ball keeps ceil(pts_cnt / 16) of its 4): as many balls of three pieces as
    it takes, one of two if the number is odd, the rest of one."""
    extra = pieces - G
    three = extra // 2
    assert 0 <= extra and three + extra % 2 <= G
    cnt = np.full(G, 5, np.int32)
    cnt[(np.arange(three) * G) // max(1, three)] = 40  # spread over the level: kept and dropped pieces alternate
    if extra % 2:
        cnt[np.flatnonzero(cnt == 5)[-1]] = 20
    return cnt


@cases("pool_half")
def test_pooled_forward_on_the_piece_layout(walk, dev, gemm_form, case):
    M = walk.M
    device_count = case.dev_tiles is not None
    tiles = R.ntiles_of(case)
    pieces = tiles * 8
    G = case.rows // 64 if device_count else 8 * ((3 * tiles + 7) // 8)  # (half_groups: a multiple of 8 centres)
    cnt = torch.from_numpy(piece_counts(G, pieces)).to(dev).view(1, G)
    half = M.half_groups(cnt, device_count=device_count).resolve()
    assert half.true_count() == pieces and half.rows == case.rows and (half.nh_limit is not None) == device_count
    valid = pieces * 16
    f = memo(("fwd", case.rows, case.cin, case.cout), lambda: forward_inputs(dev, case.rows, case.cin, case.cout))
    img = images(M, [f.w], gemm_form, True)
    try:
        fn = lambda: M.linear_dense_pool(f.x, f.w, 64, f.b, f.sc, f.sh, True, keep_z=True, half=half, gamma=f.gamma)
        z1, _, (best1, arg1) = walk.one_tile(fn)
        zw, stw, (bestw, argw) = walk.walked(case, fn)
        assert same_bits(zw, z1) and same_bits(bestw, best1) and same_bits(argw, arg1)
        # rows and pieces past the device's count are nobody's to write
        assert bool(torch.isnan(zw[valid:]).all()) and bool(torch.isnan(bestw[pieces:]).all()) and bool((argw[pieces:] == POISON_INT).all())
        weights = torch.ones(valid, device=dev)
        weights[::16] = half.wh[:pieces]
        assert float(half.wh[:pieces].max()) > 1.0
        check_forward(f, zw, stw, rows=valid, weights=weights)
        # one candidate per piece and channel: the max where gamma >= 0, else the min; the first row where it is attained
        zp = zw[:valid].cpu().numpy().reshape(pieces, 16, case.cout)
        sg = np.where(f.gamma.cpu().numpy() >= 0, 1.0, -1.0).astype(np.float32)
        assert (sg < 0).any() and (sg > 0).any()
        assert (bestw[:pieces].cpu().numpy() == sg * (sg * zp).max(1)).all()
        assert (argw[:pieces].cpu().numpy() == (sg * zp).argmax(1)).all()
    finally:
        img.close()


@cases("linear_half")
def test_linear_that_stops_at_the_device_count(walk, dev, gemm_form, case):
    """votenet_mlp_linear_half through the C ABI, the output pre-filled with NaN: rows past 16 * nh_dev[0] stay as they were."""
    from votenet_amd import _lib as L
    M = walk.M
    rows, cin, cout = case.rows, case.cin, case.cout
    valid = case.dev_tiles * 128
    nh = torch.tensor([case.dev_tiles * 8], dtype=torch.int32, device=dev)
    f = memo(("fwd", rows, cin, cout), lambda: forward_inputs(dev, rows, cin, cout))
    img = images(M, [f.w], gemm_form, True)

    def fn():
        z = torch.full((rows, cout), float("nan"), device=dev)
        with L.device_guard(dev):
            L.check(L.lib().votenet_mlp_linear_half(L.ptr(f.x), L.ptr(f.sc), L.ptr(f.sh), 1, rows, cin, cout, L.ptr(f.w), L.ptr(f.b), L.ptr(z),
                                                    L.ptr(nh), L.stream_ptr()))
        return z
    try:
        z1 = walk.one_tile(fn)
        zw = walk.walked(case, fn)
        assert same_bits(zw, z1)
        assert bool(torch.isnan(zw[valid:]).all()) and not bool(torch.isnan(zw[:valid]).any())
        check_forward(f, zw, None, rows=valid)
    finally:
        img.close()


# ---------------------------------------------------------------------------------------------- BatchNorm-backward input gradients


def off_threshold(z, scale, shift):
    """A ReLU decision within fp32 rounding of zero depends on how the compiler contracts z * scale + shift: such inputs (one in
    millions) are moved, so that the float64 reference and the kernel take the same side everywhere."""
    zs = z.double() * scale.double()
    near = (zs + shift.double()).abs() <= 1e-5 * (zs.abs() + shift.double().abs())
    z = torch.where(near, z + 0.0625, z)
    zs = z.double() * scale.double()
    assert not bool(((zs + shift.double()).abs() <= 1e-5 * (zs.abs() + shift.double().abs())).any())
    return z


def backward_inputs(dev, rows, c, cout, k=0):
    g = torch.Generator().manual_seed(rows + 5 * c + 11 * cout + k)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    pos = lambda n: torch.rand(n, generator=g).to(dev) + 0.5
    f = types.SimpleNamespace()
    f.coef, f.wT = rnd(5 * c), rnd(c, cout) * 0.1
    f.z = off_threshold(rnd(rows, c), f.coef[3 * c:4 * c], f.coef[4 * c:])
    f.da = rnd(rows, c)
    f.wh = (1 + 16 * torch.randint(0, 4, (rows // 16,), generator=g)).float().to(dev)  # piece layout: what row 0 of a piece stands for
    if k:
        f.gout = rnd(rows // k, c)
        f.argmax = torch.randint(0, k, (rows // k, c), generator=g, dtype=torch.int32).to(dev)
    # the layer below (EPI 3)
    f.bsc, f.bsh, f.bmu, f.bvar = pos(cout), rnd(cout), rnd(cout), pos(cout)
    f.zb = off_threshold(rnd(rows, cout), f.bsc, f.bsh)
    f.gamma = rnd(cout) * 0.2 + 1.0
    return f


def dz_float64(f, g, relu=True, row_weight=None):
    """BatchNorm backward of a layer from its coefficient vector [A | B | C | scale | shift]: dz = A g [bn(z) > 0] + B + C z; on the piece
    layout g is a total already and the affine part counts row_weight rows."""
    c = f.z.shape[1]
    A, B, C, S, H = f.coef.double().view(5, c)
    z = f.z.double()
    g = g.double()
    if relu:
        g = g * (z * S + H > 0)
    aff = B + C * z
    if row_weight is not None:
        aff = aff * row_weight.double()[:, None]
    return A * g + aff


def pooled_gradient_rows(f, k):
    """(rows / k, c) upstream gradient and arg-max rows -> (rows, c): the gradient at the row the pool took, zero elsewhere."""
    groups, c = f.gout.shape
    g = torch.zeros(groups, k, c, dtype=torch.float64, device=f.gout.device)
    g.scatter_(1, f.argmax.long()[:, None, :], f.gout.double()[:, None, :])
    return g.reshape(groups * k, c)


@cases("dgrad")
def test_input_gradient_from_a_dense_upstream_gradient(walk, dev, gemm_form, case):
    M = walk.M
    f = memo(("bwd", case.rows, case.cin, case.cout, 0), lambda: backward_inputs(dev, case.rows, case.cin, case.cout))
    ref = memo(("bwd-ref", case.rows, case.cin, case.cout, 0), lambda: dz_float64(f, f.da) @ f.wT.double())
    img = images(M, [f.wT], gemm_form, False)
    try:
        fn = lambda: M.dgrad_bn(f.z, f.coef, True, f.wT, da=f.da)
        one = walk.one_tile(fn)
        got = walk.walked(case, fn)
        assert same_bits(got, one)
        assert relerr(got, ref) < 2e-5  # tests/test_gpu_backward.py, test_fused_bn_backward_gemms_match_unfused
    finally:
        img.close()


@cases("dgrad_pooled")
def test_input_gradient_from_a_pooled_upstream_gradient(walk, dev, gemm_form, case):
    from votenet_amd import _lib as L
    M = walk.M
    k = case.k
    f = memo(("bwd", case.rows, case.cin, case.cout, k), lambda: backward_inputs(dev, case.rows, case.cin, case.cout, k))
    ref = memo(("bwd-ref", case.rows, case.cin, case.cout, k), lambda: dz_float64(f, pooled_gradient_rows(f, k)) @ f.wT.double())
    img = images(M, [f.wT], gemm_form, False)
    try:
        fn = lambda: M.dgrad_bn(f.z, f.coef, True, f.wT, gout=f.gout, argmax=f.argmax, k=k)
        one = walk.one_tile(fn)
        assert relerr(one, ref) < 2e-5
        if R.plan_of(case, *R.caps_of(case))[0] == "not served":  # a tile jump that is no whole number of groups
            with pytest.raises(L.InvalidArgumentError):
                walk.walked(case, fn)
            return
        got = walk.walked(case, fn)
        assert same_bits(got, one)
        assert relerr(got, ref) < 2e-5
    finally:
        img.close()


@cases("dgrad_half")
def test_input_gradient_that_stops_at_the_device_count(walk, dev, gemm_form, case):
    M = walk.M
    rows = case.rows
    valid = case.dev_tiles * 128
    f = memo(("bwd", rows, case.cin, case.cout, 0), lambda: backward_inputs(dev, rows, case.cin, case.cout))
    roww = torch.ones(rows, device=dev)
    roww[::16] = f.wh
    ref = memo(("bwd-ref-half", rows, case.cin, case.cout), lambda: dz_float64(f, f.da, row_weight=roww) @ f.wT.double())
    nh = torch.tensor([case.dev_tiles * 8], dtype=torch.int32, device=dev)
    half = types.SimpleNamespace(wh=f.wh, nh_limit=nh, nh_dev=nh, G=rows // 64)
    img = images(M, [f.wT], gemm_form, False)
    try:
        fn = lambda: M.dgrad_bn_half(f.z, f.coef, True, f.wT, f.da, half)
        one = walk.one_tile(fn)
        got = walk.walked(case, fn)
        assert same_bits(got, one)
        assert bool(torch.isnan(got[valid:]).all()) and not bool(torch.isnan(got[:valid]).any())
        if valid:
            assert relerr(got[:valid], ref[:valid]) < 2e-5
    finally:
        img.close()


@cases("dgrad_reduce")
def test_input_gradient_with_the_reduce_of_the_layer_below_and_its_tail(walk, dev, gemm_form, case):
    """EPI 3: the sums against float64 (1e-5 of the sum of their terms' magnitudes: test_fused_bn_backward_gemms_match_unfused), the
    coefficient vector of the tail against the separate votenet_bn_backward_coef launch (test_coefficient_tails_equal_the_separate_launch);
    twice on the SAME ticket, which every workgroup of the walked launch must have taken once and the last one put back to zero."""
    M = walk.M
    rows, c, cout = case.rows, case.cin, case.cout
    f = memo(("bwd", rows, c, cout, 0), lambda: backward_inputs(dev, rows, c, cout))
    ref = memo(("bwd-ref", rows, c, cout, 0), lambda: dz_float64(f, f.da) @ f.wT.double())
    img = images(M, [f.wT], gemm_form, False)
    try:
        for relu_below in (True, False):
            below = (f.zb, f.bsc, f.bsh, f.bmu, f.bvar, relu_below)
            fn = lambda: M.dgrad_bn(f.z, f.coef, True, f.wT, da=f.da, below=below)
            one, _ = walk.one_tile(fn)
            got, sums = walk.walked(case, fn)
            assert same_bits(got, one)
            assert relerr(got, ref) < 2e-5
            gm = got.double() * ((f.zb * f.bsc + f.bsh > 0).double() if relu_below else 1.0)
            zhat = (f.zb.double() - f.bmu.double()) / torch.sqrt(f.bvar.double() + M.BN_EPS)
            exact = torch.cat([gm.sum(0), (gm * zhat).sum(0)])
            scale = torch.cat([gm.abs().sum(0), (gm * zhat).abs().sum(0)])
            assert float(((sums - exact).abs() / (scale + 1e-30)).max()) < 1e-5

            def with_tail(flag):
                dg, db = torch.full((cout,), 0.25, device=dev), torch.full((cout,), -0.5, device=dev)
                prev, M.COEF_TAIL = M.COEF_TAIL, flag
                try:
                    da, coef = M.dgrad_bn(f.z, f.coef, True, f.wT, da=f.da, below=below, below_tail=(rows, f.gamma, dg, db))
                finally:
                    M.COEF_TAIL = prev
                return da, coef, dg, db
            separate = walk.one_tile(lambda: with_tail(False))
            tickets = M._tickets.get(f.z.device)
            for again in range(2):
                if tickets is not None and again:
                    tickets[1] = (tickets[1] - 1) % 64  # the same slot of the rotation as the launch before
                da, coef, dg, db = walk.walked(case, lambda: with_tail(True))
                tickets = M._tickets[f.z.device]
                slot = tickets[1]
                assert again == 0 or slot == last_slot
                last_slot = slot
                assert same_bits(da, one) and coef.shape == (5 * cout,)
                for a, b in zip((coef, dg, db), separate[1:]):
                    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12
            assert int(tickets[0].abs().sum()) == 0
    finally:
        img.close()


# ------------------------------------------------------------------------------------------------ the stage helpers under the caps


def geometry_runs(*geoms):
    runs = sorted(set((c.geom, c.gx, c.chunked) for c in R.CASES if c.geom in geoms))
    return pytest.mark.parametrize("geom,gx,chunked", runs, ids=["%s-gx%d%s" % (g, x, "c" if ch else "") for g, x, ch in runs])


def stage_case(geom, gx, chunked):
    cs = [c for c in R.CASES if (c.geom, c.gx, c.chunked) == (geom, gx, chunked)]
    assert len(set(R.caps_of(c) for c in cs)) == 1  # the helper's forward and input-gradient GEMMs walk under the same caps
    return cs[0]


@geometry_runs("narrow", "narrow_h")
def test_narrow_stage_walked(walk, dev, gemm_form, geom, gx, chunked):
    """SRC 3 (with the mask it records), EPI 4 and EPI 7: the bodies of tests/test_gpu_narrow.py and tests/test_gpu_half.py with their
    fused GEMMs walked -- their float64 assertions hold for the walked launches, the stored outputs equal the one-tile launches'."""
    from test_gpu_half import narrow_stage_kernels_on_compact_rows
    from test_gpu_narrow import narrow_first_layer
    run = walk.runner(stage_case(geom, gx, chunked))
    if geom == "narrow":
        rows = narrow_first_layer(dev, gemm_form, *R.GEOMETRY[geom]["args"], run=run)
        assert run.launches == 2 and run.compared == 1
    else:
        rows = narrow_stage_kernels_on_compact_rows(dev, gemm_form, *R.GEOMETRY[geom]["args"], run=run)
        assert run.launches == 5 and run.compared == 3  # z twice and the mask
    assert rows == R.GEOMETRY[geom]["tiles"] * 128


@geometry_runs("asm", "asm_h17", "asm_h41", "asm_h9", "asm_h208")
def test_assembled_stage_walked(walk, dev, gemm_form, geom, gx, chunked):
    """SRC 4, EPI 6 and, on the piece layout, SRC 5 and the per-XCD chunks (workgroups without a tile included: the coefficient tail of
    the EPI 6 launch still comes out): the bodies of tests/test_gpu_assembled.py and tests/test_gpu_half.py with their fused GEMMs walked."""
    from test_gpu_assembled import assembled_first_layer
    from test_gpu_half import stage_kernels_on_compact_rows
    run = walk.runner(stage_case(geom, gx, chunked))
    if geom == "asm":
        rows = assembled_first_layer(dev, gemm_form, *R.GEOMETRY[geom]["args"], run=run)
        assert run.launches == 2 and run.compared == 2
    else:
        c0, c1 = R.GEOMETRY[geom]["widths"]
        rows = stage_kernels_on_compact_rows(dev, gemm_form, *R.GEOMETRY[geom]["args"], c0=c0, c1=c1, run=run)
        assert run.launches == 4 and run.compared == 4
    assert rows == R.GEOMETRY[geom]["tiles"] * 128
