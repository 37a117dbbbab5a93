"""GPU: the fused GEMM family's entry points (csrc/mlp_fast.hip from votenet_mlp_linear_half down, the four *_wgrad_bn entries of
csrc/mlp_bwd.hip) at the edge of what they serve.

The "shape not served" refusals: every entry with a shape its kernels do not take answers code 1 and its OWN text.  The buffers are real
device memory of the stated shape (rounded up to a whole 128-row tile), so a case that were ever served by mistake would stay in bounds.
(The refusals a VN_REQUIRE makes before anything looks at a device are in tests/test_fused_entry_checks_cpu.py.)

One served call per entry at the smallest served shape -- rows = 128, widths 64, k0 = 4 -- against the float64 restatements of the
neighbouring files at their tolerances: the plain entries through the bodies of test_gpu_narrow.py and test_gpu_assembled.py, the
piece-layout (_half) entries with eight pieces of weight one, which is the full layout: the narrow ones through the same body, the
assembled and dense ones against their plain twins at the tolerances test_gpu_half.py compares the two layouts with.
Not repeated here, because those files call them directly: votenet_mlp_linear_half (test_gpu_tile_walk.py: it requires nh_dev),
votenet_narrow_linear_masked and votenet_narrow_dgrad_bn_reduce_masked (test_gpu_half.py: the mask needs the coefficient tail)."""
import ctypes
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

LINEAR_HALF = "mlp_linear_half: shape not served (rows % 128 == 0, cin % 32 == 0, cout % 64 == 0, 16-byte aligned)"
DGRAD = "mlp_dgrad_bn: shape not supported by the fused kernel (use votenet_bn_backward_apply + votenet_mlp_linear)"
DGRAD_HALF = "mlp_dgrad_bn_half: shape not served (rows % 128 == 0, c % 32 == 0, cout % 64 == 0, 16-byte aligned buffers)"
DGRAD_REDUCE = "mlp_dgrad_bn_reduce: shape not supported by the fused kernel (use votenet_mlp_dgrad_bn + votenet_bn_backward_reduce)"
NARROW_LINEAR = ("narrow_linear: shape not served (rows % 128 == 0, c0 % 32 == 0, c0 <= 128, cout == 64 or cout % 128 == 0, "
                 "16-byte aligned buffers)")
NARROW_DGRAD = ("narrow_dgrad_bn_reduce: shape not served (rows % 128 == 0, c % 32 == 0, c <= 512, c0 == 64 or c0 % 128 == 0, "
                "16-byte aligned buffers)")
NARROW_DGRAD_MASKED = "narrow_dgrad_bn_reduce_masked: shape not served (as votenet_narrow_dgrad_bn_reduce)"
ASM_LINEAR = "assembled_linear: shape not served (rows % 128 == 0, c0 % 32 == 0, c0 <= 512, cout % 64 == 0, 16-byte aligned buffers)"
ASM_LINEAR_HALF = "assembled_linear_half: shape not served (as votenet_assembled_linear)"
ASM_DGRAD = "assembled_dgrad_bn_reduce: shape not served (as votenet_mlp_dgrad_bn_reduce)"
ASM_DGRAD_HALF = "assembled_dgrad_bn_reduce_half: shape not served (as votenet_mlp_dgrad_bn_reduce)"
NARROW_WGRAD = "narrow_wgrad_bn: shape not served (c0 % 64 == 0, cout % 64 == 0, 16-byte aligned buffers)"
NARROW_WGRAD_HALF = "narrow_wgrad_bn_half: shape not served (as votenet_narrow_wgrad_bn)"
ASM_WGRAD = "assembled_wgrad_bn: shape not served (c0 % 64 == 0, cout % 64 == 0, 16-byte aligned buffers)"
ASM_WGRAD_HALF = "assembled_wgrad_bn_half: shape not served (as votenet_assembled_wgrad_bn)"

ROWS, WIDTH, WGRAD_WIDTH = (100, 64, 64), (128, 48, 64), (128, 48, 64)  # (rows, contraction width, output width)
NOT_SERVED = [
    ("votenet_mlp_linear_half", LINEAR_HALF, [ROWS, WIDTH]),
    ("votenet_mlp_dgrad_bn", DGRAD, [ROWS, WIDTH]),
    ("votenet_mlp_dgrad_bn_half", DGRAD_HALF, [ROWS, WIDTH]),
    ("votenet_mlp_dgrad_bn_reduce", DGRAD_REDUCE, [ROWS, WIDTH]),
    ("votenet_narrow_linear", NARROW_LINEAR, [ROWS, WIDTH]),
    ("votenet_narrow_linear_half", NARROW_LINEAR, [WIDTH]),  # (its own check refuses rows % 128 != 0 before: the CPU file)
    ("votenet_narrow_linear_masked", NARROW_LINEAR, [(128, 192, 64)]),  # (likewise, and c0 % 64 != 0: here the c0 > 128 no narrow loader takes)
    ("votenet_narrow_dgrad_bn_reduce", NARROW_DGRAD, [ROWS, WIDTH, (128, 64, 96)]),
    ("votenet_narrow_dgrad_bn_reduce_half", NARROW_DGRAD, [ROWS, WIDTH, (128, 64, 96)]),
    ("votenet_narrow_dgrad_bn_reduce_masked", NARROW_DGRAD_MASKED, [ROWS, WIDTH]),  # (c0 = 96 is refused by its own check before)
    ("votenet_assembled_linear", ASM_LINEAR, [ROWS, WIDTH]),
    ("votenet_assembled_linear_half", ASM_LINEAR_HALF, [ROWS, WIDTH]),
    ("votenet_assembled_dgrad_bn_reduce", ASM_DGRAD, [ROWS, WIDTH]),
    ("votenet_assembled_dgrad_bn_reduce_half", ASM_DGRAD_HALF, [ROWS, WIDTH]),
    ("votenet_narrow_wgrad_bn", NARROW_WGRAD, [WGRAD_WIDTH]),
    ("votenet_narrow_wgrad_bn_half", NARROW_WGRAD_HALF, [WGRAD_WIDTH]),
    ("votenet_assembled_wgrad_bn", ASM_WGRAD, [WGRAD_WIDTH]),
    ("votenet_assembled_wgrad_bn_half", ASM_WGRAD_HALF, [WGRAD_WIDTH]),
]


def entry_args(entry, rows, c, cout, p, tail):
    """The argument list of `entry` for a rows x c operand and a width-cout result.  p(name) -> the address of the buffer of that name
    (every buffer holds at least a whole tile of rows and 128 columns); tail: a complete votenet_coef_tail, by reference.
    k0 = 4; nh_dev NULL where the entry lets it be."""
    dz = (p("da"), p("z"), p("coef"), 1, p("w"))  # da, zsrc, coef, relu, wT
    first_bn = (p("scale"), p("shift"), None, 1)  # in_scale, in_shift, in_bn, in_relu
    below = (p("scale"), p("shift"), p("mean"), p("var"), 1e-3, 1, p("sums"))
    narrow, asm = (p("u8"), p("w0"), p("b0")), (p("geo"), p("P"), p("wx"))
    narrow_linear = (rows, 4, c, cout) + narrow + first_bn + (p("w"), p("bias"), p("out"), p("stats"))
    narrow_dgrad = (rows, c, cout, 4) + dz + narrow + below + (p("ug"),)
    asm_linear = (rows, c, cout) + asm + first_bn + (p("w"), p("bias"), p("out"), p("stats"))
    asm_dgrad = (rows, c, cout) + dz + (p("out"),) + asm + below
    wgrad = (p("scale"), p("shift"), 1, p("da"), p("z"), p("coef"), 1)
    return {
        "votenet_mlp_linear_half": lambda: (p("x"), p("scale"), p("shift"), 1, rows, c, cout, p("w"), p("bias"), p("out"), p("nh"), None),
        "votenet_mlp_dgrad_bn": lambda: (rows, c, cout, p("da"), None, None, 0, p("z"), p("coef"), 1, p("w"), p("out"), None),
        "votenet_mlp_dgrad_bn_half": lambda: (rows, c, cout) + dz + (p("out"), p("wh"), None, None),
        "votenet_mlp_dgrad_bn_reduce": lambda: (rows, c, cout) + dz + (p("out"), p("x")) + below + (None, None),
        "votenet_narrow_linear": lambda: narrow_linear + (None,),
        "votenet_narrow_linear_half": lambda: narrow_linear + (p("wh"), None),
        "votenet_narrow_linear_masked": lambda: narrow_linear + (p("wh"), p("mask"), None),
        "votenet_narrow_dgrad_bn_reduce": lambda: narrow_dgrad + (None, None),
        "votenet_narrow_dgrad_bn_reduce_half": lambda: narrow_dgrad + (None, p("wh"), None),
        "votenet_narrow_dgrad_bn_reduce_masked": lambda: narrow_dgrad + (tail, p("wh"), p("mask"), None),
        "votenet_assembled_linear": lambda: asm_linear + (None,),
        "votenet_assembled_linear_half": lambda: asm_linear + (p("wh"), None, None),
        "votenet_assembled_dgrad_bn_reduce": lambda: asm_dgrad + (None, None),
        "votenet_assembled_dgrad_bn_reduce_half": lambda: asm_dgrad + (None, p("wh"), None, None),
        "votenet_narrow_wgrad_bn": lambda: (rows, 4, c, cout) + narrow + wgrad + (p("dw"), None, None),
        "votenet_narrow_wgrad_bn_half": lambda: (rows, 4, c, cout) + narrow + wgrad + (p("wh"), p("dw"), None),
        "votenet_assembled_wgrad_bn": lambda: (rows, c, cout) + asm + wgrad + (p("dw"), None, None),
        "votenet_assembled_wgrad_bn_half": lambda: (rows, c, cout) + asm + wgrad + (p("wh"), p("dw"), None, None),
    }[entry]()


@pytest.fixture(scope="module")
def buffers(dev):
    """Zeroed device memory for every operand of every entry at the shapes of NOT_SERVED: 128 rows (a whole tile: rows = 100 rounded up)
    of 256 floats, 256 x 256 matrices, vectors of 5 * 256; 16 pieces of weight one."""
    f = lambda *s: torch.zeros(*s, device=dev)
    t = {n: f(128, 256) for n in ("x", "z", "da", "out", "P")}
    t.update({n: f(256, 256) for n in ("w", "dw")})
    t.update({n: f(5 * 256) for n in ("coef", "scale", "shift", "mean", "var", "bias", "b0", "gamma", "tcoef")})
    t.update(u8=f(128, 8), w0=f(8, 256), geo=f(128, 4), wx=f(3, 256), wh=torch.ones(16, device=dev),
             sums=torch.zeros(2 * 256, dtype=torch.float64, device=dev), stats=torch.zeros(2 * 256, dtype=torch.float64, device=dev),
             ug=torch.zeros(8 * 256, dtype=torch.float64, device=dev), mask=torch.zeros(128, 16, dtype=torch.int16, device=dev),
             nh=torch.full((1,), 8, dtype=torch.int32, device=dev), ticket=torch.zeros(4, dtype=torch.int32, device=dev))
    return t


@pytest.mark.parametrize("entry,text,shapes", NOT_SERVED, ids=[e[0][len("votenet_"):] for e in NOT_SERVED])
def test_unserved_shapes_are_refused_with_the_entry_s_own_text(hiplib, dev, buffers, entry, text, shapes):
    from votenet_amd import _lib as L
    tail = L.CoefTail()
    tail.ticket, tail.rows, tail.gamma, tail.coef = buffers["ticket"].data_ptr(), 128, buffers["gamma"].data_ptr(), buffers["tcoef"].data_ptr()
    for rows, c, cout in shapes:
        args = entry_args(entry, rows, c, cout, lambda name: buffers[name].data_ptr(), ctypes.byref(tail))
        fn = getattr(hiplib, entry)
        assert len(args) == len(fn.argtypes)
        with L.device_guard(dev):
            rc = fn(*args)
        assert rc == 1 and hiplib.votenet_last_error() == text.encode(), (rows, c, cout, rc, hiplib.votenet_last_error())
    torch.cuda.synchronize()


def test_plain_narrow_entries_at_the_smallest_served_shape(hiplib, dev):
    """votenet_narrow_linear, votenet_narrow_wgrad_bn, votenet_narrow_dgrad_bn_reduce: 1 scene x 2 balls x 64 slots, one feature channel."""
    from test_gpu_narrow import narrow_first_layer
    assert narrow_first_layer(dev, 1, 1, 300, 2, 64, 1, 64, 64) == 128


def test_half_narrow_entries_at_the_smallest_served_shape(hiplib, dev, monkeypatch):
    """votenet_narrow_linear_half, votenet_narrow_wgrad_bn_half, votenet_narrow_dgrad_bn_reduce_half on eight pieces of weight one: the
    same rows, the same float64 restatement."""
    from test_gpu_narrow import narrow_first_layer
    from votenet_amd import mlp as M
    unit = types.SimpleNamespace(wh=torch.ones(8, device=dev), nh_limit=None)
    called = []
    for name in ("narrow_linear", "narrow_wgrad_bn", "narrow_dgrad_bn_reduce"):
        def on_pieces(*a, _fn=getattr(M, name), _name=name, **k):
            called.append(_name)
            return _fn(*a, half=unit, **k)
        monkeypatch.setattr(M, name, on_pieces)
    assert narrow_first_layer(dev, 1, 1, 300, 2, 64, 1, 64, 64) == 128
    assert set(called) == {"narrow_linear", "narrow_wgrad_bn", "narrow_dgrad_bn_reduce"}


def test_plain_assembled_entries_at_the_smallest_served_shape(hiplib, dev):
    """votenet_assembled_linear, votenet_assembled_wgrad_bn, votenet_assembled_dgrad_bn_reduce and, as their stored-layer reference,
    votenet_mlp_dgrad_bn_reduce: 1 scene x 2 balls x 64 slots, 16 feature channels."""
    from test_gpu_assembled import assembled_first_layer
    assert assembled_first_layer(dev, 1, 1, 400, 2, 64, 16, 64, 64, 0.3) == 128


def test_half_assembled_and_dense_entries_at_the_smallest_served_shape(hiplib, dev):
    """votenet_assembled_linear_half, votenet_assembled_wgrad_bn_half, votenet_assembled_dgrad_bn_reduce_half and votenet_mlp_dgrad_bn_half
    on eight pieces of weight one against their plain twins (votenet_mlp_dgrad_bn for the last, itself against float64), at the
    tolerances of test_gpu_half.py::stage_kernels_on_compact_rows: z bit for bit, statistics 1e-6, gradients and sums 1e-5."""
    from test_gpu_half import relerr
    from votenet_amd import mlp as M
    rows, npts, cf, c0, c1 = 128, 40, 16, 64, 64
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    unit = types.SimpleNamespace(wh=torch.ones(rows // 16, device=dev), nh_limit=None)
    geo = rnd(rows, 4)
    geo[:, 3] = torch.randint(0, npts, (rows,), generator=g, dtype=torch.int32).view(torch.float32).to(dev)
    P, wx, w1 = rnd(npts, c0), rnd(3, c0) * 0.3, rnd(c0, c1) * 0.2
    w1T = w1.t().contiguous()
    z0 = M.assemble_z0(geo, P, wx)
    bn0 = M.FrozenBN(torch.stack([rnd(c0) * 0.2 + 1.0, rnd(c0) * 0.1]).contiguous())
    z1, st1 = M.assembled_linear(geo, P, wx, w1, None, bn0)
    z1h, st1h = M.assembled_linear(geo, P, wx, w1, None, bn0, half=unit)
    assert relerr(z1, torch.relu(z0.double() * bn0.scale.double() + bn0.shift.double()) @ w1.double()) < 2e-5
    assert torch.equal(z1h, z1) and relerr(st1h[:c1], st1[:c1]) < 1e-6 and relerr(st1h[c1:], st1[c1:]) < 1e-6
    da1, coef1 = rnd(rows, c1), rnd(5 * c1) * 0.3
    dw1, dw1h = torch.zeros(c0, c1, device=dev), torch.zeros(c0, c1, device=dev)
    M.assembled_wgrad_bn(geo, P, wx, bn0.scale, bn0.shift, True, z1, coef1, True, da1, dw1)
    M.assembled_wgrad_bn(geo, P, wx, bn0.scale, bn0.shift, True, z1, coef1, True, da1, dw1h, half=unit)
    assert float(dw1.abs().max()) > 0 and relerr(dw1h, dw1) < 1e-5
    mean0, var0 = z0.mean(0), z0.var(0, unbiased=False)
    below0 = (bn0.scale, bn0.shift, mean0, var0, True)
    da0, sums0 = M.assembled_dgrad_bn_reduce(z1, coef1, True, w1T, da1, geo, P, wx, below0)
    da0h, sums0h = M.assembled_dgrad_bn_reduce(z1, coef1, True, w1T, da1, geo, P, wx, below0, half=unit)
    assert relerr(da0h, da0) < 1e-5
    zh0 = (z0.double() - mean0.double()) / torch.sqrt(var0.double() + M.BN_EPS)
    scale0 = torch.cat([da0.double().abs().sum(0), (da0.double() * zh0).abs().sum(0)])
    assert float(((sums0h - sums0).abs() / (scale0 + 1e-30)).max()) < 1e-5
    # the dense pair: the plain entry against float64 (the restatement of test_gpu_narrow.py, its 2e-5), the piece layout against it
    g1 = da1.double() * (z1.double() * coef1[3 * c1:4 * c1].double() + coef1[4 * c1:].double() > 0)
    dz1 = coef1[:c1].double() * g1 + coef1[c1:2 * c1].double() + coef1[2 * c1:3 * c1].double() * z1.double()
    dp = M.dgrad_bn(z1, coef1, True, w1T, da=da1)
    assert relerr(dp, dz1 @ w1T.double()) < 2e-5 and relerr(da0, dz1 @ w1T.double()) < 2e-5
    assert relerr(M.dgrad_bn_half(z1, coef1, True, w1T, da1, unit), dp) < 1e-5
