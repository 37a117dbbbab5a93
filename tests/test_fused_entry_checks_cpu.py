"""The argument checks of the fused GEMM family's entry points (csrc/mlp_fast.hip from votenet_mlp_linear_half down, the four *_wgrad_bn
entries of csrc/mlp_bwd.hip): every call below has exactly ONE fault and is refused by a VN_REQUIRE, i.e. before anything looks at a
device -- the non-null pointers are small fake addresses that nothing dereferences.  Each row asserts the return code and the whole text
of votenet_last_error().  The texts are what the library answered before the launch surface was folded into argument builders and one
impl per twin set; they are the record that the folding changed no check and no text.  (With several faults in one call the text depends
on the order of the checks: not a property, not tested.  The "shape not served" refusals need real buffers: tests/test_gpu_fused_entries.py.)"""
import ctypes

import pytest


def A(k):
    return 16 * k  # a fake, 16-byte aligned device address


def _tail(**over):
    """A complete votenet_coef_tail (fake addresses) with the given fields overridden."""
    from votenet_amd import _lib
    t = _lib.CoefTail()
    t.ticket, t.rows, t.gamma, t.coef, t.dgamma, t.dbeta = A(40), 128, A(41), A(42), A(43), A(44)
    for k, v in over.items():
        setattr(t, k, v)
    return t


# the four ways a coefficient tail can be incomplete
BAD_TAILS = [dict(tail=("tail", dict(ticket=None))), dict(tail=("tail", dict(gamma=None))), dict(tail=("tail", dict(coef=None))),
             dict(tail=("tail", dict(rows=0)))]


def nulls(*names):
    return [{n: None} for n in names]


# the accepted argument list of every entry, in the order of its prototype (include/votenet_hip.h)
NARROW_LINEAR = dict(rows=128, k0=4, c0=64, cout=64, u8=A(1), w0=A(2), b0=A(3), in_scale=A(4), in_shift=A(5), in_bn=None, in_relu=1,
                     w=A(6), bias=A(7), z=A(8), stats=A(9))
NARROW_DGRAD = dict(rows=128, c=64, c0=64, k0=4, da=A(1), zsrc=A(2), coef=A(3), relu=1, wT=A(4), u8=A(5), w0=A(6), b0=A(7), scale0=A(8),
                    shift0=A(9), mean0=A(10), var0=A(11), eps=1e-3, relu0=1, sums=A(12), ug=A(13), tail=None)
ASM_LINEAR = dict(rows=128, c0=64, cout=64, geo=A(1), P=A(2), wx=A(3), in_scale=A(4), in_shift=A(5), in_bn=None, in_relu=1, w=A(6),
                  bias=A(7), z=A(8), stats=A(9))
ASM_DGRAD = dict(rows=128, c=64, cout=64, da=A(1), zsrc=A(2), coef=A(3), relu=1, wT=A(4), da_prev=A(5), geo=A(6), P=A(7), wx=A(8),
                 scale_prev=A(9), shift_prev=A(10), mean_prev=A(11), var_prev=A(12), eps=1e-3, relu_prev=1, sums=A(13), tail=None)
NARROW_WGRAD = dict(rows=128, k0=4, c0=64, cout=64, u8=A(1), w0=A(2), b0=A(3), in_scale=A(4), in_shift=A(5), in_relu=1, da=A(6), z=A(7),
                    coef=A(8), relu=1)
ASM_WGRAD = dict(rows=128, c0=64, cout=64, geo=A(1), P=A(2), wx=A(3), in_scale=A(4), in_shift=A(5), in_relu=1, da=A(6), z=A(7),
                 coef=A(8), relu=1)
BASE = {
    "votenet_mlp_linear_half": dict(x=A(1), in_scale=A(2), in_shift=A(3), in_relu=1, rows=128, cin=64, cout=64, w=A(4), bias=A(5),
                                    z=A(6), nh_dev=A(7), stream=None),
    "votenet_mlp_dgrad_bn": dict(rows=128, c=64, cout=64, da=A(1), gout=None, argmax=None, pool_k=0, zsrc=A(2), coef=A(3), relu=1,
                                 wT=A(4), da_prev=A(5), stream=None),
    "votenet_mlp_dgrad_bn_half": dict(rows=128, c=64, cout=64, da=A(1), zsrc=A(2), coef=A(3), relu=1, wT=A(4), da_prev=A(5), wh=A(6),
                                      nh_dev=None, stream=None),
    "votenet_mlp_dgrad_bn_reduce": dict(rows=128, c=64, cout=64, da=A(1), zsrc=A(2), coef=A(3), relu=1, wT=A(4), da_prev=A(5),
                                        z_prev=A(6), scale_prev=A(7), shift_prev=A(8), mean_prev=A(9), var_prev=A(10), eps=1e-3,
                                        relu_prev=1, sums=A(11), tail=None, stream=None),
    "votenet_narrow_linear": dict(NARROW_LINEAR, stream=None),
    "votenet_narrow_linear_half": dict(NARROW_LINEAR, wh=A(10), stream=None),
    "votenet_narrow_linear_masked": dict(NARROW_LINEAR, wh=A(10), mask=A(11), stream=None),
    "votenet_narrow_dgrad_bn_reduce": dict(NARROW_DGRAD, stream=None),
    "votenet_narrow_dgrad_bn_reduce_half": dict(NARROW_DGRAD, wh=A(14), stream=None),
    "votenet_narrow_dgrad_bn_reduce_masked": dict(NARROW_DGRAD, tail=("tail", {}), wh=A(14), mask=A(15), stream=None),
    "votenet_assembled_linear": dict(ASM_LINEAR, stream=None),
    "votenet_assembled_linear_half": dict(ASM_LINEAR, wh=A(10), nh_dev=None, stream=None),
    "votenet_assembled_dgrad_bn_reduce": dict(ASM_DGRAD, stream=None),
    "votenet_assembled_dgrad_bn_reduce_half": dict(ASM_DGRAD, wh=A(14), nh_dev=None, stream=None),
    "votenet_narrow_wgrad_bn": dict(NARROW_WGRAD, dw=A(9), scratch=None, stream=None),
    "votenet_narrow_wgrad_bn_half": dict(NARROW_WGRAD, wh=A(10), dw=A(9), stream=None),
    "votenet_assembled_wgrad_bn": dict(ASM_WGRAD, dw=A(9), scratch=None, stream=None),
    "votenet_assembled_wgrad_bn_half": dict(ASM_WGRAD, wh=A(10), dw=A(9), nh_dev=None, stream=None),
}

POOLED = dict(da=None, gout=A(6), argmax=A(7), pool_k=32)  # votenet_mlp_dgrad_bn's other accepted source
NARROW_SHAPES = [dict(rows=0), dict(k0=2), dict(k0=9), dict(c0=0), dict(cout=0)]
NARROW_DGRAD_SHAPES = [dict(rows=0), dict(c=0), dict(c0=0), dict(k0=2), dict(k0=9)]
NO_FIRST_BN = [dict(in_scale=None), dict(in_shift=None)]  # in_bn is NULL in every accepted list above
BELOW = nulls("scale_prev", "shift_prev", "mean_prev", "var_prev", "sums")
FIRST = nulls("scale0", "shift0", "mean0", "var0", "sums", "ug")

# entry -> [(the text of votenet_last_error(), [one-fault overrides of the accepted list, each refused with that text])]
CHECKS = {
    "votenet_mlp_linear_half": [
        ("mlp_linear_half: bad arguments", [dict(rows=0), dict(cin=0), dict(cout=0)] + nulls("x", "w", "z", "nh_dev")),
        ("mlp_linear_half: in_scale and in_shift go together", nulls("in_scale", "in_shift")),
    ],
    "votenet_mlp_dgrad_bn": [
        ("mlp_dgrad_bn expects rows > 0, c > 0, cout > 0", [dict(rows=0), dict(c=0), dict(cout=0)]),
        ("mlp_dgrad_bn: exactly one of da / gout", [dict(da=None), dict(POOLED, da=A(1))]),
        ("mlp_dgrad_bn: null buffer", nulls("zsrc", "coef", "wT", "da_prev") + [dict(POOLED, zsrc=None)]),
        ("mlp_dgrad_bn: pooled source needs argmax and k", [dict(POOLED, argmax=None), dict(POOLED, pool_k=0), dict(POOLED, pool_k=48)]),
    ],
    "votenet_mlp_dgrad_bn_half": [
        ("mlp_dgrad_bn_half expects rows > 0, c > 0, cout > 0", [dict(rows=0), dict(c=0), dict(cout=0)]),
        ("mlp_dgrad_bn_half: null buffer", nulls("da", "zsrc", "coef", "wT", "da_prev", "wh")),
    ],
    "votenet_mlp_dgrad_bn_reduce": [
        ("mlp_dgrad_bn_reduce: incomplete coefficient tail", BAD_TAILS),
        ("mlp_dgrad_bn_reduce expects rows > 0, c > 0, cout > 0", [dict(rows=0), dict(c=0), dict(cout=0)]),
        ("mlp_dgrad_bn_reduce: null buffer", nulls("da", "zsrc", "coef", "wT", "da_prev")),
        ("mlp_dgrad_bn_reduce: null buffer of the layer below", nulls("z_prev") + BELOW),
    ],
    "votenet_narrow_linear": [
        ("narrow_linear expects rows > 0, 3 <= k0 <= 8, c0 > 0, cout > 0", NARROW_SHAPES),
        ("narrow_linear: null buffer", nulls("u8", "w0", "w", "z")),
        ("narrow_linear: the first layer's BatchNorm is missing", NO_FIRST_BN),
    ],
    "votenet_narrow_linear_half": [  # the shared checks answer with the plain entry's name
        ("narrow_linear_half: null weights / rows % 128 != 0", [dict(wh=None), dict(rows=64)]),
        ("narrow_linear expects rows > 0, 3 <= k0 <= 8, c0 > 0, cout > 0", NARROW_SHAPES),
        ("narrow_linear: null buffer", nulls("u8", "w0", "w", "z")),
        ("narrow_linear: the first layer's BatchNorm is missing", NO_FIRST_BN),
    ],
    "votenet_narrow_linear_masked": [
        ("narrow_linear_masked: null mask / c0 % 64 != 0 / rows % 128 != 0", [dict(mask=None), dict(c0=32), dict(rows=64)]),
        ("narrow_linear expects rows > 0, 3 <= k0 <= 8, c0 > 0, cout > 0", NARROW_SHAPES),
        ("narrow_linear: null buffer", nulls("u8", "w0", "w", "z")),
        ("narrow_linear: the first layer's BatchNorm is missing", NO_FIRST_BN),
        ("narrow_linear: the mask must be 8-byte aligned", [dict(mask=A(11) + 4)]),
    ],
    "votenet_narrow_dgrad_bn_reduce": [
        ("narrow_dgrad_bn_reduce: incomplete coefficient tail", BAD_TAILS),
        ("narrow_dgrad_bn_reduce expects rows > 0, c > 0, c0 > 0, 3 <= k0 <= 8", NARROW_DGRAD_SHAPES),
        ("narrow_dgrad_bn_reduce: null buffer", nulls("da", "zsrc", "coef", "wT", "u8", "w0")),
        ("narrow_dgrad_bn_reduce: null buffer of the first layer", FIRST),
    ],
    "votenet_narrow_dgrad_bn_reduce_half": [
        ("narrow_dgrad_bn_reduce_half: null weights", [dict(wh=None)]),
        ("narrow_dgrad_bn_reduce: incomplete coefficient tail", BAD_TAILS),
        ("narrow_dgrad_bn_reduce expects rows > 0, c > 0, c0 > 0, 3 <= k0 <= 8", NARROW_DGRAD_SHAPES),
        ("narrow_dgrad_bn_reduce: null buffer", nulls("da", "zsrc", "coef", "wT", "u8", "w0")),
        ("narrow_dgrad_bn_reduce: null buffer of the first layer", FIRST),
    ],
    "votenet_narrow_dgrad_bn_reduce_masked": [
        ("narrow_dgrad_bn_reduce_masked: null mask", [dict(mask=None)]),
        ("narrow_dgrad_bn_reduce: incomplete coefficient tail", BAD_TAILS),
        ("narrow_dgrad_bn_reduce expects rows > 0, c > 0, c0 > 0, 3 <= k0 <= 8", NARROW_DGRAD_SHAPES),
        ("narrow_dgrad_bn_reduce: null buffer", nulls("da", "zsrc", "coef", "wT", "u8", "w0")),
        ("narrow_dgrad_bn_reduce: null buffer of the first layer", FIRST),
        ("narrow_dgrad_bn_reduce_masked needs the coefficient tail, the piece layout's weights, c0 % 64 == 0 and an 8-byte aligned mask",
         [dict(tail=None), dict(wh=None), dict(c0=32), dict(mask=A(15) + 4)]),
    ],
    "votenet_assembled_linear": [
        ("assembled_linear expects rows > 0, c0 > 0, cout > 0", [dict(rows=0), dict(c0=0), dict(cout=0)]),
        ("assembled_linear: null buffer", nulls("geo", "P", "wx", "w", "z")),
        ("assembled_linear: the first layer's BatchNorm is missing", NO_FIRST_BN),
    ],
    "votenet_assembled_linear_half": [
        ("assembled_linear_half expects rows > 0, c0 > 0, cout > 0", [dict(rows=0), dict(c0=0), dict(cout=0)]),
        ("assembled_linear_half: null buffer", nulls("geo", "P", "wx", "w", "z", "wh")),
        ("assembled_linear_half: the first layer's BatchNorm is missing", NO_FIRST_BN),
    ],
    "votenet_assembled_dgrad_bn_reduce": [
        ("assembled_dgrad_bn_reduce expects rows > 0, c > 0, cout > 0", [dict(rows=0), dict(c=0), dict(cout=0)]),
        ("assembled_dgrad_bn_reduce: null buffer", nulls("da", "zsrc", "coef", "wT", "da_prev", "geo", "P", "wx")),
        ("assembled_dgrad_bn_reduce: null buffer of the layer below", BELOW),
        ("assembled_dgrad_bn_reduce: incomplete coefficient tail", BAD_TAILS),
        ("assembled_dgrad_bn_reduce: geo must be 16-byte aligned", [dict(geo=A(6) + 8)]),
    ],
    "votenet_assembled_dgrad_bn_reduce_half": [
        ("assembled_dgrad_bn_reduce_half expects rows > 0, c > 0, cout > 0", [dict(rows=0), dict(c=0), dict(cout=0)]),
        ("assembled_dgrad_bn_reduce_half: null buffer", nulls("da", "zsrc", "coef", "wT", "da_prev", "geo", "P", "wx", "wh")),
        ("assembled_dgrad_bn_reduce_half: null buffer of the layer below", BELOW),
        ("assembled_dgrad_bn_reduce_half: incomplete coefficient tail", BAD_TAILS),
        ("assembled_dgrad_bn_reduce_half: geo must be 16-byte aligned", [dict(geo=A(6) + 8)]),
    ],
    "votenet_narrow_wgrad_bn": [
        ("narrow_wgrad_bn: bad shape", [dict(rows=0), dict(rows=1 << 31), dict(k0=2), dict(k0=9), dict(c0=0), dict(cout=0)]),
        ("narrow_wgrad_bn: null buffer", nulls("u8", "w0", "in_scale", "in_shift", "da", "z", "coef", "dw")),
    ],
    "votenet_narrow_wgrad_bn_half": [
        ("narrow_wgrad_bn_half: bad shape", [dict(rows=0), dict(rows=48), dict(rows=1 << 31), dict(k0=2), dict(k0=9), dict(c0=0), dict(cout=0)]),
        ("narrow_wgrad_bn_half: null buffer", nulls("u8", "w0", "in_scale", "in_shift", "da", "z", "coef", "wh", "dw")),
    ],
    "votenet_assembled_wgrad_bn": [
        ("assembled_wgrad_bn: bad shape", [dict(rows=0), dict(rows=1 << 31), dict(c0=0), dict(cout=0)]),
        ("assembled_wgrad_bn: null buffer", nulls("geo", "P", "wx", "in_scale", "in_shift", "da", "z", "coef", "dw")),
    ],
    "votenet_assembled_wgrad_bn_half": [
        ("assembled_wgrad_bn_half: bad shape", [dict(rows=0), dict(rows=48), dict(rows=1 << 31), dict(c0=0), dict(cout=0)]),
        ("assembled_wgrad_bn_half: null buffer", nulls("geo", "P", "wx", "in_scale", "in_shift", "da", "z", "coef", "wh", "dw")),
    ],
}

CASES = [pytest.param(entry, over, text, id="%s-%s" % (entry[len("votenet_"):], ",".join("%s=%s" % (k, v[1] if isinstance(v, tuple) else v)
                                                                                        for k, v in over.items())))
         for entry, checks in CHECKS.items() for text, overs in checks for over in overs]


def test_every_entry_has_its_rows():
    assert set(CHECKS) == set(BASE)


@pytest.mark.parametrize("entry,over,text", CASES)
def test_one_fault_is_refused_with_its_text(hiplib, entry, over, text):
    fn = getattr(hiplib, entry)
    args = dict(BASE[entry])
    assert set(over) <= set(args), "the override names an argument the entry does not have"
    args.update(over)
    assert len(args) == len(fn.argtypes), "the accepted list does not match the prototype"
    keep = [_tail(**v[1]) if isinstance(v, tuple) else v for v in args.values()]  # the structs stay alive over the call
    rc = fn(*[ctypes.byref(v) if isinstance(v, ctypes.Structure) else v for v in keep])
    assert rc == 1, "not refused as an invalid argument"
    assert hiplib.votenet_last_error() == text.encode()
