"""CPU: the launch script of every arm of the backward chain (pointnet2.mlp_chain_backward and SAModule's first-layer backward).
Real layers on a CPU store, hand-built records of tiny tagged tensors, and recording stand-ins for every votenet_amd.mlp wrapper the
backward pass calls: each case states outright which launches its arm issues on the main chain and which on the weight-gradient
lane, with which tensors in which argument.  (That the launches add up to the right gradient is what the GPU suite pins.)"""
import pytest
import torch

from votenet_amd import mlp as M
from votenet_amd import pointnet2 as P

ROWS = 128  # one 128-row tile: the fused kernels' shape predicates (kept real) accept it; widths 32 / 64 pass them, 48 does not
B, N, NPOINT, K = 1, 32, 8, 16  # an SA level with B * NPOINT * K = ROWS grouped rows


class _T(torch.Tensor):
    pass


_TAGGED = {}  # storage address -> the tagged tensor that owns it (kept alive while a case runs): names the views of one


def T(tag, *shape, dtype=torch.float32):
    t = torch.zeros(shape, dtype=dtype).as_subclass(_T)
    t.tag = tag
    _TAGGED[t.untyped_storage().data_ptr()] = t
    return t


class _Half:
    """Stand-in of a resolved mlp.HalfLayout: passed through to the wrappers, G centres."""
    tag, G = "half", B * NPOINT


class Rig:
    """The stand-ins, the store they name parameters from, and the script they record."""

    def __init__(self, monkeypatch):
        self.store = P.ParamStore(torch.device("cpu"))
        self.log, self.count, self.called, self.installed = [], {}, set(), set()
        _TAGGED.clear()
        self.fresh = {}  # storage address -> (name, tensor) of a buffer the code under test allocated itself
        self._dims = lambda t: "x".join(str(d) for d in t.shape)
        S = lambda a: (B, N, a.shape[1])  # the scatter to the points, on the first layer's output width
        outs = {
            "bn_backward_reduce": lambda z, *a, **k: self.out("coef", 3 * z.shape[1]),
            "bn_backward_reduce_pool": lambda gout, *a, **k: self.out("coef", 3 * gout.shape[1]),
            "bn_backward_apply": lambda z, *a, **k: self.out("dz", *z.shape),
            "pool_dgrad_prepare": lambda w, *a: self.out("mm", w.shape[0] + 1, w.shape[0]),
            "pool_dgrad": lambda x, *a, below=None, **k: self.out("da", *x.shape) if below is None else
            (self.out("da", *x.shape), self.out("coef_below", 3 * x.shape[1])),
            "pool_wgrad": None, "gram": lambda x, *a, **k: self.out("G", x.shape[1] + 1, x.shape[1]),
            "dgrad_bn": lambda z, coef, relu, wT, below=None, **k: self.out("da", z.shape[0], wT.shape[1]) if below is None else
            (self.out("da", z.shape[0], wT.shape[1]), self.out("coef_below", 3 * wT.shape[1])),
            "dgrad_bn_half": lambda z, coef, relu, wT, da, half: self.out("da", z.shape[0], wT.shape[1]),
            "assembled_dgrad_bn_reduce": lambda z, coef, relu, wT, *a, **k: (self.out("da", z.shape[0], wT.shape[1]),
                                                                             self.out("coef_below", 3 * wT.shape[1])),
            "assembled_wgrad_bn": None, "narrow_wgrad_bn": None, "narrow_wgrad_first": None,
            "narrow_dgrad_bn_reduce": lambda z, coef, relu, wT, *a, **k: (self.out("coef_below", 3 * wT.shape[1]), self.out("ug", 8, wT.shape[1])),
            "wgrad_dense_bn": None, "wgrad_dense": None, "wgrad_gather": None, "bias_grad": None, "row_segments": None,
            "linear_dense": lambda x, w, *a, **k: (self.out("z", x.shape[0], w.shape[1]), None),
            "_zeros_f32": lambda shape, device: self.out("scratch", *shape),
            "group_linear_backward": lambda xyz, new_xyz, idx, cnt, z, *a, want_dz=False: (
                self.out("S", *S(z)), self.out("dz", *z.shape) if want_dz else None),
            "group_linear_backward_assembled": lambda xyz, new_xyz, idx, cnt, Pt, *a, want_dz=False: (
                self.out("S", *S(Pt)), self.out("dz", ROWS, Pt.shape[1]) if want_dz else None),
            "group_linear_backward_half": lambda half, b, n, Pt, *a: self.out("S", *S(Pt)),
            "group_linear_backward_decomposed": lambda half, b, n, Pt, *a, **k: (self.out("S", *S(Pt)), self.out("coef", 3 * Pt.shape[1])),
            "group_concat_grad": lambda df, dx, idx, cnt, n, c: (
                self.out("d_feat", B, n, c) if df is not None else None, self.out("d_xyz", B, n, 3) if dx is not None else None,
                self.out("d_new", B, idx.shape[1], 3) if dx is not None else None),
            "rows_dot3": lambda dz, w3: self.out("d3", dz.shape[0], 3),
            "half_centre_sums": lambda half, Pt, *a: self.out("sums", half.G, Pt.shape[1]),
            "sa_pool_grad": lambda g, k, c, *a, **kw: self.out("dy", g.shape[0] * k, c),
            "sa_pool_weights_grad": lambda xyz, *a: self.out("dv", ROWS, 3),
        }
        for name, make in outs.items():
            self.install(monkeypatch, P.M, name, make)
        # new_xyz = gather(xyz, fps_idx): its gradient is accumulated into the points' (`into`)
        self.install(monkeypatch, P.tf_sampling, "gather_point_grad_raw", lambda n, fps, d_new, into=None: into)
        # the per-step copies of the parameters (W^T, padded copies): tagged, so that a script says which copy a GEMM was given
        def copy_of(fmt, shape_of):
            def f(store, name, *a, **k):
                return T(fmt(name, *a, **k), *shape_of(store.views[name], *a, **k))
            return f
        rng = lambda lo, hi: "" if (lo, hi) == (0, None) else "[%s:%s]" % (lo or "", "" if hi is None else hi)
        monkeypatch.setattr(P.ParamStore, "transposed", copy_of(lambda nm, lo=0, hi=None: "%s%s^T" % (nm, rng(lo, hi)),
                                                                lambda w, lo=0, hi=None: w[lo:hi].t().shape))
        monkeypatch.setattr(P.ParamStore, "padded", copy_of(lambda nm, pad, transpose=False: "[%s|0]%s" % (nm, "^T" * transpose),
                                                            lambda w, pad, transpose=False: (pad, w.shape[0]) if transpose else (w.shape[0], pad)))
        monkeypatch.setattr(P.ParamStore, "padded_rows", copy_of(lambda nm, pad, transpose=False: "[%s;0]%s" % (nm, "^T" * transpose),
                                                                 lambda w, pad, transpose=False: (w.shape[1], pad) if transpose else (pad, w.shape[1])))

    def install(self, monkeypatch, module, name, make):
        assert callable(getattr(module, name))  # a stand-in stands in for something

        def stand_in(*args, **kwargs):
            self.called.add(name)
            self.count[name] = self.count.get(name, 0) + 1
            self._fn = name if self.count[name] == 1 else "%s%d" % (name, self.count[name])
            said = [self.say(a) for a in args] + ["%s=%s" % (k, self.say(v)) for k, v in kwargs.items()]
            self.log.append("%s(%s)" % (name, ", ".join(said)))
            return make(*args, **kwargs) if make is not None else None
        self.installed.add(name)
        monkeypatch.setattr(module, name, stand_in)

    def out(self, what, *shape):
        """A result of the stand-in running now: tagged <wrapper><nth call, from the second on>.<what>."""
        return T("%s.%s" % (self._fn, what), *shape)

    def say(self, v):
        """An argument as the script shows it: a tensor by its tag (a view of one: tag[shape@offset]), a parameter or its gradient by
        the store's name, a buffer the code under test allocated as new<n>[shape@offset], scalars as they are."""
        if isinstance(v, (tuple, list)):
            return "(%s)" % ", ".join(self.say(x) for x in v)
        if isinstance(v, torch.device):
            return "dev"
        if not isinstance(v, torch.Tensor):
            return getattr(v, "tag", None) or ("<fn>" if callable(v) else repr(v))
        if getattr(v, "tag", None):
            return v.tag
        where = lambda t, lo: "[%s@%d]" % (self._dims(t), t.storage_offset() - lo)
        base = _TAGGED.get(v.untyped_storage().data_ptr())
        if base is not None:
            return base.tag + where(v, base.storage_offset())
        st = self.store
        for buf, fmt in ((st.flat, "%s"), (st.grad, "d(%s)")):
            if buf is not None and v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr():
                for name, w in st.views.items():
                    lo = w.storage_offset()
                    if lo <= v.storage_offset() < lo + w.numel():
                        return fmt % name + ("" if (v.storage_offset() == lo and v.shape == w.shape) else where(v, lo))
        name, _ = self.fresh.setdefault(v.untyped_storage().data_ptr(), ("new%d" % (len(self.fresh) + 1), v))
        return name + where(v, 0)

    def script(self, run):
        """run() under a capturing lane: -> the main chain's launches, then per thunk 'lane <- what it reads' and its launches, then
        '-> the result' (a first-layer hand-over by its name and exactly the fields that are set)."""
        deferred = []
        with P.WGRAD.capturing(keep=[], defer=deferred):
            res = run()
        for fn, tensors in deferred:
            self.log.append("lane <- " + ", ".join(self.say(t) for t in tensors))
            fn()
        self.log.append("-> " + (hand_over(self, res) if isinstance(res, P.FirstLayerGrad) else self.say(res)))
        return self.log


SWITCHES = (((P, "PRE_LINEAR"), True), ((P, "FUSE_BN_REDUCE"), True), ((P, "ASSEMBLED_DECOMPOSED"), True), ((P, "WGRAD_BATCH"), False),
            ((M, "NARROW_MASK"), True))  # the defaults the scripts are stated for; a case flips its own


@pytest.fixture
def rig(monkeypatch):
    for name, default in SWITCHES:
        monkeypatch.setattr(*name, default)
    return Rig(monkeypatch)


def hand_over(rig, h):
    """The first-layer hand-over as the cases state it: the record's name and exactly the fields that are set."""
    assert type(h) is P.FirstLayerGrad and h._fields == ("dz", "da", "coef", "relu", "bn", "tail")
    return "FirstLayerGrad(%s)" % ", ".join("%s=%s" % (k, rig.say(v)) for k, v in h._asdict().items() if v is not None)


# ---- records by hand
def bn_of(tag, c):
    return dict(scale=T("scale" + tag, c), shift=T("shift" + tag, c), mean=T("mean" + tag, c), var=T("var" + tag, c))


def dense_recs(layers, x0, below=None):
    """Records of a dense chain as mlp_chain_forward leaves them: layer i reads the raw z of layer i - 1 (the same object).
    below: the first layer's record, when another form (gather, narrow, assembled) made it."""
    recs, x = [], x0
    for i, L in enumerate(layers, 0 if below is None else 1):
        prev = recs[-1] if recs else below
        r = dict(layer=L, kind="dense", x=x, in_scale=prev["scale"] if prev and prev["layer"].bn else None,
                 in_shift=prev["shift"] if prev and prev["layer"].bn else None, in_relu=bool(prev and prev["layer"].relu),
                 z=T("z%d" % i, ROWS, L.cout), rows=ROWS, pool=None)
        if L.bn:
            r.update(bn_of(str(i), L.cout))
        recs.append(r)
        x = r["z"]
    return recs


def chain(rig, cin, widths, last_plain=False, x0=None):
    layers = P.make_mlp(rig.store, "m", cin, widths, "fc", last_plain=last_plain)
    rig.store.materialize(0)
    return dense_recs(layers, T("x", ROWS, cin) if x0 is None else x0)


def gram_form(r, half=None):
    """The pooled last record in Gram form: its z is neither stored nor read."""
    r.update(gram_form=True, z=None, in_affine=T("affine", 4, r["x"].shape[1]), cout=r["layer"].cout, half=half)
    return r


def pooled(c):
    """gout, arg-max and selected z of a max over K rows."""
    return T("gout", ROWS // K, c), T("argmax", ROWS // K, c, dtype=torch.int32), T("zsel", ROWS // K, c)


def first_layer(layers, form, cin=4, half=None):
    """-> the records of a grouped chain whose first layer has `form`: 'gather' (z0 stored), 'assembled' or 'narrow' (never stored;
    the second record then says so)."""
    L0 = layers[0]
    geom = dict(xyz=T("xyz", B, N, 3), new_xyz=T("new_xyz", B, NPOINT, 3), feat=T("feat", B, N, cin) if cin else None,
                idx=T("idx", B, NPOINT, K, dtype=torch.int32))
    r0 = dict(layer=L0, kind=form, rows=ROWS, pool=None, z=None, **bn_of("0", L0.cout))
    if form == "gather":
        r0.update(geom, z=T("z0", ROWS, L0.cout))
    elif form == "assembled":
        r0.update(geom, geo=T("geo", ROWS, 4), P=T("P", B * N, L0.cout), wx=L0.p("W")[:3], half=half, cntv=T("cntv", B * N, 4), mom=T("mom", 16))
    else:
        r0.update(u8=T("u8", ROWS, 8), mom=T("mom", 64), half=half)
    rest = dense_recs(layers[1:], r0["z"], below=r0)
    if form == "assembled":
        rest[0].update(assembled=True, half=half)
    elif form == "narrow":
        rest[0].update(narrow=True, half=half, mask0=T("mask0", ROWS, 4, dtype=torch.int16))
    return [r0] + rest


def grouped_chain(rig, form, widths, cin=4, half=None):
    layers = P.make_mlp(rig.store, "m", 3 + cin, widths, "fc")
    rig.store.materialize(0)
    return first_layer(layers, form, cin, half)


def sa_level(rig, form, widths, cin=4, half=None, pooling="max"):
    """An SA module and its tape record by hand: the first layer in `form`, the last one pooled (max: in Gram form)."""
    sa = P.SAModule(rig.store, "sa", NPOINT, 0.4, K, cin, widths, pooling=pooling)
    rig.store.materialize(0)
    recs = first_layer(sa.mlp, form, cin, half)
    r0, c = recs[0], widths[-1]
    tape = dict(op="sa", module=sa, recs=recs, recs2=[], argmax=T("argmax", B * NPOINT, c, dtype=torch.int32), zsel=None,
                fps_idx=T("fps_idx", B, NPOINT, dtype=torch.int32), idx=r0.get("idx"), pts_cnt=T("pts_cnt", B, NPOINT, dtype=torch.int32),
                xyz=r0.get("xyz"), points=r0.get("feat"), new_xyz=r0.get("new_xyz"), b=B)
    if pooling == "max":
        gram_form(recs[-1], half)
        tape["zsel"] = T("zsel", B * NPOINT, c)
    else:
        tape.update(m=NPOINT, k=K, weights=T("weights", ROWS))
    return sa, tape, T("g_out", B, NPOINT, c)


CASES = []


def case(f):
    CASES.append(f)
    return f


# ---- the pooled last layer in Gram form
@case
def gram_below_batchnormed(rig):
    recs = chain(rig, 64, [64, 64])
    gram_form(recs[1])
    gout, argmax, zsel = pooled(64)
    return rig.script(lambda: P.mlp_chain_backward(recs, gout, "pool", argmax=argmax, k=K, zsel=zsel)), [
        'bn_backward_reduce_pool(gout, zsel, scale1, shift1, mean1, var1, True, tail=(128, m/fc1/gamma, d(m/fc1/gamma), d(m/fc1/beta)))',
        'pool_dgrad_prepare(m/fc1/W, m/fc1/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z0, scale0, shift0, True, m/fc1/W, m/fc1/b, m/fc1/W^T, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'below=(scale0, shift0, mean0, var0, True), mm=pool_dgrad_prepare.mm, below_tail=(128, m/fc0/gamma, d(m/fc0/gamma), '
        'd(m/fc0/beta)), half=None)',
        'dgrad_bn(z0, pool_dgrad.coef_below, True, m/fc0/W^T, da=pool_dgrad.da)',
        'lane <- z0, affine, bn_backward_reduce_pool.coef, gout, argmax, zsel',
        'gram(z0, affine[2x64@0], True, half=None)',
        'pool_wgrad(z0, scale0, shift0, True, gram.G, m/fc1/W, m/fc1/b, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'd(m/fc1/W), half=None)',
        'lane <- x, z0, pool_dgrad.coef_below, pool_dgrad.da',
        'wgrad_dense_bn(x, z0, pool_dgrad.coef_below, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=pool_dgrad.da)',
        '-> dgrad_bn.da',
    ]


@case
def gram_below_plain(rig):
    layers = [P.Layer(rig.store, "m/fc0", 64, 64, bn=False, relu=False), P.Layer(rig.store, "m/fc1", 64, 64)]
    rig.store.materialize(0)
    recs = dense_recs(layers, T("x", ROWS, 64))
    gram_form(recs[1])
    gout, argmax, zsel = pooled(64)
    return rig.script(lambda: P.mlp_chain_backward(recs, gout, "pool", argmax=argmax, k=K, zsel=zsel)), [
        'bn_backward_reduce_pool(gout, zsel, scale1, shift1, mean1, var1, True, tail=(128, m/fc1/gamma, d(m/fc1/gamma), d(m/fc1/beta)))',
        'pool_dgrad_prepare(m/fc1/W, m/fc1/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z0, None, None, False, m/fc1/W, m/fc1/b, m/fc1/W^T, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'mm=pool_dgrad_prepare.mm, half=None)',
        'linear_dense(pool_dgrad.da, m/fc0/W^T, want_stats=False)',
        'lane <- z0, affine, bn_backward_reduce_pool.coef, gout, argmax, zsel',
        'gram(z0, affine[2x64@0], False, half=None)',
        'pool_wgrad(z0, None, None, False, gram.G, m/fc1/W, m/fc1/b, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'd(m/fc1/W), half=None)',
        'lane <- pool_dgrad.da',
        'bias_grad(pool_dgrad.da, d(m/fc0/b))',
        'lane <- pool_dgrad.da, x',
        'wgrad_dense(x, pool_dgrad.da, d(m/fc0/W), None, None, False)',
        '-> linear_dense.z',
    ]


@case
def gram_one_layer_no_input_grad(rig):
    recs = chain(rig, 64, [64])
    gram_form(recs[0])
    gout, argmax, zsel = pooled(64)
    return rig.script(lambda: P.mlp_chain_backward(recs, gout, "pool", argmax=argmax, k=K, need_input_grad=False, zsel=zsel)), [
        'bn_backward_reduce_pool(gout, zsel, scale0, shift0, mean0, var0, True, tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)))',
        'lane <- x, affine, bn_backward_reduce_pool.coef, gout, argmax, zsel',
        'gram(x, affine[2x64@0], False, half=None)',
        'pool_wgrad(x, None, None, False, gram.G, m/fc0/W, m/fc0/b, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'd(m/fc0/W), half=None)',
        '-> None',
    ]


@case
def gram_one_layer_with_input_grad(rig):
    recs = chain(rig, 64, [64])
    gram_form(recs[0])
    gout, argmax, zsel = pooled(64)
    return rig.script(lambda: P.mlp_chain_backward(recs, gout, "pool", argmax=argmax, k=K, zsel=zsel)), [
        'bn_backward_reduce_pool(gout, zsel, scale0, shift0, mean0, var0, True, tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)))',
        'pool_dgrad_prepare(m/fc0/W, m/fc0/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(x, None, None, False, m/fc0/W, m/fc0/b, m/fc0/W^T, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'mm=pool_dgrad_prepare.mm, half=None)',
        'lane <- x, affine, bn_backward_reduce_pool.coef, gout, argmax, zsel',
        'gram(x, affine[2x64@0], False, half=None)',
        'pool_wgrad(x, None, None, False, gram.G, m/fc0/W, m/fc0/b, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'd(m/fc0/W), half=None)',
        '-> pool_dgrad.da',
    ]


@case
def gram_launched_ahead(rig):
    recs = chain(rig, 64, [64])
    gram_form(recs[0])["gram_ahead"] = T("gram_ahead", 65, 64)
    gout, argmax, zsel = pooled(64)
    deferred = []
    with P.WGRAD.capturing(keep=[], defer=deferred):
        P.mlp_chain_backward(recs, gout, "pool", argmax=argmax, k=K, need_input_grad=False, zsel=zsel)
    assert "gram_ahead" in recs[0]  # consumed when the lane's thunk runs, not when it is built
    rig.log.clear()
    deferred[0][0]()
    assert "gram_ahead" not in recs[0]
    return rig.log, [
        'pool_wgrad(x, None, None, False, gram_ahead, m/fc0/W, m/fc0/b, bn_backward_reduce_pool.coef, True, gout, argmax, zsel, 16, '
        'd(m/fc0/W), half=None)',
    ]


# ---- the second layer above an assembled / a narrow first layer
def _above_assembled(rig, half):
    recs = grouped_chain(rig, "assembled", [64, 64], half=half)
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 64), "act"))


@case
def assembled_decomposed(rig):
    return _above_assembled(rig, _Half()), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'dgrad_bn_half(z1, bn_backward_reduce.coef, True, m/fc1/W^T, dy, half)',
        'lane <- geo, P, z1, bn_backward_reduce.coef, dy',
        'assembled_wgrad_bn(geo, P, m/fc0/W[3x64@0], scale0, shift0, True, z1, bn_backward_reduce.coef, True, dy, d(m/fc1/W), half=half)',
        '-> FirstLayerGrad(da=dgrad_bn_half.da, relu=True, bn=(scale0, shift0, mean0, var0), tail=(128, m/fc0/gamma, d(m/fc0/gamma), '
        'd(m/fc0/beta)))',
    ]


@case
def assembled_piece_layout_switch_off(rig, monkeypatch):
    monkeypatch.setattr(P, "ASSEMBLED_DECOMPOSED", False)
    return _above_assembled(rig, _Half()), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'assembled_dgrad_bn_reduce(z1, bn_backward_reduce.coef, True, m/fc1/W^T, dy, geo, P, m/fc0/W[3x64@0], (scale0, shift0, mean0, '
        'var0, True), below_tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)), half=half)',
        'lane <- geo, P, z1, bn_backward_reduce.coef, dy',
        'assembled_wgrad_bn(geo, P, m/fc0/W[3x64@0], scale0, shift0, True, z1, bn_backward_reduce.coef, True, dy, d(m/fc1/W), half=half)',
        '-> FirstLayerGrad(da=assembled_dgrad_bn_reduce.da, coef=assembled_dgrad_bn_reduce.coef_below, relu=True)',
    ]


@case
def assembled_full_layout(rig):
    return _above_assembled(rig, None), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'assembled_dgrad_bn_reduce(z1, bn_backward_reduce.coef, True, m/fc1/W^T, dy, geo, P, m/fc0/W[3x64@0], (scale0, shift0, mean0, '
        'var0, True), below_tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)), half=None)',
        'lane <- geo, P, z1, bn_backward_reduce.coef, dy',
        'assembled_wgrad_bn(geo, P, m/fc0/W[3x64@0], scale0, shift0, True, z1, bn_backward_reduce.coef, True, dy, d(m/fc1/W), half=None)',
        '-> FirstLayerGrad(da=assembled_dgrad_bn_reduce.da, coef=assembled_dgrad_bn_reduce.coef_below, relu=True)',
    ]


def _above_narrow(rig):
    recs = grouped_chain(rig, "narrow", [64, 64], half=_Half())
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 64), "act", need_input_grad=False))


@case
def narrow_with_the_mask(rig):
    return _above_narrow(rig), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'narrow_dgrad_bn_reduce(z1, bn_backward_reduce.coef, True, m/fc1/W^T, dy, u8, m/fc0/W, m/fc0/b, (scale0, shift0, mean0, var0, '
        'True), tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)), half=half, mask=mask0)',
        'narrow_wgrad_first(mom, narrow_dgrad_bn_reduce.ug, narrow_dgrad_bn_reduce.coef_below, m/fc0/W, m/fc0/b, d(m/fc0/W))',
        'lane <- u8, z1, bn_backward_reduce.coef, dy',
        'narrow_wgrad_bn(u8, m/fc0/W, m/fc0/b, scale0, shift0, True, z1, bn_backward_reduce.coef, True, dy, d(m/fc1/W), half=half)',
        '-> None',
    ]


@case
def narrow_mask_switched_off(rig, monkeypatch):
    monkeypatch.setattr(M, "NARROW_MASK", False)
    return _above_narrow(rig), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'narrow_dgrad_bn_reduce(z1, bn_backward_reduce.coef, True, m/fc1/W^T, dy, u8, m/fc0/W, m/fc0/b, (scale0, shift0, mean0, var0, '
        'True), tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)), half=half, mask=None)',
        'narrow_wgrad_first(mom, narrow_dgrad_bn_reduce.ug, narrow_dgrad_bn_reduce.coef_below, m/fc0/W, m/fc0/b, d(m/fc0/W))',
        'lane <- u8, z1, bn_backward_reduce.coef, dy',
        'narrow_wgrad_bn(u8, m/fc0/W, m/fc0/b, scale0, shift0, True, z1, bn_backward_reduce.coef, True, dy, d(m/fc1/W), half=half)',
        '-> None',
    ]


# ---- dense BatchNorm'ed layers
def _act_three_layers(rig):
    recs = chain(rig, 64, [64, 64, 32])
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 32), "act"))


@case
def fused_dense_reduce_in_the_epilogue(rig):
    return _act_three_layers(rig), [
        'bn_backward_reduce(z2, scale2, shift2, mean2, var2, True, dy, argmax=None, k=0, tail=(128, m/fc2/gamma, d(m/fc2/gamma), '
        'd(m/fc2/beta)))',
        'dgrad_bn(z2, bn_backward_reduce.coef, True, m/fc2/W^T, da=dy, below=(z1, scale1, shift1, mean1, var1, True), below_tail=(128, '
        'm/fc1/gamma, d(m/fc1/gamma), d(m/fc1/beta)))',
        'dgrad_bn(z1, dgrad_bn.coef_below, True, m/fc1/W^T, da=dgrad_bn.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, m/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)))',
        'dgrad_bn(z0, dgrad_bn2.coef_below, True, m/fc0/W^T, da=dgrad_bn2.da)',
        'lane <- z1, z2, bn_backward_reduce.coef, dy',
        'wgrad_dense_bn(z1, z2, bn_backward_reduce.coef, True, d(m/fc2/W), in_scale=scale1, in_shift=shift1, in_relu=True, da=dy)',
        'lane <- z0, z1, dgrad_bn.coef_below, dgrad_bn.da',
        'wgrad_dense_bn(z0, z1, dgrad_bn.coef_below, True, d(m/fc1/W), in_scale=scale0, in_shift=shift0, in_relu=True, da=dgrad_bn.da)',
        'lane <- x, z0, dgrad_bn2.coef_below, dgrad_bn2.da',
        'wgrad_dense_bn(x, z0, dgrad_bn2.coef_below, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=dgrad_bn2.da)',
        '-> dgrad_bn3.da',
    ]


@case
def fused_dense_reduce_on_its_own(rig, monkeypatch):
    monkeypatch.setattr(P, "FUSE_BN_REDUCE", False)
    return _act_three_layers(rig), [
        'bn_backward_reduce(z2, scale2, shift2, mean2, var2, True, dy, argmax=None, k=0, tail=(128, m/fc2/gamma, d(m/fc2/gamma), '
        'd(m/fc2/beta)))',
        'dgrad_bn(z2, bn_backward_reduce.coef, True, m/fc2/W^T, da=dy)',
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dgrad_bn.da, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'dgrad_bn(z1, bn_backward_reduce2.coef, True, m/fc1/W^T, da=dgrad_bn.da)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, dgrad_bn2.da, argmax=None, k=0, tail=(128, m/fc0/gamma, d(m/fc0/gamma), '
        'd(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce3.coef, True, m/fc0/W^T, da=dgrad_bn2.da)',
        'lane <- z1, z2, bn_backward_reduce.coef, dy',
        'wgrad_dense_bn(z1, z2, bn_backward_reduce.coef, True, d(m/fc2/W), in_scale=scale1, in_shift=shift1, in_relu=True, da=dy)',
        'lane <- z0, z1, bn_backward_reduce2.coef, dgrad_bn.da',
        'wgrad_dense_bn(z0, z1, bn_backward_reduce2.coef, True, d(m/fc1/W), in_scale=scale0, in_shift=shift0, in_relu=True, '
        'da=dgrad_bn.da)',
        'lane <- x, z0, bn_backward_reduce3.coef, dgrad_bn2.da',
        'wgrad_dense_bn(x, z0, bn_backward_reduce3.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=dgrad_bn2.da)',
        '-> dgrad_bn3.da',
    ]


@case
def fused_dense_pooled_not_gram(rig):
    recs = chain(rig, 64, [64, 64])
    gout, argmax, _ = pooled(64)
    return rig.script(lambda: P.mlp_chain_backward(recs, gout, "pool", argmax=argmax, k=K)), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, gout, argmax=argmax, k=16, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'dgrad_bn(z1, bn_backward_reduce.coef, True, m/fc1/W^T, gout=gout, argmax=argmax, k=16)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, dgrad_bn.da, argmax=None, k=0, tail=(128, m/fc0/gamma, d(m/fc0/gamma), '
        'd(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce2.coef, True, m/fc0/W^T, da=dgrad_bn.da)',
        'lane <- z0, z1, bn_backward_reduce.coef, gout, argmax',
        'wgrad_dense_bn(z0, z1, bn_backward_reduce.coef, True, d(m/fc1/W), in_scale=scale0, in_shift=shift0, in_relu=True, gout=gout, '
        'argmax=argmax, k=16)',
        'lane <- x, z0, bn_backward_reduce2.coef, dgrad_bn.da',
        'wgrad_dense_bn(x, z0, bn_backward_reduce2.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=dgrad_bn.da)',
        '-> dgrad_bn2.da',
    ]


@case
def fused_dense_no_input_grad(rig):
    recs = chain(rig, 32, [64])  # (a 32-wide input: only the input-gradient GEMM would refuse it)
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 64), "act", need_input_grad=False)), [
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, dy, argmax=None, k=0, tail=(128, m/fc0/gamma, d(m/fc0/gamma), '
        'd(m/fc0/beta)))',
        'lane <- x, z0, bn_backward_reduce.coef, dy',
        'wgrad_dense_bn(x, z0, bn_backward_reduce.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=dy)',
        '-> None',
    ]


@case
def unfused_width(rig):
    recs = chain(rig, 64, [48, 64])  # 48: neither as c nor as the input width does dgrad_bn_supported take it
    assert not M.dgrad_bn_supported(ROWS, 48, 64) and not M.dgrad_bn_supported(ROWS, 64, 48) and M.dgrad_bn_supported(ROWS, 64, 64)
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 64), "act")), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'bn_backward_apply(z1, bn_backward_reduce.coef, True, dy, argmax=None, k=0)',
        'linear_dense(bn_backward_apply.dz, m/fc1/W^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, m/fc0/gamma, '
        'd(m/fc0/gamma), d(m/fc0/beta)))',
        'bn_backward_apply(z0, bn_backward_reduce2.coef, True, linear_dense.z, argmax=None, k=0)',
        'linear_dense(bn_backward_apply2.dz, m/fc0/W^T, want_stats=False)',
        'lane <- bn_backward_apply.dz, z0',
        'wgrad_dense(z0, bn_backward_apply.dz, d(m/fc1/W), scale0, shift0, True)',
        'lane <- bn_backward_apply2.dz, x',
        'wgrad_dense(x, bn_backward_apply2.dz, d(m/fc0/W), None, None, False)',
        '-> linear_dense2.z',
    ]


@case
def padded_input_width(rig):
    layers = P.make_mlp(rig.store, "m", 70, [64], "fc")
    rig.store.materialize(0)
    assert layers[0].cin_pad == 128
    recs = dense_recs(layers, T("[x|0]", ROWS, 128))
    recs[0]["cin_padded"] = True
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 64), "act")), [
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, dy, argmax=None, k=0, tail=(128, m/fc0/gamma, d(m/fc0/gamma), '
        'd(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce.coef, True, [m/fc0/W;0]^T, da=dy)',
        'lane <- [x|0], z0, bn_backward_reduce.coef, dy',
        '_zeros_f32((128, 64), dev)',
        'wgrad_dense_bn([x|0], z0, bn_backward_reduce.coef, True, _zeros_f32.scratch, da=dy)',
        'row_segments(70, ((d(m/fc0/W), d(m/fc0/W), _zeros_f32.scratch[70x64@0])))',
        '-> dgrad_bn.da[128x70@0]',
    ]


# ---- the plain last layer
@case
def plain_last_layer(rig):
    recs = chain(rig, 64, [64, 64], last_plain=True)
    assert not recs[1]["layer"].cout_pad
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dz", ROWS, 64), "plain")), [
        'linear_dense(dz, m/fc1/W^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, m/fc0/gamma, '
        'd(m/fc0/gamma), d(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce.coef, True, m/fc0/W^T, da=linear_dense.z)',
        'lane <- dz',
        'bias_grad(dz, d(m/fc1/b))',
        'lane <- dz, z0',
        'wgrad_dense(z0, dz, d(m/fc1/W), scale0, shift0, True)',
        'lane <- x, z0, bn_backward_reduce.coef, linear_dense.z',
        'wgrad_dense_bn(x, z0, bn_backward_reduce.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=linear_dense.z)',
        '-> dgrad_bn.da',
    ]


def _plain_padded(rig, g_padded):
    recs = chain(rig, 64, [64, 40], last_plain=True)
    assert recs[1]["layer"].cout_pad == 64
    recs[1].update(padded=True, z=T("[z1|0]", ROWS, 64)[:, :40])
    g = g_padded[:, :40] if g_padded is not None else T("dz", ROWS, 40)
    return rig.script(lambda: P.mlp_chain_backward(recs, g, "plain", g_padded=g_padded))


@case
def plain_padded(rig):
    return _plain_padded(rig, None), [
        'row_segments(128, ((new1[128x40@0], dz, None), (new1[128x24@40], None, None)))',
        'linear_dense(new1[128x64@0], [m/fc1/W|0]^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, m/fc0/gamma, '
        'd(m/fc0/gamma), d(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce.coef, True, m/fc0/W^T, da=linear_dense.z)',
        'lane <- dz',
        'bias_grad(dz, d(m/fc1/b))',
        'lane <- new1[128x64@0], z0',
        '_zeros_f32((64, 64), dev)',
        'wgrad_dense(z0, new1[128x64@0], _zeros_f32.scratch, scale0, shift0, True)',
        'row_segments(64, ((d(m/fc1/W), d(m/fc1/W), _zeros_f32.scratch[64x40@0])))',
        'lane <- x, z0, bn_backward_reduce.coef, linear_dense.z',
        'wgrad_dense_bn(x, z0, bn_backward_reduce.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=linear_dense.z)',
        '-> dgrad_bn.da',
    ]


@case
def plain_padded_gradient_arrives_padded(rig):
    return _plain_padded(rig, T("[dz|0]", ROWS, 64)), [
        'linear_dense([dz|0], [m/fc1/W|0]^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, m/fc0/gamma, '
        'd(m/fc0/gamma), d(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce.coef, True, m/fc0/W^T, da=linear_dense.z)',
        'lane <- [dz|0][128x40@0]',
        'bias_grad([dz|0][128x40@0], d(m/fc1/b))',
        'lane <- [dz|0], z0',
        '_zeros_f32((64, 64), dev)',
        'wgrad_dense(z0, [dz|0], _zeros_f32.scratch, scale0, shift0, True)',
        'row_segments(64, ((d(m/fc1/W), d(m/fc1/W), _zeros_f32.scratch[64x40@0])))',
        'lane <- x, z0, bn_backward_reduce.coef, linear_dense.z',
        'wgrad_dense_bn(x, z0, bn_backward_reduce.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=linear_dense.z)',
        '-> dgrad_bn.da',
    ]


@case
def plain_padded_gradient_of_another_width(rig):
    return _plain_padded(rig, T("[dz|0]", ROWS, 128)), [
        'row_segments(128, ((new1[128x40@0], [dz|0][128x40@0], None), (new1[128x24@40], None, None)))',
        'linear_dense(new1[128x64@0], [m/fc1/W|0]^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, m/fc0/gamma, '
        'd(m/fc0/gamma), d(m/fc0/beta)))',
        'dgrad_bn(z0, bn_backward_reduce.coef, True, m/fc0/W^T, da=linear_dense.z)',
        'lane <- [dz|0][128x40@0]',
        'bias_grad([dz|0][128x40@0], d(m/fc1/b))',
        'lane <- new1[128x64@0], z0',
        '_zeros_f32((64, 64), dev)',
        'wgrad_dense(z0, new1[128x64@0], _zeros_f32.scratch, scale0, shift0, True)',
        'row_segments(64, ((d(m/fc1/W), d(m/fc1/W), _zeros_f32.scratch[64x40@0])))',
        'lane <- x, z0, bn_backward_reduce.coef, linear_dense.z',
        'wgrad_dense_bn(x, z0, bn_backward_reduce.coef, True, d(m/fc0/W), in_scale=None, in_shift=None, in_relu=False, da=linear_dense.z)',
        '-> dgrad_bn.da',
    ]


# ---- the gather first layer: where the chain stops
def _gather_chain(rig, c0):
    recs = grouped_chain(rig, "gather", [c0, 64])
    return rig.script(lambda: P.mlp_chain_backward(recs, T("dy", ROWS, 64), "act"))


@case
def gather_fused(rig):
    return _gather_chain(rig, 64), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'dgrad_bn(z1, bn_backward_reduce.coef, True, m/fc1/W^T, da=dy, below=(z0, scale0, shift0, mean0, var0, True), below_tail=(128, '
        'm/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)))',
        'lane <- z0, z1, bn_backward_reduce.coef, dy',
        'wgrad_dense_bn(z0, z1, bn_backward_reduce.coef, True, d(m/fc1/W), in_scale=scale0, in_shift=shift0, in_relu=True, da=dy)',
        '-> FirstLayerGrad(da=dgrad_bn.da, coef=dgrad_bn.coef_below, relu=True)',
    ]


@case
def gather_width_the_fused_kernel_refuses(rig):
    assert not M.group_linear_backward_supported(48, K) and M.group_linear_backward_supported(64, K)
    return _gather_chain(rig, 48), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'bn_backward_apply(z1, bn_backward_reduce.coef, True, dy, argmax=None, k=0)',
        'linear_dense(bn_backward_apply.dz, m/fc1/W^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, m/fc0/gamma, '
        'd(m/fc0/gamma), d(m/fc0/beta)))',
        'bn_backward_apply(z0, bn_backward_reduce2.coef, True, linear_dense.z, argmax=None, k=0)',
        'lane <- bn_backward_apply.dz, z0',
        'wgrad_dense(z0, bn_backward_apply.dz, d(m/fc1/W), scale0, shift0, True)',
        '-> FirstLayerGrad(dz=bn_backward_apply2.dz)',
    ]


@case
def gather_pre_linear_off(rig, monkeypatch):
    monkeypatch.setattr(P, "PRE_LINEAR", False)
    return _gather_chain(rig, 64), [
        'bn_backward_reduce(z1, scale1, shift1, mean1, var1, True, dy, argmax=None, k=0, tail=(128, m/fc1/gamma, d(m/fc1/gamma), '
        'd(m/fc1/beta)))',
        'dgrad_bn(z1, bn_backward_reduce.coef, True, m/fc1/W^T, da=dy, below=(z0, scale0, shift0, mean0, var0, True), below_tail=(128, '
        'm/fc0/gamma, d(m/fc0/gamma), d(m/fc0/beta)))',
        'bn_backward_apply(z0, dgrad_bn.coef_below, True, dgrad_bn.da, argmax=None, k=0)',
        'lane <- z0, z1, bn_backward_reduce.coef, dy',
        'wgrad_dense_bn(z0, z1, bn_backward_reduce.coef, True, d(m/fc1/W), in_scale=scale0, in_shift=shift0, in_relu=True, da=dy)',
        '-> FirstLayerGrad(dz=bn_backward_apply.dz)',
    ]


# ---- SAModule.backward: the chain, then the first layer's four ways to S and dz and their common tail
def _sa(rig, form, widths, xyz_grad, cin=4, half=None, feat_grad=True, pooling="max"):
    sa, tape, g_out = sa_level(rig, form, widths, cin, half, pooling)
    return rig.script(lambda: sa.backward(tape, g_out, need_feat_grad=feat_grad, need_xyz_grad=xyz_grad))


@case
def sa_written_out_dz_no_features(rig):
    return _sa(rig, "gather", [64, 64, 64], False, cin=0), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'dgrad_bn(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, da=pool_dgrad.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)))',
        'bn_backward_apply(z0, dgrad_bn.coef_below, True, dgrad_bn.da, argmax=None, k=0)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- z0, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'wgrad_dense_bn(z0, z1, pool_dgrad.coef_below, True, d(sa/conv1/W), in_scale=scale0, in_shift=shift0, in_relu=True, '
        'da=pool_dgrad.da)',
        'lane <- bn_backward_apply.dz',
        'wgrad_gather(xyz, new_xyz, None, idx, bn_backward_apply.dz, d(sa/conv0/W))',
        '-> (None, None)',
    ]


@case
def sa_written_out_dz_no_features_xyz(rig):
    return _sa(rig, "gather", [64, 64, 64], True, cin=0), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'dgrad_bn(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, da=pool_dgrad.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)))',
        'bn_backward_apply(z0, dgrad_bn.coef_below, True, dgrad_bn.da, argmax=None, k=0)',
        'rows_dot3(bn_backward_apply.dz, sa/conv0/W)',
        'group_concat_grad(None, rows_dot3.d3, idx, pts_cnt, 32, 0)',
        'gather_point_grad_raw(32, fps_idx, group_concat_grad.d_new, into=group_concat_grad.d_xyz)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- z0, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'wgrad_dense_bn(z0, z1, pool_dgrad.coef_below, True, d(sa/conv1/W), in_scale=scale0, in_shift=shift0, in_relu=True, '
        'da=pool_dgrad.da)',
        'lane <- bn_backward_apply.dz',
        'wgrad_gather(xyz, new_xyz, None, idx, bn_backward_apply.dz, d(sa/conv0/W))',
        '-> (None, group_concat_grad.d_xyz)',
    ]


@case
def sa_written_out_dz_scattered(rig):
    return _sa(rig, "gather", [48, 64, 64], False), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'bn_backward_apply(z1, pool_dgrad.coef_below, True, pool_dgrad.da, argmax=None, k=0)',
        'linear_dense(bn_backward_apply.dz, sa/conv1/W^T, want_stats=False)',
        'bn_backward_reduce(z0, scale0, shift0, mean0, var0, True, linear_dense.z, argmax=None, k=0, tail=(128, sa/conv0/gamma, '
        'd(sa/conv0/gamma), d(sa/conv0/beta)))',
        'bn_backward_apply(z0, bn_backward_reduce.coef, True, linear_dense.z, argmax=None, k=0)',
        'group_concat_grad(bn_backward_apply2.dz, None, idx, pts_cnt, 32, 48)',
        'linear_dense(group_concat_grad.d_feat[32x48@0], sa/conv0/W[3:]^T, want_stats=False)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- bn_backward_apply.dz, z0',
        'wgrad_dense(z0, bn_backward_apply.dz, d(sa/conv1/W), scale0, shift0, True)',
        'lane <- bn_backward_apply2.dz',
        'wgrad_gather(xyz, new_xyz, None, idx, bn_backward_apply2.dz, d(sa/conv0/W))',
        'lane <- group_concat_grad.d_feat[32x48@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_concat_grad.d_feat[32x48@0], d(sa/conv0/W)[4x48@144])',
        '-> (linear_dense2.z[1x32x4@0], None)',
    ]


@case
def sa_written_out_dz_gather_gemms_xyz(rig, monkeypatch):
    monkeypatch.setattr(P, "PRE_LINEAR", False)
    return _sa(rig, "gather", [64, 64, 64], True), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'dgrad_bn(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, da=pool_dgrad.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)))',
        'bn_backward_apply(z0, dgrad_bn.coef_below, True, dgrad_bn.da, argmax=None, k=0)',
        'linear_dense(bn_backward_apply.dz, sa/conv0/W[3:]^T, want_stats=False)',
        'group_concat_grad(linear_dense.z, None, idx, pts_cnt, 32, 4)',
        'rows_dot3(bn_backward_apply.dz, sa/conv0/W[3x64@0])',
        'group_concat_grad(None, rows_dot3.d3, idx, pts_cnt, 32, 0)',
        'gather_point_grad_raw(32, fps_idx, group_concat_grad2.d_new, into=group_concat_grad2.d_xyz)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- z0, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'wgrad_dense_bn(z0, z1, pool_dgrad.coef_below, True, d(sa/conv1/W), in_scale=scale0, in_shift=shift0, in_relu=True, '
        'da=pool_dgrad.da)',
        'lane <- bn_backward_apply.dz, feat',
        'wgrad_gather(xyz, new_xyz, feat, idx, bn_backward_apply.dz, d(sa/conv0/W))',
        '-> (group_concat_grad.d_feat, group_concat_grad2.d_xyz)',
    ]


@case
def sa_piece_layout_decomposed(rig):
    return _sa(rig, "assembled", [64, 64, 64], False, half=_Half()), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=half)',
        'dgrad_bn_half(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, pool_dgrad.da, half)',
        'group_linear_backward_decomposed(half, 1, 32, P, sa/conv0/W[3x64@0], dgrad_bn_half.da, (scale0, shift0, mean0, var0), True, (128, '
        'sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)), cntv, mom, d(sa/conv0/W)[3x64@0], defer=<fn>)',
        'linear_dense(group_linear_backward_decomposed.S[32x64@0], sa/conv0/W[3:]^T, want_stats=False)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=half)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=half)',
        'lane <- geo, P, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'assembled_wgrad_bn(geo, P, sa/conv0/W[3x64@0], scale0, shift0, True, z1, pool_dgrad.coef_below, True, pool_dgrad.da, '
        'd(sa/conv1/W), half=half)',
        'lane <- group_linear_backward_decomposed.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward_decomposed.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (linear_dense.z[1x32x4@0], None)',
    ]


@case
def sa_piece_layout_decomposed_xyz(rig):
    return _sa(rig, "assembled", [64, 64, 64], True, half=_Half()), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=half)',
        'dgrad_bn_half(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, pool_dgrad.da, half)',
        'group_linear_backward_decomposed(half, 1, 32, P, sa/conv0/W[3x64@0], dgrad_bn_half.da, (scale0, shift0, mean0, var0), True, (128, '
        'sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)), cntv, mom, d(sa/conv0/W)[3x64@0], defer=<fn>)',
        'rows_dot3(group_linear_backward_decomposed.S[32x64@0], sa/conv0/W[3x64@0])',
        'half_centre_sums(half, P, sa/conv0/W[3x64@0], dgrad_bn_half.da, group_linear_backward_decomposed.coef, True)',
        'rows_dot3(half_centre_sums.sums, sa/conv0/W[3x64@0])',
        'gather_point_grad_raw(32, fps_idx, rows_dot32.d3[1x8x3@0], into=rows_dot3.d3[1x32x3@0])',
        'linear_dense(group_linear_backward_decomposed.S[32x64@0], sa/conv0/W[3:]^T, want_stats=False)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=half)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=half)',
        'lane <- geo, P, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'assembled_wgrad_bn(geo, P, sa/conv0/W[3x64@0], scale0, shift0, True, z1, pool_dgrad.coef_below, True, pool_dgrad.da, '
        'd(sa/conv1/W), half=half)',
        'lane <- group_linear_backward_decomposed.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward_decomposed.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (linear_dense.z[1x32x4@0], rows_dot3.d3[1x32x3@0])',
    ]


@case
def sa_piece_layout_not_decomposed_xyz(rig, monkeypatch):
    monkeypatch.setattr(P, "ASSEMBLED_DECOMPOSED", False)
    return _sa(rig, "assembled", [64, 64, 64], True, half=_Half(), feat_grad=False), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=half)',
        'assembled_dgrad_bn_reduce(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, pool_dgrad.da, geo, P, sa/conv0/W[3x64@0], (scale0, '
        'shift0, mean0, var0, True), below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)), half=half)',
        'group_linear_backward_half(half, 1, 32, P, sa/conv0/W[3x64@0], assembled_dgrad_bn_reduce.da, '
        'assembled_dgrad_bn_reduce.coef_below, True, d(sa/conv0/W)[3x64@0])',
        'rows_dot3(group_linear_backward_half.S[32x64@0], sa/conv0/W[3x64@0])',
        'half_centre_sums(half, P, sa/conv0/W[3x64@0], assembled_dgrad_bn_reduce.da, assembled_dgrad_bn_reduce.coef_below, True)',
        'rows_dot3(half_centre_sums.sums, sa/conv0/W[3x64@0])',
        'gather_point_grad_raw(32, fps_idx, rows_dot32.d3[1x8x3@0], into=rows_dot3.d3[1x32x3@0])',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=half)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=half)',
        'lane <- geo, P, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'assembled_wgrad_bn(geo, P, sa/conv0/W[3x64@0], scale0, shift0, True, z1, pool_dgrad.coef_below, True, pool_dgrad.da, '
        'd(sa/conv1/W), half=half)',
        'lane <- group_linear_backward_half.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward_half.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (None, rows_dot3.d3[1x32x3@0])',
    ]


@case
def sa_assembled_full_layout(rig):
    return _sa(rig, "assembled", [64, 64, 64], False), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'assembled_dgrad_bn_reduce(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, pool_dgrad.da, geo, P, sa/conv0/W[3x64@0], (scale0, '
        'shift0, mean0, var0, True), below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)), half=None)',
        'group_linear_backward_assembled(xyz, new_xyz, idx, pts_cnt, P, sa/conv0/W[3x64@0], assembled_dgrad_bn_reduce.da, '
        'assembled_dgrad_bn_reduce.coef_below, True, d(sa/conv0/W)[3x64@0], want_dz=False)',
        'linear_dense(group_linear_backward_assembled.S[32x64@0], sa/conv0/W[3:]^T, want_stats=False)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- geo, P, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'assembled_wgrad_bn(geo, P, sa/conv0/W[3x64@0], scale0, shift0, True, z1, pool_dgrad.coef_below, True, pool_dgrad.da, '
        'd(sa/conv1/W), half=None)',
        'lane <- group_linear_backward_assembled.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward_assembled.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (linear_dense.z[1x32x4@0], None)',
    ]


@case
def sa_assembled_full_layout_xyz(rig):
    return _sa(rig, "assembled", [64, 64, 64], True), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'assembled_dgrad_bn_reduce(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, pool_dgrad.da, geo, P, sa/conv0/W[3x64@0], (scale0, '
        'shift0, mean0, var0, True), below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)), half=None)',
        'group_linear_backward_assembled(xyz, new_xyz, idx, pts_cnt, P, sa/conv0/W[3x64@0], assembled_dgrad_bn_reduce.da, '
        'assembled_dgrad_bn_reduce.coef_below, True, d(sa/conv0/W)[3x64@0], want_dz=True)',
        'linear_dense(group_linear_backward_assembled.S[32x64@0], sa/conv0/W[3:]^T, want_stats=False)',
        'rows_dot3(group_linear_backward_assembled.dz, sa/conv0/W[3x64@0])',
        'group_concat_grad(None, rows_dot3.d3, idx, pts_cnt, 32, 0)',
        'gather_point_grad_raw(32, fps_idx, group_concat_grad.d_new, into=group_concat_grad.d_xyz)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- geo, P, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'assembled_wgrad_bn(geo, P, sa/conv0/W[3x64@0], scale0, shift0, True, z1, pool_dgrad.coef_below, True, pool_dgrad.da, '
        'd(sa/conv1/W), half=None)',
        'lane <- group_linear_backward_assembled.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward_assembled.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (linear_dense.z[1x32x4@0], group_concat_grad.d_xyz)',
    ]


@case
def sa_gather_fused(rig):
    return _sa(rig, "gather", [64, 64, 64], False), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'dgrad_bn(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, da=pool_dgrad.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)))',
        'group_linear_backward(xyz, new_xyz, idx, pts_cnt, z0, dgrad_bn.da, dgrad_bn.coef_below, True, d(sa/conv0/W)[3x64@0], '
        'want_dz=False)',
        'linear_dense(group_linear_backward.S[32x64@0], sa/conv0/W[3:]^T, want_stats=False)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- z0, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'wgrad_dense_bn(z0, z1, pool_dgrad.coef_below, True, d(sa/conv1/W), in_scale=scale0, in_shift=shift0, in_relu=True, '
        'da=pool_dgrad.da)',
        'lane <- group_linear_backward.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (linear_dense.z[1x32x4@0], None)',
    ]


@case
def sa_gather_fused_xyz(rig):
    return _sa(rig, "gather", [64, 64, 64], True, feat_grad=False), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=None)',
        'dgrad_bn(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, da=pool_dgrad.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)))',
        'group_linear_backward(xyz, new_xyz, idx, pts_cnt, z0, dgrad_bn.da, dgrad_bn.coef_below, True, d(sa/conv0/W)[3x64@0], '
        'want_dz=True)',
        'rows_dot3(group_linear_backward.dz, sa/conv0/W[3x64@0])',
        'group_concat_grad(None, rows_dot3.d3, idx, pts_cnt, 32, 0)',
        'gather_point_grad_raw(32, fps_idx, group_concat_grad.d_new, into=group_concat_grad.d_xyz)',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=None)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=None)',
        'lane <- z0, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'wgrad_dense_bn(z0, z1, pool_dgrad.coef_below, True, d(sa/conv1/W), in_scale=scale0, in_shift=shift0, in_relu=True, '
        'da=pool_dgrad.da)',
        'lane <- group_linear_backward.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (None, group_concat_grad.d_xyz)',
    ]


@case
def sa_weighted_avg_adds_the_weights_gradient(rig):
    return _sa(rig, "gather", [64, 64, 64], True, pooling="weighted_avg"), [
        "sa_pool_grad(g_out[8x64@0], 16, 64, 'weighted_avg', w=weights, argmax=argmax)",
        'sa_pool_weights_grad(xyz, new_xyz, idx, z2, scale2, shift2, True, g_out[8x64@0], weights)',
        'bn_backward_reduce(z2, scale2, shift2, mean2, var2, True, sa_pool_grad.dy, argmax=None, k=0, tail=(128, sa/conv2/gamma, '
        'd(sa/conv2/gamma), d(sa/conv2/beta)))',
        'dgrad_bn(z2, bn_backward_reduce.coef, True, sa/conv2/W^T, da=sa_pool_grad.dy, below=(z1, scale1, shift1, mean1, var1, True), '
        'below_tail=(128, sa/conv1/gamma, d(sa/conv1/gamma), d(sa/conv1/beta)))',
        'dgrad_bn(z1, dgrad_bn.coef_below, True, sa/conv1/W^T, da=dgrad_bn.da, below=(z0, scale0, shift0, mean0, var0, True), '
        'below_tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)))',
        'group_linear_backward(xyz, new_xyz, idx, pts_cnt, z0, dgrad_bn2.da, dgrad_bn2.coef_below, True, d(sa/conv0/W)[3x64@0], '
        'want_dz=True)',
        'linear_dense(group_linear_backward.S[32x64@0], sa/conv0/W[3:]^T, want_stats=False)',
        'rows_dot3(group_linear_backward.dz, sa/conv0/W[3x64@0])',
        'row_segments(128, ((new1[128x3@0], rows_dot3.d3[128x3@0], sa_pool_weights_grad.dv[128x3@0])))',
        'group_concat_grad(None, new1[128x3@0], idx, pts_cnt, 32, 0)',
        'gather_point_grad_raw(32, fps_idx, group_concat_grad.d_new, into=group_concat_grad.d_xyz)',
        'lane <- z1, z2, bn_backward_reduce.coef, sa_pool_grad.dy',
        'wgrad_dense_bn(z1, z2, bn_backward_reduce.coef, True, d(sa/conv2/W), in_scale=scale1, in_shift=shift1, in_relu=True, '
        'da=sa_pool_grad.dy)',
        'lane <- z0, z1, dgrad_bn.coef_below, dgrad_bn.da',
        'wgrad_dense_bn(z0, z1, dgrad_bn.coef_below, True, d(sa/conv1/W), in_scale=scale0, in_shift=shift0, in_relu=True, da=dgrad_bn.da)',
        'lane <- group_linear_backward.S[32x64@0], feat[32x4@0]',
        'wgrad_dense(feat[32x4@0], group_linear_backward.S[32x64@0], d(sa/conv0/W)[4x64@192])',
        '-> (linear_dense.z[1x32x4@0], group_concat_grad.d_xyz)',
    ]


@case
def sa_narrow_leaf(rig):
    sa, tape, g_out = sa_level(rig, "narrow", [64, 64, 64], cin=0, half=_Half())
    with pytest.raises(ValueError, match="narrow first layer keeps no per-row gradient"):
        sa.backward(tape, g_out, need_xyz_grad=True)
    rig.log.clear()
    rig.count.clear()
    return rig.script(lambda: sa.backward(tape, g_out)), [
        'bn_backward_reduce_pool(g_out[8x64@0], zsel, scale2, shift2, mean2, var2, True, tail=(128, sa/conv2/gamma, d(sa/conv2/gamma), '
        'd(sa/conv2/beta)))',
        'pool_dgrad_prepare(sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, 128)',
        'pool_dgrad(z1, scale1, shift1, True, sa/conv2/W, sa/conv2/b, sa/conv2/W^T, bn_backward_reduce_pool.coef, True, g_out[8x64@0], '
        'argmax, zsel, 16, below=(scale1, shift1, mean1, var1, True), mm=pool_dgrad_prepare.mm, below_tail=(128, sa/conv1/gamma, '
        'd(sa/conv1/gamma), d(sa/conv1/beta)), half=half)',
        'narrow_dgrad_bn_reduce(z1, pool_dgrad.coef_below, True, sa/conv1/W^T, pool_dgrad.da, u8, sa/conv0/W, sa/conv0/b, (scale0, shift0, '
        'mean0, var0, True), tail=(128, sa/conv0/gamma, d(sa/conv0/gamma), d(sa/conv0/beta)), half=half, mask=mask0)',
        'narrow_wgrad_first(mom, narrow_dgrad_bn_reduce.ug, narrow_dgrad_bn_reduce.coef_below, sa/conv0/W, sa/conv0/b, d(sa/conv0/W))',
        'lane <- z1, affine, bn_backward_reduce_pool.coef, g_out[8x64@0], argmax, zsel',
        'gram(z1, affine[2x64@0], True, half=half)',
        'pool_wgrad(z1, scale1, shift1, True, gram.G, sa/conv2/W, sa/conv2/b, bn_backward_reduce_pool.coef, True, g_out[8x64@0], argmax, '
        'zsel, 16, d(sa/conv2/W), half=half)',
        'lane <- u8, z1, pool_dgrad.coef_below, pool_dgrad.da',
        'narrow_wgrad_bn(u8, sa/conv0/W, sa/conv0/b, scale0, shift0, True, z1, pool_dgrad.coef_below, True, pool_dgrad.da, d(sa/conv1/W), '
        'half=half)',
        '-> (None, None)',
    ]


def _run(f, rig, monkeypatch):
    return f(rig, monkeypatch) if f.__code__.co_argcount == 2 else f(rig)


@pytest.mark.parametrize("f", CASES, ids=lambda f: f.__name__)
def test_launch_script(f, rig, monkeypatch):
    got, want = _run(f, rig, monkeypatch)
    assert got == want


def test_every_stand_in_is_exercised():
    """The union of the wrappers the cases reach is the set of stand-ins installed: no backward wrapper pointnet2 uses is left out."""
    called = set()
    for f in CASES:
        with pytest.MonkeyPatch.context() as mp:
            for name, default in SWITCHES:
                mp.setattr(*name, default)
            r = Rig(mp)
            _run(f, r, mp)
            called |= r.called
            installed = r.installed
    assert called == installed
