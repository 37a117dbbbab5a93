"""PointNet++ SA / FP layers of VoteNet on the HIP hot path -- mirror of the reference's utils.py.

    sample_and_group     utils.py:25-61
    pointnet_sa_module   utils.py:93-158   (group_all=False, pooling='max', knn=False is the
                                            configuration model.py uses; knn=True, group_all=True and
                                            pooling='avg' / 'weighted_avg' / 'max_and_avg' are served too)
    pointnet_sa_module_msg utils.py:161-201 (multi-scale grouping; never reached by model.py)
    pointnet_fp_module   utils.py:266-294

The reference builds these from ~6 TF graph nodes per MLP layer on a materialised
(B,m,K,3+C) tensor.  Here a layer is ONE fused launch (votenet_mlp_linear): the grouped
tensor is never written, BN+ReLU of layer l is applied while layer l+1 loads its input, and
BatchNorm batch statistics come out of the GEMM epilogue.  torch is used for buffers only;
the backward pass is explicit (tape + hand-written backward kernels), not torch.autograd.

Parameters live in one flat fp32 bucket (ParamStore) so that data-parallel training needs a
single RCCL all-reduce over one contiguous gradient buffer per step.
"""
import math
import threading
from typing import NamedTuple

import torch

from . import mlp as M
from . import tf_grouping, tf_interpolate, tf_sampling


PAD_RAGGED = True  # False: ragged plain layers go through the generic bounds-checked GEMM (A/B, tests)
NARROW_FIRST = True  # leaf SA module with 3 + c <= 8 grouped channels: the first layer's output is rebuilt from 8 floats per row, never stored (csrc/narrow.hip)
PAD_RAGGED_IN = True  # ragged INPUT widths (voting's 259) padded as well (Layer.cin_pad); False: the bounds-checked GEMMs (A/B)
ASSEMBLE_FIRST = True  # other SA modules: the first layer's output z0 = P[idx] + dxyz W[0:3] is rebuilt inside the kernels that consume it, never stored (csrc/assemble.hip)
ASSEMBLE_INLINE = True  # also where the geo records were not computed ahead with the geometry (they are built in place)
HALF_GROUPS = True     # modules with nsample = 64 run their grouped MLP on the PIECE layout (csrc/half.hip): a ball keeps the 16-row pieces that hold a real neighbour, slot 0 stands for the dropped copies -- same results up to summation order, 28-68 % fewer grouped rows on room scenes
FUSE_BN_REDUCE = True  # dense input-gradient GEMMs reduce the BatchNorm backward of the layer below in their epilogue


# --------------------------------------------------------------------------- parameters
class ParamStore:
    """All trainable tensors as views into one flat fp32 buffer (and one flat gradient buffer)."""

    def __init__(self, device):
        self.device = device
        self._specs = []  # (name, shape, init)
        self.flat = None
        self.grad = None
        self.views = {}
        self.gviews = {}
        self._tspecs = []   # (tensor name, row_lo, row_hi): W^T blocks wanted by the input-gradient GEMMs
        self._tviews = {}
        self._tflat = self._ttable = None
        self.t_event = None  # recorded after the transposes of the current step; None = stale
        self.split = False      # enable_split(): bf16 x 3 images of the weight matrices for the fused GEMMs (mlp.SplitImages)
        self._split_flat = self._split_t = None
        # every derived copy of the parameters (bf16 x 3 images, transposes, padded copies, inference BatchNorm tables) belongs to a
        # GENERATION of the bucket: params_changed() opens a new one (the optimizer does; so must anyone who writes the parameters in
        # place), and a copy of an older generation is rebuilt before its next use instead of being multiplied by silently
        self.generation = 0
        self._split_gen = -1
        # the (scale | shift | mean | var) blocks the BatchNorm consumers leave behind, one per BatchNorm'ed layer, in ONE persistent
        # buffer (bn_block): the moving-average update of a train step is then one launch over it (votenet_ema_update)
        self._split_rows = []  # (tensor name, row_lo, row_hi): row blocks of a matrix that are GEMM operands of their own (W[3:] of an SA first layer)
        self._bn_specs = []   # (layer name, cout)
        self.bn_flat = None
        self._bn_views = {}
        self._bn_pass = {}     # layer name -> number of the forward pass that wrote its persistent block last (check_bn_block)
        self._bn_passes = 0

    def want_transpose(self, name, lo=0, hi=None):
        """Register rows [lo, hi) of the 2-D tensor `name`: transposed() then serves its transpose from one bucket that
        refresh_transposes() fills with a single launch per step."""
        self._tspecs.append((name, lo, hi, "T", 0))

    def want_padded(self, name, pad_to):
        """Register copies of the tensor `name` whose ragged width is padded to `pad_to` columns (16-byte aligned rows for the
        fast GEMMs): padded(name) = [W | 0] (rows x pad_to) and padded(name, True) = [W | 0]^T (pad_to x rows), refreshed by
        the same launch as the transposes.  A 1-D tensor (bias) is a 1 x n matrix."""
        self._tspecs.append((name, 0, None, "P", pad_to))
        self._tspecs.append((name, 0, None, "PT", pad_to))  # skipped for 1-D tensors when the table is built

    def want_padded_rows(self, name, pad_to):
        """Register copies of the 2-D tensor `name` with its ragged ROW count padded to `pad_to`: padded_rows(name) = [W ; 0]
        (pad_to x cols) for a GEMM whose input carries zero columns up to pad_to, padded_rows(name, True) = [W ; 0]^T
        (cols x pad_to) for the input-gradient GEMM.  Same launch as the transposes."""
        self._tspecs.append((name, 0, None, "R", pad_to))
        self._tspecs.append((name, 0, None, "RT", pad_to))

    def enable_split(self, on=True):
        """The owner promises to call refresh_split() whenever the parameters changed before the next GEMM reads them
        (VoteNetHotPath.forward does, at its start; refresh_transposes() covers the transposed / padded copies)."""
        self.split = bool(on)
        if not on:
            for im in (self._split_flat, self._split_t, getattr(self, "_split_tf", None)):
                if im is not None:
                    im.close()
            self._split_flat = self._split_t = self._split_tf = None

    def refresh_split(self):
        """One launch on the current stream: the images of every eligible 2-D tensor of the bucket."""
        if not self.split or self.flat is None or not self.flat.is_cuda:
            return
        if self._split_flat is None:
            mats = [v for v in self.views.values() if v.dim() == 2]
            mats += [self.views[name][lo:hi] for name, lo, hi in self._split_rows]  # e.g. W[3:]: the per-point GEMM P = feat W[3:]
            self._split_flat = M.SplitImages(mats, pieces=2 if (M.FORWARD_H2 and not M.SPLIT_K) else 3)
        self._split_flat.refresh()
        self._split_gen = self.generation

    def rebuild_split(self):
        """Forget the images of the forward matrices: the next refresh_split() builds them in the form mlp.FORWARD_H2 names NOW (fp16 x 2
        or bf16 x 3).  Captured graphs hold the old images' addresses: the configuration epoch their keys carry moves on."""
        for name in ("_split_flat", "_split_t", "_split_tf"):  # (the padded forward copies change form with the flat images)
            im = getattr(self, name, None)
            if im is not None:
                im.close()
            setattr(self, name, None)
        self._split_gen = -1
        self.t_event = None  # the copies' images are rebuilt with the next refresh_transposes()
        M.CONFIG_EPOCH += 1

    def ensure_split(self):
        """Images of the current generation before a GEMM reads them: a no-op inside a pass (forward() refreshed them at its start),
        one launch when a module is driven directly after the parameters changed (SAModule.forward after an optimizer step)."""
        if self.split and self._split_gen != self.generation:
            self.refresh_split()

    def refresh_transposes(self, stream=None):
        """One launch for every registered W^T block / padded copy, on `stream` (default: the current one); transposed() /
        padded() make the current stream wait for it.  Call again whenever the parameters changed (once per training step)."""
        if not self._tspecs:
            return
        if self._tflat is None:
            base = self.flat.data_ptr()
            table, total, shapes = [], 0, {}
            for name, lo, hi, kind, pad in self._tspecs:
                v = self.views[name]
                v2 = v if v.dim() == 2 else v.view(1, -1)
                if kind == "PT" and v.dim() != 2:
                    continue
                hi_ = v2.shape[0] if hi is None else hi
                rows, cols = hi_ - lo, v2.shape[1]
                src = (v.data_ptr() - base) // 4 + lo * cols
                if kind == "T":      # (cols x rows), leading dimension rows
                    table += [src, total, rows, cols, rows, 1]
                    shp = (cols, rows)
                elif kind == "R":    # (pad x cols): rows >= the tensor's stay zero
                    table += [src, total, rows, cols, cols, 0]
                    shp = (pad, cols)
                elif kind == "RT":   # (cols x pad): the transpose with leading dimension pad
                    table += [src, total, rows, cols, pad, 1]
                    shp = (cols, pad)
                elif kind == "P":    # (rows x pad), zero padding
                    table += [src, total, rows, cols, pad, 0]
                    shp = (rows, pad) if v.dim() == 2 else (pad,)
                else:                # "PT": (pad x rows): rows >= cols of the transpose stay zero
                    table += [src, total, rows, cols, rows, 1]
                    shp = (pad, rows)
                shapes[(name, lo, hi, kind)] = (total, shp)
                n_el = 1
                for d in shp:
                    n_el *= d
                total += (n_el + 3) // 4 * 4
            self._tflat = torch.zeros(total, dtype=torch.float32, device=self.device)  # the padding is never written: stays 0
            self._ttable = torch.tensor(table, dtype=torch.int64, device=self.device)
            self._nseg = len(table) // 6
            for key, (off, shp) in shapes.items():
                n_el = 1
                for d in shp:
                    n_el *= d
                self._tviews[key] = self._tflat[off:off + n_el].view(shp)
        from . import _lib as L_
        cur = torch.cuda.current_stream()
        st = stream if stream is not None else cur
        if st is not cur:
            st.wait_stream(cur)  # the optimizer's update of the parameters is on the caller's stream
        with M.L.device_guard(self.device), torch.cuda.stream(st):
            L_.check(L_.lib().votenet_transpose_segments(self._nseg, L_.ptr(self._ttable), L_.ptr(self.flat),
                                                         L_.ptr(self._tflat), L_.stream_ptr()))
            if self.split:  # the images of the copies, behind the copies on the same stream
                if self._split_t is None:
                    # transposes ("T", "RT", "PT") are read by the backward GEMMs (gradient operands: bf16 x 3); the zero-padded copies
                    # ("R", "P") stand in for W itself in FORWARD GEMMs of ragged widths (voting 259 -> 288 rows, mlp2 79 -> 128 columns):
                    # fp16 x 2 like every other forward matrix (mlp.FORWARD_H2)
                    fwd = [v for k, v in self._tviews.items() if v.dim() == 2 and k[3] in ("R", "P")]
                    bwd = [v for k, v in self._tviews.items() if v.dim() == 2 and k[3] not in ("R", "P")]
                    h2 = M.FORWARD_H2 and not M.SPLIT_K
                    self._split_t = M.SplitImages(bwd + ([] if h2 else fwd))
                    self._split_tf = M.SplitImages(fwd, pieces=2) if h2 else None
                self._split_t.refresh()
                if self._split_tf is not None:
                    self._split_tf.refresh()
            self.t_event = torch.cuda.Event()
            self.t_event.record(st)
        self._t_waited = False

    def params_changed(self):
        """The parameters were written (optimizer step, manual edit): every derived copy is stale from here on."""
        self.generation += 1
        self.t_event = None

    def invalidate_transposes(self):
        self.params_changed()

    def _fresh(self, key):
        if self.t_event is None and self._tspecs and self.flat is not None and self.flat.is_cuda:
            self.refresh_transposes()  # first use since the parameters last changed (inference: once)
        v = self._tviews.get(key) if self.t_event is not None else None
        if v is None:
            return None
        if not self._t_waited:
            torch.cuda.current_stream().wait_event(self.t_event)
            self._t_waited = True
        return v

    def _fresh_wait(self):
        """The current stream waits for this step's derived copies now (a captured stretch must not contain that wait: the event is
        recorded outside the capture)."""
        if self.t_event is None and self._tspecs and self.flat is not None and self.flat.is_cuda:
            self.refresh_transposes()
        if self.t_event is not None and not self._t_waited:
            torch.cuda.current_stream().wait_event(self.t_event)
            self._t_waited = True

    def transposed(self, name, lo=0, hi=None):
        """W[lo:hi]^T, contiguous: from the per-step bucket when registered and fresh, else an ad-hoc copy."""
        v = self._fresh((name, lo, hi, "T"))
        return v if v is not None else self.views[name][lo:hi].t().contiguous()

    def padded(self, name, pad_to, transpose=False):
        """[W | 0] (rows x pad_to), or its transpose: from the per-step bucket when registered and fresh, else an ad-hoc copy."""
        v = self._fresh((name, 0, None, "PT" if transpose else "P"))
        if v is not None:
            return v
        w = self.views[name]
        p = torch.nn.functional.pad(w, (0, pad_to - w.shape[-1]))
        return p.t().contiguous() if transpose else p

    def padded_rows(self, name, pad_to, transpose=False):
        """[W ; 0] (pad_to x cols), or its transpose (cols x pad_to): from the per-step bucket when registered and fresh, else ad hoc."""
        v = self._fresh((name, 0, None, "RT" if transpose else "R"))
        if v is not None:
            return v
        w = self.views[name]
        p = torch.nn.functional.pad(w, (0, 0, 0, pad_to - w.shape[0]))
        return p.t().contiguous() if transpose else p

    def declare(self, name, shape, init):
        self._specs.append((name, tuple(shape), init))

    def bn_block_written(self, name):
        """A forward pass is about to (re)write layer `name`'s persistent BatchNorm block: -> the stamp its record keeps."""
        self._bn_passes += 1
        self._bn_pass[name] = self._bn_passes
        return self._bn_passes

    def materialize(self, seed=0):
        # every view starts on a 16-byte boundary (float4 loads of scale/shift/W rows)
        offs, total = [], 0
        for _, shape, _ in self._specs:
            offs.append(total)
            total += (math.prod(shape) + 3) // 4 * 4
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(total, dtype=torch.float32, device=self.device)
        nbn = sum(4 * c for _, c in self._bn_specs)
        self.bn_flat = torch.zeros(max(nbn, 1), dtype=torch.float32, device=self.device)
        o = 0
        for name, c in self._bn_specs:
            self._bn_views[name] = self.bn_flat[o:o + 4 * c].view(4, c)
            o += 4 * c
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for (name, shape, init), off in zip(self._specs, offs):
            n = math.prod(shape)
            v = self.flat[off:off + n].view(shape)
            if init == "he":
                v.copy_((torch.randn(shape, generator=gen) * math.sqrt(2.0 / shape[0])).to(self.device))
            elif init == "ones":
                v.fill_(1.0)
            self.views[name] = v
            self.gviews[name] = self.grad[off:off + n].view(shape)
        return self

    def offset_of(self, prefix):
        """Element offset inside the flat bucket of the first tensor whose name starts with `prefix` (declaration order)."""
        for name, _, _ in self._specs:
            if name.startswith(prefix):
                return self.views[name].storage_offset()
        raise KeyError(prefix)

    def __getitem__(self, name):
        return self.views[name]

    def g(self, name):
        return self.gviews[name]

    def numel(self):
        return sum(math.prod(s) for _, s, _ in self._specs)


class Layer:
    """One 1x1 Conv2D / FullyConnected (+ BatchNorm + ReLU): utils.py:126-127, model.py:56."""

    def __init__(self, store, name, cin, cout, bn=True, relu=True):
        self.store, self.name, self.cin, self.cout, self.bn, self.relu = store, name, cin, cout, bn, relu
        store.declare(name + "/W", (cin, cout), "he")
        store.want_transpose(name + "/W")
        store.declare(name + "/b", (cout,), "zeros")
        if bn:
            store.declare(name + "/gamma", (cout,), "ones")
            store.declare(name + "/beta", (cout,), "zeros")
            store._bn_specs.append((name, cout))
        # a plain (no BatchNorm) layer with a ragged width -- voting's 259, mlp2's 79 -- runs on copies padded to a multiple of 64
        # columns: the fast GEMMs want 16-byte aligned rows (the generic kernel they replace ran at 19 TFLOP/s)
        self.cout_pad = 0
        if PAD_RAGGED and not bn and cout % 64 != 0 and cin % 32 == 0:
            self.cout_pad = (cout + 63) // 64 * 64
            store.want_padded(name + "/W", self.cout_pad)
            store.want_padded(name + "/b", self.cout_pad)
        # a BatchNorm'ed layer with a ragged INPUT width -- voting's 259 -- takes its dense input zero-padded to a multiple of 64
        # columns against [W ; 0]: forward, weight-gradient and input-gradient GEMMs all leave the bounds-checked kernels
        self.cin_pad = 0
        if PAD_RAGGED and bn and cin % 32 != 0 and cin > 64 and cout % 64 == 0:
            self.cin_pad = (cin + 63) // 64 * 64
            store.want_padded_rows(name + "/W", self.cin_pad)

    def p(self, k):
        st = self.store
        if st.split and st._split_gen != st.generation:
            st.refresh_split()  # a weight is about to be handed to a GEMM: its image must be of this generation
        return st[self.name + "/" + k]

    def wT(self, lo=0, hi=None):
        return self.store.transposed(self.name + "/W", lo, hi)

    def gp(self, k):
        return self.store.g(self.name + "/" + k)


def make_mlp(store, scope, cin, widths, prefix="conv", last_plain=False):
    layers = []
    for i, co in enumerate(widths):
        plain = last_plain and i == len(widths) - 1
        layers.append(Layer(store, "%s/%s%d" % (scope, prefix, i), cin, co, bn=not plain, relu=not plain))
        cin = co
    return layers


# --------------------------------------------------------------------------- MLP chains
# First SA layer: linear map before the grouping (see mlp_chain_forward).  False = the fused GATHER GEMM over the grouped
# rows (votenet_mlp_linear with a GATHER input), kept for comparison and tests.
PRE_LINEAR = True
# Max-pool over the nsample rows of a group started in the last GEMM's epilogue (votenet_mlp_linear_pool) instead of a
# separate pass over z (votenet_bn_relu_max).
POOL_IN_EPILOGUE = True
# Backward of that pooled layer in Gram form (pool_bwd.hip): both GEMMs contract over cin x cin instead of cin x cout and z
# of the layer is neither stored nor read.  False = votenet_mlp_wgrad_bn / votenet_mlp_dgrad_bn on the stored z.
POOL_GRAM_BACKWARD = True
# Backward of an ASSEMBLED first layer on the piece layout decomposed over the points (csrc/half.hip, round 4): the input-gradient GEMM of
# the layer above is a plain one (no epilogue gathers of the per-point table), the pass over the rows bucketed by point reduces the
# first layer's BatchNorm backward and scatters the MASKED gradient, a pass over the points finishes S.  False = the epilogue reduce
# (votenet_assembled_dgrad_bn_reduce_half) + votenet_group_linear_backward_sorted.
ASSEMBLED_DECOMPOSED = True
# Inference mode of every BatchNorm (model.py:98-139 runs with is_training=False): dict layer name -> mlp.FrozenBN built from the
# moving averages (VoteNetHotPath.inference_bn); None = training mode (batch statistics).
class _FrozenBN(threading.local):
    """Inference-mode BatchNorm table (layer name -> mlp.FrozenBN) of the forward pass running on THIS thread, or None (batch
    statistics).  Set with frozen_bn(table) as a context manager (VoteNetHotPath.predict does): thread-local and nesting-safe, so two
    models used from two threads, or a predict() inside another model's pass, do not see each other's tables."""
    table = None


_FROZEN = _FrozenBN()


class frozen_bn:
    def __init__(self, table):
        self.table = table

    def __enter__(self):
        self.prev, _FROZEN.table = _FROZEN.table, self.table
        return self.table

    def __exit__(self, *a):
        _FROZEN.table = self.prev
        return False


# ---- what travels between geometry(), the prefetch ring, forward() and mlp_chain_forward: named records, told apart by type
def _with_inverse(idx):
    """idx and, where it rides on it, the grouping's inverse index (mlp.attach_inverse)."""
    yield idx
    yield from getattr(idx, "_inv", None) or ()


class NarrowRows(NamedTuple):
    """First-layer rows of a narrow module built ahead (csrc/narrow.hip).  half: the unresolved mlp.HalfLayout whose u8 holds the
    compact rows (u8 is then the whole buffer they were written into), or None: the full layout."""
    u8: torch.Tensor
    mom: torch.Tensor
    half: object = None

    def tensors(self):
        yield from (self.u8, self.mom)
        if self.half is not None:
            yield from self.half.tensors()


class AssembledRows(NamedTuple):
    """geo records and per-point sums of an assembled first layer built ahead (csrc/assemble.hip); half as in NarrowRows (its geo)."""
    geo: torch.Tensor
    cntv: torch.Tensor
    mom: torch.Tensor
    half: object = None

    def tensors(self):
        yield from (self.geo, self.cntv, self.mom)
        if self.half is not None:
            yield from self.half.tensors()


class SAGeometry(NamedTuple):
    """The coordinate-only part of one SA level (SAModule.geometry).  first: None -- the first layer's rows are built in place by
    forward() --, NarrowRows or AssembledRows."""
    fps_idx: torch.Tensor
    new_xyz: torch.Tensor
    idx: torch.Tensor
    pts_cnt: torch.Tensor
    first: object = None

    def tensors(self):
        """Every device tensor the record holds (a consumer on another stream tags them with record_stream)."""
        yield from (self.fps_idx, self.new_xyz)
        yield from _with_inverse(self.idx)
        yield self.pts_cnt
        if self.first is not None:
            yield from self.first.tensors()


class FPGeometry(NamedTuple):
    """three_nn taps and their inverse-distance weights (FPModule.geometry)."""
    idx: torch.Tensor
    weight: torch.Tensor

    def tensors(self):
        yield from _with_inverse(self.idx)
        yield self.weight


class FirstLayerGrad(NamedTuple):
    """What mlp_chain_backward hands to SAModule._first_layer_backward where the chain stops at a gather or an assembled first layer.
    Which fields are set says which of three cases it is:
      dz                   the first layer's dz (rows, cout), written out;
      da, coef, relu       the fused first-layer kernels form dz themselves from the gradient da of the layer's activation and the
                           layer's BatchNorm-backward coefficients (coef set, dz not);
      da, relu, bn, tail   the pass decomposed over the points (piece layout) reduces the layer's BatchNorm backward itself: it takes
                           the layer's (scale, shift, mean, var) and the tail of tail_of() and produces the coefficients (neither dz
                           nor coef set)."""
    dz: torch.Tensor = None
    da: torch.Tensor = None
    coef: torch.Tensor = None
    relu: bool = None
    bn: tuple = None
    tail: tuple = None


class DenseInput(NamedTuple):
    """Chain input: rows x (rows, cin).  padded: [x | 0] at the first layer's padded width, when the caller built it (x = padded[:, :cin])."""
    x: torch.Tensor
    padded: torch.Tensor = None


class GatherInput(NamedTuple):
    """Chain input: the sample_and_group concat [xyz[idx] - new_xyz | feat[idx]], never materialised."""
    xyz: torch.Tensor
    new_xyz: torch.Tensor
    feat: torch.Tensor
    idx: torch.Tensor


class NarrowInput(NamedTuple):
    """Chain input: the narrow form's 8 floats per row.  half: the resolved mlp.HalfLayout when u8 (and every row tensor of the chain)
    holds compact rows, or None."""
    u8: torch.Tensor
    mom: torch.Tensor
    half: object = None


class AssembledInput(NamedTuple):
    """Chain input: a first layer assembled inside its consumers from geo and the per-point GEMM.  half: as in NarrowInput (geo)."""
    xyz: torch.Tensor
    new_xyz: torch.Tensor
    feat: torch.Tensor
    idx: torch.Tensor
    geo: torch.Tensor
    cntv: torch.Tensor
    mom: torch.Tensor
    half: object = None


# ---- a layer's record: a plain dict, one per layer on the chain's tape.  Who sets which key, and who reads it:
#   every record (_close_layer)   layer, rows, z (the raw output; None: never stored), pool (the epilogue's raw max / min, for
#                                 bn_pool_finalize); a BatchNorm'ed layer also scale, shift, mean, var (bn_of), bn_out (the block the
#                                 finalize writes: model.py reads it) and bn_pass (check_bn_block); inference mode: scale, shift only
#   kind                          'dense' | 'gather' | 'narrow' | 'assembled': the form of the layer's INPUT (backward: _bn_arm,
#                                 _bwd_written_out; SAModule.backward and _first_layer_backward on the first record)
#   kind 'dense'                  x (the input as the GEMM read it, None above a narrow / assembled first layer), in_scale, in_shift,
#                                 in_relu: the BatchNorm + ReLU of the layer below, folded into this layer's loads
#     cin_padded                  x is [x | 0] at Layer.cin_pad (_first_dense -> _bwd_padded_input)
#     padded                      a plain layer on the copies padded to Layer.cout_pad, z = z_p[:, :cout] (-> _bwd_plain)
#     gram_form, in_affine,       the pooled last layer (mlp_chain_forward -> _bwd_pooled_gram; model.py reads gram_form / in_affine
#       cout, half                and leaves the Gram matrix it launched ahead in gram_ahead, which the lane's thunk pops)
#     narrow, mask0, half         the second layer above a narrow first layer (_first_narrow -> _bwd_above_narrow)
#     assembled, half             the second layer above an assembled first layer (_first_assembled -> _bwd_above_assembled)
#   kind 'gather'                 xyz, new_xyz, feat, idx (_first_gather -> _bn_arm, _first_layer_backward)
#   kind 'narrow'                 u8, mom, half (_first_narrow -> _bwd_above_narrow); z is None
#   kind 'assembled'              xyz, new_xyz, feat, idx, geo, P, wx, half, cntv, mom (_first_assembled -> _bwd_above_assembled and the
#                                 _first_piece_layout / _first_full_layout arms of _first_layer_backward); z is None
#   half                          the chain's resolved mlp.HalfLayout (piece layout) or None; bench.py reads it off the first record
def _close_layer(L, rows, rec, z, st, tape, pool=None):
    """Behind a layer's launch: its BatchNorm as an mlp.PendingBN on the raw sums st (inference mode: the frozen table's entry; a
    plain layer: None), the layer's record completed and appended to the tape.  -> that BatchNorm."""
    if L.bn and _FROZEN.table is not None:
        pend = _FROZEN.table[L.name]  # moving averages: the batch sums of this launch are ignored
        rec.update(scale=pend.scale, shift=pend.shift)
    elif L.bn:
        blk = L.store._bn_views.get(L.name)
        pend = M.PendingBN(st, L.p("gamma"), L.p("beta"), rows, out=blk)
        rec.update(scale=pend.scale, shift=pend.shift, mean=pend.mean, var=pend.var, bn_out=pend.out)
        if blk is not None:
            # the block is PERSISTENT (one per layer, rewritten by every training-mode forward pass of the net): the record
            # remembers which pass wrote it, and whoever reads it later through this record checks that no other pass has since
            rec["bn_pass"] = L.store.bn_block_written(L.name)
    else:
        pend = None
    rec.update(z=z, rows=rows, pool=pool)
    tape.append(rec)
    return pend


# The first layer(s) of a chain per form of its input: (layers, rows, first, tape, keep_z) -> (z, pend, half, layers done).
def _first_dense(layers, rows, first, tape, keep_z):
    L = layers[0]
    w, b = L.p("W"), L.p("b")
    if L.cin_pad and PAD_RAGGED_IN and first.x.is_cuda:
        # [x | 0] against [W ; 0]
        xp = first.padded if first.padded is not None else torch.nn.functional.pad(first.x, (0, L.cin_pad - L.cin))
        z, st = M.linear_dense(xp, L.store.padded_rows(L.name + "/W", L.cin_pad), b, want_stats=L.bn)
        rec = dict(layer=L, kind="dense", x=xp, in_scale=None, in_shift=None, in_relu=False, cin_padded=True)
    else:
        z, st = M.linear_dense(first.x, w, b, want_stats=L.bn)
        rec = dict(layer=L, kind="dense", x=first.x, in_scale=None, in_shift=None, in_relu=False)
    return z, _close_layer(L, rows, rec, z, st, tape), None, 1


def _first_gather(layers, rows, first, tape, keep_z):
    # conv over the sample_and_group concat [xyz[idx]-new_xyz | feat[idx]] (utils.py:50-57,125-127).  A gather
    # commutes with a per-point linear map, so the feature block is ONE GEMM over the b*n points (P = feat W[3:])
    # and the layer output is assembled per grouped row: z = P[idx] + dxyz W[0:3] + bias (votenet_group_linear).
    L = layers[0]
    w, b = L.p("W"), L.p("b")
    xyz, new_xyz, feat, idx = first.xyz, first.new_xyz, first.feat, first.idx
    co = w.shape[1]
    if feat is not None and PRE_LINEAR and co % 4 == 0 and co <= 1024 and 256 % (co // 4) == 0:
        bb, nn, cc = feat.shape
        P, _ = M.linear_dense(feat.reshape(bb * nn, cc), w[3:], None, want_stats=False)
        z, st = M.group_linear(xyz, new_xyz, idx, P, w[:3], b, want_stats=L.bn)
    else:
        z, st = M.linear_gather(xyz, new_xyz, feat, idx, w, b, want_stats=L.bn)
    rec = dict(layer=L, kind="gather", xyz=xyz, new_xyz=new_xyz, feat=feat, idx=idx)
    return z, _close_layer(L, rows, rec, z, st, tape), None, 1


def _first_narrow(layers, rows, first, tape, keep_z):
    # narrow first layer (csrc/narrow.hip): no kernel writes z0 = u8 W0 + b0; its BatchNorm statistics follow from the moments
    # of u8 and the next layer's GEMM rebuilds it in its operand loader
    L0, L = layers[:2]
    u8, mom, half = first.u8, first.mom, first.half
    w0, b0 = L0.p("W"), L0.p("b")
    st = M.narrow_stats(rows, mom, w0, b0) if (L0.bn and _FROZEN.table is None) else None
    pend = _close_layer(L0, rows, dict(layer=L0, kind="narrow", u8=u8, mom=mom, half=half), None, st, tape)
    # training on the piece layout: the GEMM also leaves the first layer's ReLU mask (2 bytes per row and 16 channels) for the
    # backward pass, whose input-gradient epilogue then needs no rebuild of z0 (mlp.NARROW_MASK)
    want_mask = bool(M.NARROW_MASK and keep_z and half is not None and L0.relu and _FROZEN.table is None and M.COEF_TAIL
                     and M.narrow_mask_supported(u8.shape[0], L0.cout))
    res = M.narrow_linear(u8, w0, b0, L.p("W"), L.p("b"), pend, L0.relu, want_stats=L.bn, half=half, want_mask=want_mask)
    z, st = res[:2]
    rec = dict(layer=L, kind="dense", x=None, narrow=True, in_scale=pend.scale if pend is not None else None,
               in_shift=pend.shift if pend is not None else None, in_relu=L0.relu, half=half, mask0=res[2] if want_mask else None)
    return z, _close_layer(L, rows, rec, z, st, tape), half, 2


def _first_assembled(layers, rows, first, tape, keep_z):
    # first layer assembled inside its consumers (csrc/assemble.hip): the per-point GEMM P = feat W[3:] + b is all that runs for it;
    # the BatchNorm statistics of z0 = P[idx] + dxyz W[0:3] come from one pass over the points, the next layer's GEMM rebuilds z0
    L0, L = layers[:2]
    feat, geo, half = first.feat, first.geo, first.half
    w0, b0 = L0.p("W"), L0.p("b")
    bb, nn, cc = feat.shape
    P, _ = M.linear_dense(feat.reshape(bb * nn, cc), w0[3:], b0, want_stats=False)
    st = M.assemble_stats(P, first.cntv, w0[:3], first.mom) if (L0.bn and _FROZEN.table is None) else None
    rec = dict(layer=L0, kind="assembled", xyz=first.xyz, new_xyz=first.new_xyz, feat=feat, idx=first.idx, geo=geo, P=P, wx=w0[:3],
               half=half, cntv=first.cntv, mom=first.mom)
    pend = _close_layer(L0, rows, rec, None, st, tape)
    z, st = M.assembled_linear(geo, P, w0[:3], L.p("W"), L.p("b"), pend, L0.relu, want_stats=L.bn, half=half)
    rec = dict(layer=L, kind="dense", x=None, assembled=True, in_scale=pend.scale if pend is not None else None,
               in_shift=pend.shift if pend is not None else None, in_relu=L0.relu, half=half)
    return z, _close_layer(L, rows, rec, z, st, tape), half, 2


_FIRST_LAYERS = {DenseInput: _first_dense, GatherInput: _first_gather, NarrowInput: _first_narrow, AssembledInput: _first_assembled}


def mlp_chain_forward(layers, rows, first, tape, pool_k=0, keep_z=True):
    """Run a chain of layers over `rows` rows.  first: the chain's input, a DenseInput, GatherInput, NarrowInput or AssembledInput.
    Returns (z_last, pend): the last layer's RAW output and its BatchNorm as an mlp.PendingBN (None for a plain last
    layer) -- nobody has launched a finalize: every BatchNorm is derived from the raw sums in the prologue of the kernel
    that consumes it (the next GEMM inside the chain; the pooling / activation kernel of the caller for the last layer).
    Appends one record per layer to `tape`.
    pool_k > 0: the chain is followed by a max over groups of pool_k rows (utils.py:132); where the shape allows, the last
    GEMM's epilogue starts the pool (raw max / min per group) and the last record carries 'pool' for bn_pool_finalize;
    keep_z=False then skips the store of the last layer's z altogether (nothing downstream reads it in inference)."""
    # pend: BatchNorm of z whose finalize rides in the prologue of z's consumer (mlp.PendingBN); half: the chain's piece layout
    z, pend, half, done = _FIRST_LAYERS[type(first)](layers, rows, first, tape, keep_z)
    for i in range(done, len(layers)):
        L, prev_relu = layers[i], layers[i - 1].relu
        w, b = L.p("W"), L.p("b")
        pool = None
        sc = pend.scale if pend is not None else None  # views: filled when the consumer below has run
        sh = pend.shift if pend is not None else None
        if pool_k and i == len(layers) - 1 and L.bn and POOL_IN_EPILOGUE and \
                M.linear_pool_supported(rows, w.shape[0], w.shape[1], pool_k):
            # training does not store z of this layer either when its backward runs in Gram form (it never reads z)
            gram_form = POOL_GRAM_BACKWARD and pend is not None and M.pool_backward_supported(w.shape[0], w.shape[1], pool_k)
            if half is not None and not (gram_form or not keep_z):
                raise M.L.VotenetError("piece layout: the pooled layer's backward must be in Gram form")
            zn, st, pool = M.linear_dense_pool(z, w, pool_k, b, None, None, prev_relu, keep_z=keep_z and not gram_form, in_bn=pend, half=half,
                                               gamma=L.p("gamma") if half is not None else None)
            rec = dict(layer=L, kind="dense", x=z, in_scale=sc, in_shift=sh, in_relu=prev_relu, gram_form=gram_form,
                       in_affine=pend.out if pend is not None else None, cout=w.shape[1], half=half)
        elif L.cout_pad:
            # ragged plain layer on zero-padded copies of W and b: the fast GEMM, output (rows, cout_pad), the layer's z = [:, :cout]
            zp, st = M.linear_dense(z, L.store.padded(L.name + "/W", L.cout_pad), L.store.padded(L.name + "/b", L.cout_pad), None, None,
                                    prev_relu, want_stats=False, in_bn=pend)
            zn = zp[:, :L.cout]
            rec = dict(layer=L, kind="dense", x=z, in_scale=sc, in_shift=sh, in_relu=prev_relu, padded=True)
        else:
            zn, st = M.linear_dense(z, w, b, None, None, prev_relu, want_stats=L.bn, in_bn=pend)
            rec = dict(layer=L, kind="dense", x=z, in_scale=sc, in_shift=sh, in_relu=prev_relu)
        pend = _close_layer(L, rows, rec, zn, st, tape, pool)
        z = zn
    return z, pend


# Every hand-over to the weight-gradient stream costs an event (a barrier packet in the main queue: a few microseconds in which the
# chain stands still).  WGRAD_BATCH = True collects the weight-gradient launches of a module and hands them over together at
# wgrad_flush() (one event per module: its weight gradients then run underneath the NEXT module's chain); inside WGRAD.fine() (the
# last module of the backward pass, whose weight gradients have nothing after them to hide under) every launch keeps its own hand-over.
WGRAD_BATCH = False  # measured (tools/ab_step.py, same box): 7.81 ms per step per launch vs 7.99 ms batched per module -- where the weight gradients run matters more than the ~30 events saved


class _LaneScope:
    """`with` scope over attributes of the lane: sets them on entry and puts back exactly what it found on exit, also when the body
    raises.  An exception that leaves the OUTERMOST stream scope also drops what the failed pass left behind: deferred thunks (they
    close over a dead step's tensors) and the pending flag (the next join would wait on a stream nobody used)."""

    def __init__(self, lane, **values):
        self.lane, self.values = lane, values

    def __enter__(self):
        self.found = {k: getattr(self.lane, k) for k in self.values}
        self.lane.__dict__.update(self.values)
        self.lane._stream_scopes += "stream" in self.values

    def __exit__(self, exc_type, exc, tb):
        lane = self.lane
        lane.__dict__.update(self.found)
        if "stream" in self.values:
            lane._stream_scopes -= 1
            if exc_type is not None and not lane._stream_scopes:
                lane._deferred.clear()
                lane._pending = False


class WgradLane:
    """Weight gradients hang off the backward chain (reduce -> coef -> dgrad -> reduce ...): nothing downstream needs them before the
    optimizer.  Inside `with WGRAD.on(stream)` (a second HIP stream) they are launched there, concurrently with the input gradient of
    the same layer; join() makes the current stream wait for them.  Tensors a side-stream kernel reads are tagged with record_stream so
    the caching allocator does not hand their memory out early.  One lane per process (WGRAD below); the scopes on() / fine() /
    capturing() are the only way its state changes from outside."""

    def __init__(self):
        self.stream = None  # where weight gradients go; None: inline on the current stream
        self._stream_scopes = 0
        self._pending = False  # something was handed over since the last join()
        self._deferred = []  # WGRAD_BATCH: (thunk, tensors) waiting for the next flush()
        self._fine = False
        # hand-over events, reused round-robin: a wait that has been enqueued keeps the record it saw, so an event may be recorded again
        # as soon as its wait is in the queue (creating and destroying a HIP event per hand-over was ~3 us of host time, 25 times per step)
        self._events, self._event_turn = [], 0
        # A list while a stretch of the step is being captured into a HIP graph (model.StretchGraph): hand-overs then use fresh events (a
        # captured record must not be mixed with the eager life of a pooled event) and, instead of record_stream -- whose bookkeeping
        # the caching allocator defers during a capture -- every tensor a side-branch kernel reads is kept alive until the capture ends, so
        # that the graph's private pool cannot hand its memory to a later allocation of the main branch.
        self._keep = None
        # A list while a stretch is being captured in SEGMENTS (model.StretchGraph): a weight-gradient launch is then not captured at all
        # but recorded as (thunk, tensors) -- the owner replays the segment's graph and runs its thunks on the weight-gradient stream
        # afterwards, launch by launch, beside the next segment.  (Captured on a side branch of the graph instead, the branch's internal
        # stream shared a hardware queue with the geometry prefetch: the whole graph then waited for the 1.6 ms sampling kernel -- 3.94 ->
        # 5.8 ms per step.)
        self._defer = None

    def on(self, stream):
        """Scope: weight gradients go to `stream`, or run inline when it is None."""
        return _LaneScope(self, stream=stream)

    def fine(self):
        """Scope: one hand-over per launch, whatever WGRAD_BATCH says."""
        return _LaneScope(self, _fine=True)

    def capturing(self, keep, defer=None):
        """Scope: a graph capture is under way -- `keep` collects what the side-stream kernels read, `defer` (when a list) the launches."""
        return _LaneScope(self, _keep=keep, _defer=defer)

    def _event(self):
        if self._keep is not None:
            return torch.cuda.Event()
        if len(self._events) < 64:
            self._events.append(torch.cuda.Event())
            return self._events[-1]
        self._event_turn = (self._event_turn + 1) % 64
        return self._events[self._event_turn]

    def hand_over(self, thunks, tensors=()):
        """Run the thunks on the lane's stream behind everything issued so far on the current one.  tensors: what their kernels read
        (none when it lives in a graph's pool: nothing for the allocator to track)."""
        main = torch.cuda.current_stream()
        ev = self._event()
        ev.record(main)
        self.stream.wait_event(ev)
        if self._keep is not None:
            self._keep.extend(tensors)
            self._keep.append(thunks)  # (the closures hold what the kernels they launch read)
        else:
            for t in tensors:
                t.record_stream(self.stream)
        # set_stream both ways instead of the `with torch.cuda.stream(...)` context: the context manager looks the current stream up
        # twice on entry and exit (~40 us per hand-over on the host, ~24 hand-overs per step)
        torch.cuda.set_stream(self.stream)
        try:
            for f in thunks:
                f()
        finally:
            torch.cuda.set_stream(main)
        self._pending = True

    def run(self, fn, *tensors):
        """Run fn() -- launches of weight-gradient kernels reading `tensors` -- on the lane's stream after everything issued so far on
        the current stream (now, or together with the module's other weight gradients at the next flush()); on the current stream when
        there is no weight-gradient stream."""
        tensors = [t for t in tensors if isinstance(t, torch.Tensor)]
        if self._defer is not None:
            self._defer.append((fn, tensors))
        elif self.stream is None:
            fn()
        elif WGRAD_BATCH and not self._fine:
            self._deferred.append((fn, tensors))
        else:
            self.hand_over([fn], tensors)

    def flush(self):
        if self._deferred:
            if self.stream is None:
                for f, _ in self._deferred:
                    f()
            else:
                self.hand_over([f for f, _ in self._deferred], [t for _, ts in self._deferred for t in ts])
            self._deferred.clear()

    def join(self):
        """The current stream waits for every weight-gradient kernel launched on the lane's stream so far."""
        self.flush()
        if self.stream is not None and self._pending:
            ev = self._event()
            ev.record(self.stream)
            torch.cuda.current_stream().wait_event(ev)
            self._pending = False


WGRAD = WgradLane()
on_wgrad_stream, wgrad_flush, wgrad_join = WGRAD.run, WGRAD.flush, WGRAD.join


def check_bn_block(rec):
    """A layer's BatchNorm vectors (scale | shift | mean | var) live in ONE persistent block per layer: a record of an earlier forward
    pass of the same net reads another pass's statistics once a second training-mode pass has run (predict(batch_statistics=True), a
    forward without a tape, a finite-difference probe between forward(tape) and backward(tape)).  Raises instead."""
    n = rec.get("bn_pass")
    if n is not None and rec["layer"].store._bn_pass.get(rec["layer"].name) != n:
        raise M.L.VotenetError("BatchNorm statistics of layer %s: the record belongs to forward pass %d, the layer's persistent block was "
                               "rewritten by a later training-mode pass (run backward / update_moving_averages before the next forward of "
                               "the same net)" % (rec["layer"].name, n))


# ---- backward of a chain: one handler per form of a layer's record r (below: the record of the layer below, None at the first),
# mirroring _first_dense ... _first_assembled.  -> (the gradient that goes on, the BatchNorm-backward coefficients its kernel already
# produced for the layer below or None, True when the chain ends here).  Weight gradients go to the lane as closures over the handler's
# locals: they run LATER, so a handler never rebinds a name its closure reads (the gradient it computes gets a name of its own).
def bn_of(rec):
    """A record's BatchNorm quadruple."""
    return rec["scale"], rec["shift"], rec["mean"], rec["var"]


def below_of(rec, with_z=False):
    """The 'layer below' tuple of the kernels that reduce that layer's BatchNorm backward in their epilogue: (scale, shift, mean, var,
    relu) for pool_dgrad / assembled_dgrad_bn_reduce / narrow_dgrad_bn_reduce, with the layer's z in front for dgrad_bn."""
    if with_z:
        return rec["z"], rec["scale"], rec["shift"], rec["mean"], rec["var"], rec["layer"].relu
    return rec["scale"], rec["shift"], rec["mean"], rec["var"], rec["layer"].relu


def tail_of(rec):
    """What a kernel's tail needs to turn a layer's BatchNorm-backward sums into its coefficient vector (and d gamma, d beta)."""
    Lr = rec["layer"]
    return (rec["rows"], Lr.p("gamma"), Lr.gp("gamma"), Lr.gp("beta"))


def _bwd_pooled_gram(r, below, gout, argmax, zsel, k, want_da):
    # Gram form (pool_bwd.hip).  The short dependent chain reduce -> coef -> prepare goes first, alone on the GPU; the
    # weight-gradient stream (x^T x, arg-max rows, finish) starts beside the dense GEMM that follows it
    L = r["layer"]
    x, aff, W, b, half = r["x"], r["in_affine"], L.p("W"), L.p("b"), r.get("half")
    coef = M.bn_backward_reduce_pool(gout, zsel, *bn_of(r), L.relu, tail=tail_of(r))
    mm = M.pool_dgrad_prepare(W, b, coef, x.shape[0]) if want_da else None

    def wgrad():
        G = r.pop("gram_ahead", None)  # the Gram matrix depends on forward data only: train_step may have launched it ahead
        if G is None:
            G = M.gram(x, aff[:2], r["in_relu"], half=half)
        M.pool_wgrad(x, r["in_scale"], r["in_shift"], r["in_relu"], G, W, b, coef, L.relu, gout, argmax, zsel, k, L.gp("W"), half=half)
    on_wgrad_stream(wgrad, x, aff, coef, gout, argmax, zsel)
    if not want_da:
        return None, None, False
    if below is not None and below["layer"].bn and below["z"] is x:
        da_below, coef_below = M.pool_dgrad(x, r["in_scale"], r["in_shift"], r["in_relu"], W, b, L.wT(), coef, L.relu, gout, argmax, zsel, k,
                                            below=below_of(below), mm=mm, below_tail=tail_of(below), half=half)
        return da_below, coef_below, False
    return M.pool_dgrad(x, r["in_scale"], r["in_shift"], r["in_relu"], W, b, L.wT(), coef, L.relu, gout, argmax, zsel, k, mm=mm,
                        half=half), None, False


# The BatchNorm'ed arms: (r, below, da, coef, pool, want_da); coef: the layer's own coefficients, pool: (argmax, k) when da is the
# pooled gout.  d bias of a BatchNorm'ed layer is identically zero (BN removes the mean): left at 0.
def _bwd_above_assembled(r, r0, da, coef, pool, want_da):
    # second layer above an ASSEMBLED first layer (i == 1): both GEMMs rebuild z0 from geo + P; the input-gradient GEMM's
    # epilogue reduces the first layer's BatchNorm backward on the rebuilt z0
    L, z = r["layer"], r["z"]
    geo, Pt, wx, half = r0["geo"], r0["P"], r0["wx"], r0["half"]
    on_wgrad_stream(lambda: M.assembled_wgrad_bn(geo, Pt, wx, r["in_scale"], r["in_shift"], r["in_relu"], z, coef, L.relu, da, L.gp("W"),
                                                 half=half), geo, Pt, z, coef, da)
    if ASSEMBLED_DECOMPOSED and half is not None and r0["layer"].bn and r0.get("cntv") is not None:
        # the first layer's backward decomposed over the points (csrc/half.hip): a PLAIN input-gradient GEMM here -- no epilogue
        # that gathers the per-point table --; the pass over the rows bucketed by point that follows (SAModule.
        # _first_layer_backward) reduces the first layer's BatchNorm backward itself
        da0 = M.dgrad_bn_half(z, coef, L.relu, L.wT(), da, half)
        return FirstLayerGrad(da=da0, relu=r0["layer"].relu, bn=bn_of(r0), tail=tail_of(r0)), None, True
    da0, coef0 = M.assembled_dgrad_bn_reduce(z, coef, L.relu, L.wT(), da, geo, Pt, wx, below_of(r0), below_tail=tail_of(r0), half=half)
    return da0, coef0, False


def _bwd_above_narrow(r, r0, da, coef, pool, want_da):
    # second layer above a NARROW first layer (i == 1): both GEMMs rebuild z0 from u8; the input-gradient GEMM stores
    # nothing -- its epilogue leaves the first layer's BatchNorm-backward sums and the data term of its weight gradient
    L, z = r["layer"], r["z"]
    L0, u8, mom, half = r0["layer"], r0["u8"], r0["mom"], r0["half"]
    w0, b0 = L0.p("W"), L0.p("b")
    on_wgrad_stream(lambda: M.narrow_wgrad_bn(u8, w0, b0, r["in_scale"], r["in_shift"], r["in_relu"], z, coef, L.relu, da, L.gp("W"),
                                              half=half), u8, z, coef, da)
    coef0, ug = M.narrow_dgrad_bn_reduce(z, coef, L.relu, L.wT(), da, u8, w0, b0, below_of(r0), tail=tail_of(r0), half=half,
                                         mask=r.get("mask0") if M.NARROW_MASK else None)
    M.narrow_wgrad_first(mom, ug, coef0, w0, b0, L0.gp("W"))
    return None, None, True  # a leaf: nothing upstream takes a gradient


def _bwd_padded_input(r, below, da, coef, pool, want_da):
    # the layer on [x | 0] and [W ; 0]: dW through a padded scratch (its rows >= cin multiply zeros), da = dz [W ; 0]^T
    L, z = r["layer"], r["z"]

    def wgrad():
        G = M._zeros_f32((L.cin_pad, L.cout), z.device)
        M.wgrad_dense_bn(r["x"], z, coef, L.relu, G, da=da)
        gw = L.gp("W")
        M.row_segments(L.cin, [(gw, gw, G[:L.cin])])  # dW += the scratch's first cin rows (in place, one launch)
    on_wgrad_stream(wgrad, r["x"], z, coef, da)
    if not want_da:
        return None, None, False
    return M.dgrad_bn(z, coef, L.relu, L.store.padded_rows(L.name + "/W", L.cin_pad, transpose=True), da=da)[:, :L.cin], None, False


def _bwd_fused_dense(r, below, da, coef, pool, want_da):
    # dz never materialised: both GEMMs rebuild it from (da | gout, z, coef) in their loaders
    L, z = r["layer"], r["z"]
    src = dict(gout=da, argmax=pool[0], k=pool[1]) if pool else dict(da=da)
    on_wgrad_stream(lambda: M.wgrad_dense_bn(r["x"], z, coef, L.relu, L.gp("W"), in_scale=r["in_scale"], in_shift=r["in_shift"],
                                             in_relu=r["in_relu"], **src), r["x"], z, coef, da, pool[0] if pool else None)
    if not want_da:
        return None, None, False
    if FUSE_BN_REDUCE and not pool and below is not None and below["layer"].bn and below["z"] is r["x"]:
        # the layer below's BatchNorm-backward sums come out of this GEMM's store epilogue
        da_below, coef_below = M.dgrad_bn(z, coef, L.relu, L.wT(), da=da, below=below_of(below, with_z=True), below_tail=tail_of(below))
        return da_below, coef_below, False
    return M.dgrad_bn(z, coef, L.relu, L.wT(), **src), None, False


def _bwd_first_fused(r, below, da, coef, pool, want_da):
    # an assembled or gather first layer whose dz is formed inside votenet_group_linear_backward[_assembled]: the module finishes it
    return FirstLayerGrad(da=da, coef=coef, relu=r["layer"].relu), None, True


def _bwd_unfused(r, below, da, coef, pool, want_da):
    dz = M.bn_backward_apply(r["z"], coef, r["layer"].relu, da, argmax=pool[0] if pool else None, k=pool[1] if pool else 0)
    return _bwd_written_out(r, below, dz, want_da)


def _bwd_written_out(r, below, dz, want_da):
    """The plain GEMMs on a dz that exists in memory (unfused BatchNorm'ed layer, plain layer)."""
    L = r["layer"]
    if below is None and r["kind"] == "gather":
        return FirstLayerGrad(dz=dz), None, True  # the module finishes the first layer: it owns idx / pts_cnt / the tables
    on_wgrad_stream(lambda: M.wgrad_dense(r["x"], dz, L.gp("W"), r["in_scale"], r["in_shift"], r["in_relu"]), dz, r.get("x"))
    return (M.linear_dense(dz, L.wT(), want_stats=False)[0] if want_da else None), None, False  # da_prev = dz W^T


def _bwd_plain(r, below, dz, want_da, g_padded):
    """A layer without BatchNorm: dz is the gradient that arrived.  g_padded: the caller's [dz | 0] (last layer only), or None."""
    L = r["layer"]
    # (a weight gradient like the others: on their stream -- the two launches of a column sum were 31 us of the main chain per step)
    on_wgrad_stream(lambda: M.bias_grad(dz, L.gp("b")), dz)
    if not r.get("padded"):
        return _bwd_written_out(r, below, dz, want_da)
    # the layer on the padded copies: dz -> [dz | 0] (rows, cout_pad); dW through a padded scratch, da = dz_p [W | 0]^T
    if g_padded is not None and g_padded.shape[1] == L.cout_pad:
        dzp = g_padded
    else:
        dzp = torch.empty((dz.shape[0], L.cout_pad), dtype=torch.float32, device=dz.device)
        M.row_segments(dz.shape[0], [(dzp[:, :L.cout], dz, None), (dzp[:, L.cout:], None, None)])

    def wgrad():
        G = M._zeros_f32((L.cin, L.cout_pad), dzp.device)
        M.wgrad_dense(r["x"], dzp, G, r["in_scale"], r["in_shift"], r["in_relu"])
        gw = L.gp("W")
        M.row_segments(L.cin, [(gw, gw, G[:, :L.cout])])  # dW += the scratch's first cout columns (in place, one launch)
    on_wgrad_stream(wgrad, dzp, r.get("x"))
    if not want_da:
        return None, None, False
    return M.linear_dense(dzp, L.store.padded(L.name + "/W", L.cout_pad, transpose=True), want_stats=False)[0], None, False


def mlp_chain_backward(recs, g, mode, argmax=None, k=0, need_input_grad=True, zsel=None, g_padded=None):
    """Backward of mlp_chain_forward.  g / mode describe the gradient arriving at the LAST layer:
         'pool'  : g = gout (rows/k, c) of the max over k of relu(bn(z))      (SA layers, utils.py:132)
         'act'   : g = dy (rows, c) of y = relu(bn(z))                         (FP layers)
         'plain' : g = dz (rows, c) of a last layer without BN / activation    (mlp2, voting)
    Accumulates parameter gradients into the store's gradient bucket.  Returns
         a tensor         : the gradient with respect to the chain's dense input (rows, cin), when need_input_grad;
         None             : a dense input with need_input_grad=False, or a narrow first layer (a leaf: its weight gradient is done);
         a FirstLayerGrad : a gather or an assembled first layer -- the chain stops there and SAModule._first_layer_backward
                            finishes the layer (weight gradient, point gradients)."""
    for r in recs:
        check_bn_block(r)
    last = len(recs) - 1
    da = g
    coef_from_above = None  # BatchNorm-backward coefficients of layer i that the kernel of layer i + 1 already produced (the reduce
    #                         rides in its scatter pass / GEMM epilogue, the coefficient vector in that kernel's tail)
    for i in range(last, -1, -1):
        r, below = recs[i], recs[i - 1] if i > 0 else None
        L = r["layer"]
        pooled = mode == "pool" and i == last
        want_da = i > 0 or need_input_grad
        if pooled and r.get("gram_form") and zsel is not None:
            step = _bwd_pooled_gram(r, below, da, argmax, zsel, k, want_da)
        elif not L.bn:
            step = _bwd_plain(r, below, da, want_da, g_padded if i == last else None)
        else:
            coef = coef_from_above
            if coef is None:  # (z is None for a first layer that is never stored: its coefficients always come from above)
                coef = M.bn_backward_reduce(r["z"], *bn_of(r), L.relu, da, argmax=argmax if pooled else None, k=k if pooled else 0,
                                            tail=tail_of(r))
            if r.get("assembled"):
                arm = _bwd_above_assembled
            elif r.get("narrow"):
                arm = _bwd_above_narrow
            elif r.get("cin_padded") and not pooled and M.dgrad_bn_supported(r["rows"], L.cout, L.cin_pad):
                arm = _bwd_padded_input
            elif r["kind"] == "dense" and (not want_da or M.dgrad_bn_supported(r["rows"], L.cout, r["x"].shape[1])):
                arm = _bwd_fused_dense
            elif i == 0 and r["kind"] == "assembled":
                arm = _bwd_first_fused
            elif i == 0 and r["kind"] == "gather" and PRE_LINEAR and not pooled and r["feat"] is not None and \
                    M.group_linear_backward_supported(L.cout, r["idx"].shape[2]):
                arm = _bwd_first_fused
            else:
                arm = _bwd_unfused
            step = arm(r, below, da, coef, (argmax, k) if pooled else None, want_da)
        da, coef_from_above, done = step
        if done:
            break
    return da


def add_rows(a, b):
    """a + b for two (..., c) tensors of equal shape as ONE launch of the glue kernel; either may be a column slice of a wider
    row-major tensor (FPModule.backward returns d_points1 that way).  -> a new contiguous tensor."""
    c = a.shape[-1]
    rows = a.numel() // c
    out = torch.empty(a.shape, dtype=torch.float32, device=a.device)

    def two_d(t):
        if t.is_contiguous():
            return t.view(rows, c)
        if M.L.pitched_rows(t):
            return t.as_strided((rows, c), (t.stride(1), 1), t.storage_offset())
        return t.contiguous().view(rows, c)
    M.row_segments(rows, [(out.view(rows, c), two_d(a), two_d(b))])
    return out


# --------------------------------------------------------------------------- SA / FP modules
def _group_indices(radius, nsample, xyz, new_xyz, knn):
    """utils.py:46-49: ball query, or the nsample nearest points with knn=True (every slot then holds a distinct point)."""
    if knn:
        _, idx = tf_grouping.knn_point(nsample, xyz, new_xyz)
        return M.attach_inverse(idx, xyz.shape[1]), torch.full(idx.shape[:2], nsample, dtype=torch.int32, device=idx.device)
    idx, cnt = tf_grouping.query_ball_point(radius, nsample, xyz, new_xyz)
    return M.attach_inverse(idx, xyz.shape[1]), cnt  # the grouping's inverse (idx._inv) for the deterministic backward pass


def sample_and_group(npoint, radius, nsample, xyz, sample_xyz=None, knn=False):
    """utils.py:42-49 (geometry part): FPS on sample_xyz if given, centres gathered from xyz."""
    fps_idx = tf_sampling.farthest_point_sample(npoint, sample_xyz if sample_xyz is not None else xyz)
    new_xyz = tf_sampling.gather_point(xyz, fps_idx)
    idx, pts_cnt = _group_indices(radius, nsample, xyz, new_xyz, knn)
    return fps_idx, new_xyz, idx, pts_cnt


POOLINGS = ("max", "avg", "weighted_avg", "max_and_avg")  # utils.py:131-146


class SAModule:
    """pointnet_sa_module (utils.py:93-158) with use_xyz=True, bn=True.

    The default configuration (group_all=False, pooling='max') runs the fused forms below (narrow / assembled first layer, piece
    layout, max-pool in the GEMM epilogue, Gram-form backward).  group_all=True or another pooling mode runs the plain chain (every
    z stored) and the pool as its own launch (votenet_bn_relu_pool, csrc/pool_modes.hip): the fused forms are max-specific -- the
    piece layout drops the rows that repeat a ball's first hit, which a mean or a softmax counts."""

    def __init__(self, store, scope, npoint, radius, nsample, cin, mlp, mlp2=None, knn=False, prefix="conv", leaf=False, pooling="max",
                 group_all=False):
        """leaf: the input points carry no gradient (the first module of a network): backward() then returns (None, None), which
        lets a narrow first layer (3 + cin <= 8) run without ever storing its output (NARROW_FIRST, csrc/narrow.hip).
        pooling: 'max' | 'avg' | 'weighted_avg' | 'max_and_avg' (utils.py:131-146; the last pools to 2 mlp[-1] channels, [avg | max]).
        group_all: one group of all n points per scene, centre 0, uncentred coordinates (utils.py:64-90); npoint, radius, nsample
        and knn are ignored."""
        if pooling not in POOLINGS:
            raise ValueError("SAModule: pooling must be one of %s, got %r" % (", ".join(POOLINGS), pooling))
        self.pooling, self.group_all = pooling, bool(group_all)
        self.plain_pool = self.group_all or pooling != "max"  # the pool as its own launch behind the plain chain
        if self.group_all:
            npoint, radius, nsample, knn = 1, None, None, False
        self.npoint, self.radius, self.nsample, self.knn = npoint, radius, nsample, knn
        self.leaf, self.cin = leaf, cin
        self.mlp = make_mlp(store, scope, 3 + cin, mlp, prefix)
        store.want_transpose(self.mlp[0].name + "/W", 3, None)  # W[3:]^T: the per-point feature gradient
        store._split_rows.append((self.mlp[0].name + "/W", 3, None))  # W[3:]: the per-point GEMM of the forward pass gets its image too
        store.want_transpose(self.mlp[0].name + "/W", 0, 3)     # W[:3]^T: the xyz gradient (proposal layer)
        pooled = 2 * mlp[-1] if pooling == "max_and_avg" else mlp[-1]
        self.mlp2 = make_mlp(store, scope, pooled, mlp2, "conv_post_", last_plain=True) if mlp2 else None

    def narrow(self, rows):
        """True when this module runs its first layer in the narrow form for `rows` grouped rows."""
        m = self.mlp
        return bool(NARROW_FIRST and not self.plain_pool and self.leaf and len(m) >= 3 and m[0].bn and m[1].bn and m[0].relu and
                    M.narrow_supported(rows, 3 + self.cin, m[0].cout, m[1].cout))

    def assembled(self, b, n):
        """True when this module's first layer is assembled inside its consumers (csrc/assemble.hip) for b scenes of n points."""
        m = self.mlp
        if self.plain_pool:
            return False
        rows = b * self.npoint * self.nsample
        return bool(ASSEMBLE_FIRST and PRE_LINEAR and not M.DETERMINISTIC and self.cin > 0 and not self.narrow(rows) and len(m) >= 3
                    and m[0].bn and m[1].bn and m[0].relu and M.assembled_supported(rows, m[0].cout, m[1].cout)
                    and M.group_linear_backward_supported(m[0].cout, self.nsample) and b * n * m[0].cout * 4 < 2 ** 32)

    def half_groups(self, b, n):
        """True when this module's grouped MLP runs on the piece layout (csrc/half.hip: the rows that repeat slot 0 dropped by
        halves of a ball) for b scenes of n points: an assembled first layer, three BatchNorm'ed layers, the pooled one in Gram form."""
        m = self.mlp
        if not (HALF_GROUPS and not self.plain_pool and not M.DETERMINISTIC and not self.knn and self.nsample == 64 and len(m) == 3 and m[2].bn and POOL_IN_EPILOGUE
                and POOL_GRAM_BACKWARD and (b * self.npoint) % 8 == 0 and M.pool_backward_supported(m[1].cout, m[2].cout, 64)):
            return False
        return bool(self.narrow(b * self.npoint * 64) or (m[1].cout == 128 and self.assembled(b, n)))

    def geometry(self, xyz, sample_xyz=None, fps_idx=None, points=None, ahead=True, grouped=None):
        """The weight-independent part of the layer (FPS, centres, ball query) as an SAGeometry: can run ahead on a side stream.
        points: the module's input features; given for a narrow leaf module, the grouped rows u8 and their moments (which depend
        on coordinates and input features only) come with the result (first = NarrowRows).
        grouped: (fps_idx, new_xyz, idx, pts_cnt) already made for xyz (vote_sampling.cluster_votes): no gather, no ball query here;
        the rest as with ahead=False -- the caller is inside the step it serves."""
        if grouped is not None:
            fps_idx, new_xyz, idx, pts_cnt = grouped
            idx = M.attach_inverse(idx, xyz.shape[1])  # (the deterministic mode's inverse, as _group_indices attaches it)
            ahead = False
        elif fps_idx is None:
            fps_idx, new_xyz, idx, pts_cnt = sample_and_group(self.npoint, self.radius, self.nsample, xyz, sample_xyz, self.knn)
        else:
            new_xyz = tf_sampling.gather_point(xyz, fps_idx)
            idx, pts_cnt = _group_indices(self.radius, self.nsample, xyz, new_xyz, self.knn)
        first = None
        if (points is not None or self.cin == 0) and self.narrow(xyz.shape[0] * self.npoint * self.nsample):
            if ahead and self.half_groups(xyz.shape[0], xyz.shape[1]):
                half = M.half_groups(pts_cnt)
                first = NarrowRows(*M.narrow_rows_half(xyz, new_xyz, points, idx, pts_cnt, half), half)
            else:
                first = NarrowRows(*M.narrow_rows(xyz, new_xyz, points, idx))
        elif (ahead or ASSEMBLE_INLINE) and self.half_groups(xyz.shape[0], xyz.shape[1]):
            # the layout and the count of its pieces: known on the host by the time the MLP runs when the geometry is computed ahead;
            # inside the step it serves (the proposal module: the votes exist only now) the count stays on the device -- waiting for it
            # would drain the queue -- and the kernels stop at it themselves
            half = M.half_groups(pts_cnt, device_count=not ahead)
            first = AssembledRows(*M.assemble_rows_half(xyz, new_xyz, idx, pts_cnt, half), half)
            M.half_sort_rows(half, xyz.shape[0] * xyz.shape[1])  # the rows bucketed by point, for the first layer's backward
        elif self.assembled(xyz.shape[0], xyz.shape[1]) and (ahead or ASSEMBLE_INLINE):  # ahead=False: called inside the step it serves
            first = AssembledRows(*M.assemble_rows(xyz, new_xyz, idx, pts_cnt=pts_cnt, in_pass=not ahead))  # geo records + per-point sums: coordinates only
        return SAGeometry(fps_idx, new_xyz, idx, pts_cnt, first)

    def forward(self, xyz, points, sample_xyz=None, tape=None, geom=None):
        """xyz (B,n,3), points (B,n,C) or None -> new_xyz (B,m,3), new_points (B,m,C'), idx (B,m,K).
        geom: the SAGeometry returned by geometry() when it was computed ahead of time."""
        if self.plain_pool:
            return self._forward_plain_pool(xyz, points, sample_xyz, tape, geom)
        b = xyz.shape[0]
        geom = geom if geom is not None else self.geometry(xyz, sample_xyz, points=points)
        fps_idx, new_xyz, idx, pts_cnt, ahead = geom.fps_idx, geom.new_xyz, geom.idx, geom.pts_cnt, geom.first
        recs = []
        rows = b * self.npoint * self.nsample
        if self.narrow(rows):
            r = ahead if isinstance(ahead, NarrowRows) else NarrowRows(*M.narrow_rows(xyz, new_xyz, points, idx))
            half = r.half.resolve() if r.half is not None else None  # piece layout: the compact rows
            first = NarrowInput(half.u8 if half is not None else r.u8, r.mom, half)
        elif points is not None and self.assembled(b, xyz.shape[1]) and (isinstance(ahead, AssembledRows) or ASSEMBLE_INLINE):
            r = ahead if isinstance(ahead, AssembledRows) else AssembledRows(*M.assemble_rows(xyz, new_xyz, idx, pts_cnt=pts_cnt, in_pass=True))
            half = r.half.resolve() if r.half is not None else None  # piece layout: the compact rows
            first = AssembledInput(xyz, new_xyz, points, idx, half.geo if half is not None else r.geo, r.cntv, r.mom, half)
        else:
            first = GatherInput(xyz, new_xyz, points, idx)
        z, pend = mlp_chain_forward(self.mlp, rows, first, recs, pool_k=self.nsample, keep_z=tape is not None)
        if recs[-1]["pool"] is not None:  # utils.py:132, the pass over z already done by the GEMM epilogue
            res = M.bn_pool_finalize(recs[-1]["pool"], None, None, True, want_argmax=tape is not None, bn=pend,
                                     want_zsel=tape is not None and bool(recs[-1].get("gram_form")), half=recs[-1].get("half"))
            pooled, argmax, zsel = res if len(res) == 3 else (res[0], res[1], None)
        else:
            zsel = None
            sc, sh = pend.finalize()
            pooled, argmax = M.bn_relu_max(z, self.nsample, sc, sh, True, want_argmax=tape is not None)
        recs2 = []
        out = pooled
        if self.mlp2:
            z2, _ = mlp_chain_forward(self.mlp2, b * self.npoint, DenseInput(pooled), recs2)
            out = z2  # last conv_post layer has no activation (utils.py:153)
        if tape is not None:
            tape.append(dict(op="sa", module=self, recs=recs, recs2=recs2, argmax=argmax, zsel=zsel, fps_idx=fps_idx, idx=idx, pts_cnt=pts_cnt,
                             xyz=xyz, points=points, new_xyz=new_xyz, b=b))
        return new_xyz, out.reshape(b, self.npoint, -1), idx


    def backward(self, rec, g_out, need_feat_grad=True, need_xyz_grad=False):
        """g_out (B,m,C') -> d_points (B,n,C) or None, d_xyz (B,n,3) or None."""
        if self.plain_pool:
            return self._backward_plain_pool(rec, g_out, need_feat_grad, need_xyz_grad)
        b = rec["b"]
        g = g_out.reshape(b * self.npoint, -1).contiguous()
        if self.mlp2:
            g = mlp_chain_backward(rec["recs2"], g, "plain", need_input_grad=True)
        need_feat = need_feat_grad and rec["points"] is not None
        h = mlp_chain_backward(rec["recs"], g, "pool", argmax=rec["argmax"], k=self.nsample, need_input_grad=need_feat,
                               zsel=rec.get("zsel"))
        if rec["recs"][0]["kind"] == "narrow":
            if need_feat or need_xyz_grad:
                raise ValueError("SAModule(leaf=True): the narrow first layer keeps no per-row gradient; build the module with leaf=False")
            return None, None
        return self._first_layer_backward(rec, h, need_feat, need_xyz_grad)

    def _forward_plain_pool(self, xyz, points, sample_xyz, tape, geom):
        """forward() of a group_all module or of a pooling mode other than max: the plain chain with every z stored, then
        votenet_bn_relu_pool over the last layer's raw z (its BatchNorm finalized first)."""
        b, n = xyz.shape[:2]
        if self.group_all:
            # sample_and_group_all (utils.py:64-90): centre 0, idx = arange(n), the grouped rows [xyz | points] of every point
            # uncentred -- a dense (b n, 3 + c) input built in one launch, no gather
            fps_idx = pts_cnt = None
            new_xyz = torch.zeros((b, 1, 3), dtype=torch.float32, device=xyz.device)
            idx = torch.arange(n, dtype=torch.int32, device=xyz.device).view(1, 1, n).expand(b, 1, n).contiguous()
            m, k = 1, n
            x = xyz.reshape(b * n, 3)
            if points is not None:
                c = points.shape[2]
                x = torch.empty((b * n, 3 + c), dtype=torch.float32, device=xyz.device)
                M.row_segments(b * n, [(x[:, :3], xyz.reshape(b * n, 3), None), (x[:, 3:], points.reshape(b * n, c), None)])
            first = DenseInput(x)
        else:
            geom = geom if geom is not None else self.geometry(xyz, sample_xyz)
            fps_idx, new_xyz, idx, pts_cnt = geom.fps_idx, geom.new_xyz, geom.idx, geom.pts_cnt
            m, k = self.npoint, self.nsample
            first = GatherInput(xyz, new_xyz, points, idx)
        rows = b * m * k
        recs = []
        z, pend = mlp_chain_forward(self.mlp, rows, first, recs)
        sc, sh = pend.finalize()
        w = None
        if self.pooling == "weighted_avg":
            w = M.sa_pool_weights(xyz, None, None) if self.group_all else M.sa_pool_weights(xyz, new_xyz, idx)
        pooled, argmax = M.bn_relu_pool(z, k, sc, sh, self.mlp[-1].relu, self.pooling, w=w, want_argmax=tape is not None)
        recs2 = []
        out = pooled
        if self.mlp2:
            out, _ = mlp_chain_forward(self.mlp2, b * m, DenseInput(pooled), recs2)
        if tape is not None:
            tape.append(dict(op="sa", module=self, recs=recs, recs2=recs2, argmax=argmax, zsel=None, fps_idx=fps_idx, idx=idx,
                             pts_cnt=pts_cnt, xyz=xyz, points=points, new_xyz=new_xyz, b=b, m=m, k=k, weights=w))
        return new_xyz, out.reshape(b, m, -1), idx

    def _backward_plain_pool(self, rec, g_out, need_feat_grad, need_xyz_grad):
        """backward() of _forward_plain_pool: the gradient reaching the last activation is written out (votenet_sa_pool_grad) and the
        chain runs its 'act' backward; weighted_avg adds the coordinate gradient through its softmax weights."""
        b, m, k = rec["b"], rec["m"], rec["k"]
        g = g_out.reshape(b * m, -1).contiguous()
        if self.mlp2:
            g = mlp_chain_backward(rec["recs2"], g, "plain", need_input_grad=True)
        last = rec["recs"][-1]
        c = last["layer"].cout
        need_feat = need_feat_grad and rec["points"] is not None
        dy = M.sa_pool_grad(g, k, c, self.pooling, w=rec["weights"], argmax=rec["argmax"])
        dv = None
        if need_xyz_grad and self.pooling == "weighted_avg":
            new_xyz, idx = (None, None) if self.group_all else (rec["new_xyz"], rec["idx"])
            dv = M.sa_pool_weights_grad(rec["xyz"], new_xyz, idx, last["z"], last["scale"], last["shift"], last["layer"].relu, g,
                                        rec["weights"])
        xyz = rec["xyz"]
        n = xyz.shape[1]
        if not self.group_all:
            h = mlp_chain_backward(rec["recs"], dy, "act", need_input_grad=need_feat)
            return self._first_layer_backward(rec, h, need_feat, need_xyz_grad, d_rows_xyz_extra=dv)
        # group_all: the chain's input is the dense [xyz | points]; its gradient splits into the two blocks
        dx = mlp_chain_backward(rec["recs"], dy, "act", need_input_grad=need_feat or need_xyz_grad)
        d_feat = d_xyz = None
        if need_feat:
            c_in = rec["points"].shape[2]
            d_feat = torch.empty((b * n, c_in), dtype=torch.float32, device=xyz.device)
            M.row_segments(b * n, [(d_feat, dx[:, 3:3 + c_in], None)])
            d_feat = d_feat.view(b, n, c_in)
        if need_xyz_grad:
            d_xyz = torch.empty((b * n, 3), dtype=torch.float32, device=xyz.device)
            M.row_segments(b * n, [(d_xyz, dx[:, :3], dv)])
            d_xyz = d_xyz.view(b, n, 3)
        return d_feat, d_xyz

    def _first_layer_backward(self, rec, h, need_feat, need_xyz_grad, d_rows_xyz_extra=None):
        """Backward of z = P[idx] + dxyz W[0:3] (P = feat W[3:]) from the chain's FirstLayerGrad h:
             dW[0:3] += dxyz^T dz                     (over the grouped rows)
             S = scatter-add of dz rows by idx        (b, n, cout)  -- GroupPointGrad on the layer OUTPUT width
             dW[3:]  += feat^T S ,  d_feat = S W[3:]^T                (two GEMMs over the b*n points, not the grouped rows)
             d_xyz / d_new_xyz from dz W[0:3]^T       (proposal layer only)
        Four ways to S and dz -- dz written out, assembled on the piece layout, assembled on the full layout, gather fused: one
        kernel forms dz from (z, da), scatters it and reduces the xyz rows of dW in a single pass --, then the common tail."""
        r0 = rec["recs"][0]
        L0 = r0["layer"]
        W, gW = L0.p("W"), L0.gp("W")
        xyz, new_xyz, feat, idx, pts_cnt = r0["xyz"], r0["new_xyz"], r0["feat"], r0["idx"], rec["pts_cnt"]
        b, n = xyz.shape[:2]
        cout = W.shape[1]
        d_feat = d_xyz = None
        if h.dz is not None:
            S, dz = _first_written_out(rec, h.dz, gW), h.dz
        elif r0["kind"] == "assembled" and r0.get("half") is not None:
            S, dz, d_xyz = _first_piece_layout(rec, h, W, gW, need_xyz_grad)  # d_xyz: finished there
        elif r0["kind"] == "assembled":
            S, dz = M.group_linear_backward_assembled(xyz, new_xyz, idx, pts_cnt, r0["P"], r0["wx"], h.da, h.coef, h.relu, gW[:3],
                                                      want_dz=need_xyz_grad)
        else:
            S, dz = M.group_linear_backward(xyz, new_xyz, idx, pts_cnt, r0["z"], h.da, h.coef, h.relu, gW[:3], want_dz=need_xyz_grad)
        if feat is not None:
            c = feat.shape[2]
            if PRE_LINEAR:
                S2, feat2 = S.view(b * n, cout), feat.reshape(b * n, c)
                on_wgrad_stream(lambda: M.wgrad_dense(feat2, S2, gW[3:]), S2, feat2)
                if need_feat:
                    d2, _ = M.linear_dense(S2, L0.wT(3, None), want_stats=False)
                    d_feat = d2.view(b, n, c)
            else:  # the fused GATHER GEMMs over the grouped rows
                on_wgrad_stream(lambda: M.wgrad_gather(xyz, new_xyz, feat, idx, dz, gW), dz, feat)
                if need_feat:
                    d_rows_feat, _ = M.linear_dense(dz, L0.wT(3, None), want_stats=False)
                    d_feat, _, _ = M.group_concat_grad(d_rows_feat, None, idx, pts_cnt, n, c)
        if need_xyz_grad and d_xyz is None:
            d_rows_xyz = M.rows_dot3(dz, W[:3])  # dz W[0:3]^T, three columns: a streaming kernel, not a 128-wide GEMM tile
            if d_rows_xyz_extra is not None:  # weighted_avg: the gradient through the pooling weights, also per grouped row
                d_rows_xyz = add_rows(d_rows_xyz, d_rows_xyz_extra)
            _, d_xyz, d_new = M.group_concat_grad(None, d_rows_xyz, idx, pts_cnt, n, 0)
            d_xyz = tf_sampling.gather_point_grad_raw(n, rec["fps_idx"], d_new, into=d_xyz)  # new_xyz = gather(xyz, fps_idx): accumulated in place
        return d_feat, d_xyz


def _first_written_out(rec, dz, gW):
    """_first_layer_backward on a dz (rows, cout) in memory: the xyz rows of dW on the lane -> S (b, n, cout), or None: no feature block."""
    r0 = rec["recs"][0]
    xyz, new_xyz, feat, idx = r0["xyz"], r0["new_xyz"], r0["feat"], r0["idx"]
    if feat is None or PRE_LINEAR:
        on_wgrad_stream(lambda: M.wgrad_gather(xyz, new_xyz, None, idx, dz, gW), dz)  # rows 0..2 of dW (no feature block)
    if feat is not None and PRE_LINEAR:
        return M.group_concat_grad(dz, None, idx, rec["pts_cnt"], xyz.shape[1], gW.shape[1])[0]
    return None


def _first_piece_layout(rec, h, W, gW, need_xyz_grad):
    """_first_layer_backward of a layer assembled on the piece layout (csrc/half.hip): decomposed over the points -- the pass produces the
    layer's coefficients itself -- or from the coefficients the layer above produced.  -> (S (b, n, cout), None: dz is never written,
    d_xyz (b, n, 3) or None: it comes from S and the centre sums)."""
    r0 = rec["recs"][0]
    half = r0["half"]
    b, n = r0["xyz"].shape[:2]
    if h.coef is None:
        S, coef = M.group_linear_backward_decomposed(half, b, n, r0["P"], r0["wx"], h.da, h.bn, h.relu, h.tail, r0["cntv"], r0["mom"],
                                                     gW[:3], defer=on_wgrad_stream)
    else:
        S, coef = M.group_linear_backward_half(half, b, n, r0["P"], r0["wx"], h.da, h.coef, h.relu, gW[:3]), h.coef
    if not need_xyz_grad:
        return S, None, None
    # dz0 W[0:3]^T is linear in dz0: the points receive S W[0:3]^T, a centre minus the sum of its rows' dz0 times W[0:3]^T
    d_xyz = M.rows_dot3(S.view(b * n, W.shape[1]), W[:3]).view(b, n, 3)
    d_new = M.rows_dot3(M.half_centre_sums(half, r0["P"], r0["wx"], h.da, coef, h.relu), W[:3]).view(b, -1, 3)
    return S, None, tf_sampling.gather_point_grad_raw(n, rec["fps_idx"], d_new, into=d_xyz)


class SAModuleMSG:
    """pointnet_sa_module_msg (utils.py:161-201): one FPS, then per scale i a ball query (radius_list[i], nsample_list[i]),
    the MLP mlp_list[i] (layers "conv<i>_<j>") and a max-pool; the per-scale features are concatenated.
    Each scale is an SAModule sharing the sampled centres, so it runs through the same fused kernels.

    Weight layout: the reference concatenates [grouped_points, grouped_xyz] here (utils.py:186-187) -- features first --
    while the fused first layer takes its rows as [xyz (3) | features (c)] like sample_and_group.  The first-layer W of a
    scale is therefore stored with the three xyz rows FIRST; reference_rows() / from_reference_rows() convert."""

    def __init__(self, store, scope, npoint, radius_list, nsample_list, cin, mlp_list):
        self.npoint, self.cin = npoint, cin
        self.scales = [SAModule(store, scope, npoint, r, k, cin, mlp, prefix="conv%d_" % i)
                       for i, (r, k, mlp) in enumerate(zip(radius_list, nsample_list, mlp_list))]
        self.widths = [mlp[-1] for mlp in mlp_list]

    @staticmethod
    def reference_rows(w):
        """first-layer W stored here ([xyz | feat] rows) -> the reference's row order ([feat | xyz])."""
        return torch.cat([w[3:], w[:3]], 0)

    @staticmethod
    def from_reference_rows(w):
        return torch.cat([w[-3:], w[:-3]], 0)

    def forward(self, xyz, points, tape=None):
        """xyz (B,n,3), points (B,n,C) or None -> new_xyz (B,m,3), new_points (B,m,sum of the scales' last widths)."""
        fps_idx = tf_sampling.farthest_point_sample(self.npoint, xyz)  # utils.py:179
        subs, outs, new_xyz = [], [], None
        for sc in self.scales:
            sub = [] if tape is not None else None
            new_xyz, o, _ = sc.forward(xyz, points, tape=sub, geom=sc.geometry(xyz, fps_idx=fps_idx))
            outs.append(o)
            subs.append(sub[0] if sub else None)
        if tape is not None:
            tape.append(dict(op="sa_msg", module=self, subs=subs))
        return new_xyz, torch.cat(outs, -1)

    def backward(self, rec, g_out, need_feat_grad=True):
        """g_out (B,m,sum widths) -> d_points (B,n,C) or None (summed over the scales)."""
        d_feat, o = None, 0
        for sc, sub, w in zip(self.scales, rec["subs"], self.widths):
            d, _ = sc.backward(sub, g_out[..., o:o + w].contiguous(), need_feat_grad=need_feat_grad)
            o += w
            if d is not None:
                d_feat = d if d_feat is None else d_feat + d
        return d_feat


class FPModule:
    """pointnet_fp_module (utils.py:266-294): 3-NN inverse-distance interpolation + MLP."""

    def __init__(self, store, scope, cin1, cin2, mlp):
        self.mlp = make_mlp(store, scope, cin1 + cin2, mlp, "conv_")

    @staticmethod
    def geometry(xyz1, xyz2):
        """three_nn + inverse-distance weights (utils.py:278-282) as an FPGeometry: feature independent."""
        dist, idx = tf_interpolate.three_nn(xyz1, xyz2)
        return FPGeometry(M.attach_inverse(idx, xyz2.shape[1], always=tf_interpolate.GATHER_GRAD), tf_interpolate.three_nn_weights(dist))

    def forward(self, xyz1, xyz2, points1, points2, tape=None, geom=None):
        b, n1 = xyz1.shape[:2]
        geom = geom if geom is not None else self.geometry(xyz1, xyz2)  # utils.py:278-282
        idx, weight = geom.idx, geom.weight
        if points1 is not None:  # utils.py:283-286: the interpolation writes the concat [interpolated | points1] itself
            x = tf_interpolate.three_interpolate_concat(points2, idx, weight, points1)
        else:
            x = tf_interpolate.three_interpolate(points2, idx, weight)
        rows = b * n1
        recs = []
        z, pend = mlp_chain_forward(self.mlp, rows, DenseInput(x.view(rows, -1)), recs)
        y = M.bn_relu(z, None, None, True, bn=pend)
        if tape is not None:
            tape.append(dict(op="fp", module=self, recs=recs, idx=idx, weight=weight, m=xyz2.shape[1],
                             c2=points2.shape[2], c1=0 if points1 is None else points1.shape[2], b=b, n1=n1))
        return y.view(b, n1, -1)

    def backward(self, rec, dy):
        """dy (B,n1,C) -> d_points1 (B,n1,c1) or None, d_points2 (B,m,c2)."""
        b, n1, c1, c2 = rec["b"], rec["n1"], rec["c1"], rec["c2"]
        d_x = mlp_chain_backward(rec["recs"], dy.reshape(b * n1, -1).contiguous(), "act", need_input_grad=True)
        # [d interpolated | d points1] are column slices of d_x, read in place: ThreeInterpolateGrad takes a row pitch, and
        # d_points1 is returned as a VIEW (its consumer adds it to another gradient: add_rows)
        d_x3 = d_x.view(b, n1, c2 + c1)
        d_p1 = d_x3[:, :, c2:] if c1 else None
        d_p2 = tf_interpolate.three_interpolate_grad_raw(rec["m"], rec["idx"], rec["weight"], d_x3[:, :, :c2])
        return d_p1, d_p2
