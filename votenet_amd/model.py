"""Driver of the hot path in VoteNet's layer configuration (the caller side of the path).

It wires the SA / FP / voting / proposal layers with the exact shapes and hyper-parameters of
model.py:39-49,53-61,89-93, the reference's loss graph (loss.py: model.py:61-84,141-231 as one kernel),
the predict tower (box decode -> 3D NMS, model.py:98-139) and the optimizer (model.py:240-250), so that
the hot path can be driven, checked and timed end to end:

    sa1 20480->2048 r0.2 K64 [64,64,128]     sa2 ->1024 r0.4 [128,128,256]
    sa3 ->512 r0.8 [128,128,256]             sa4 ->256 r1.2 [128,128,256]
    fp1 (l3<-l4) [256,256]                   fp2 (l2<-l3) [256,256]         seeds = l2_xyz
    voting FC 259->256->256->259 (BNReLU,BNReLU,none); votes = [seed_xyz, seed_feat] + offset
    proposal SA on votes, FPS on seeds (utils.py:42-43), 256 x r0.3 K64 [128,128,128] + [128,128,79]
"""

import math
from typing import NamedTuple

import torch

from . import checkpoint
from . import dp
from . import head as H
from . import mlp as M
from . import pointnet2 as P

NH, NS, NC = 12, 10, 10  # config.py:2-3
PREFETCH_AFTER = 2  # when the geometry chain of the next batch is enqueued: -1 at the start of the pass, k after the forward of sa<k>, 5 at the start of the backward pass.  Its FPS holds 8 CUs for 1.7 ms and every GEMM beside it runs ~18 % longer (tools/probe/gemm_beside_fps.py): after sa2 it falls on the small-kernel stretch of the pass (7.03 -> 6.88 ms per step, same box)
SIDE_PRIORITY = 0   # HIP stream priorities of the geometry (prefetch) streams and of the weight-gradient stream (0 = normal)
WGRAD_PRIORITY = 0
PROPOSAL_NUM = 256       # config.py:6
PROPOSAL_OUT = 5 + 2 * NH + 4 * NS + NC  # model.py:91 -> 79
LEARNING_RATE = 1e-3     # the initial value of the reference's learning_rate variable (model.py:241)


GEOMETRY_GRAPHS = True  # prefetch_geometry replays the coordinate-only chain of a batch as ONE HIP graph (GeometryGraph) instead of enqueuing its ~50 launches
GEOMETRY_MAX_EVICTIONS = 8  # a net whose input shape keeps changing stops capturing (two shapes / configurations are kept side by side)
GEOMETRY_RING = 3       # graphs (= sets of geometry buffers) per input shape: a prefetch may run two batches ahead of the step that consumes it


class GeometryGraph:
    """The coordinate-only chain of one batch -- four FPS + ball queries, the piece layouts and their compact rows, the proposal
    layer's FPS, both three_nn: ~50 launches that depend on nothing but the points -- captured once on a prefetch stream and replayed
    per batch.  The chain's buffers live in the graph's memory pool at fixed addresses: a replay overwrites the geometry of the batch
    the graph served before, which is why a net keeps a ring of GEOMETRY_RING of them and tags every hand-out with the graph's
    generation.  The piece counts still reach the host through mapped pinned ints (the graph's own), the layouts are re-armed with the
    event that follows the replay."""

    def __init__(self, chain, x, side, feats=None):
        """chain(x, g, ev, levels, feats): the net's geometry chain (VoteNetHotPath._geometry_chain)."""
        self.x = torch.empty_like(x)
        self.feats = torch.empty_like(feats) if feats is not None else None  # sa1's input features (a net with point_features): its narrow rows are built from them
        self.slots = torch.zeros(16, dtype=torch.int32).pin_memory()
        self.generation = 0
        self.graph = torch.cuda.CUDAGraph()
        g = {}
        # thread_local: a process group's watchdog thread (RCCL, one rank per GPU) queries its events while this thread captures
        with M.layout_slots(self.slots), torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
            chain(self.x, g, None, ("sa1", "sa2", "sa3", "sa4"), self.feats)
        self.g = g
        firsts = [v.first for v in g.values() if isinstance(v, P.SAGeometry) and v.first is not None]
        self.layouts = [f.half for f in firsts if f.half is not None]

    def replay(self, x, side, feats=None):
        """On `side` (current): copy the points (and sa1's input features) in, run the chain -> (g, ev) as _geometry_chain leaves them."""
        self.x.copy_(x, non_blocking=True)
        if self.feats is not None:
            self.feats.copy_(feats, non_blocking=True)
        self.graph.replay()
        done = torch.cuda.Event()
        done.record(side)
        self.generation += 1
        for h in self.layouts:
            h.rearm(done)
        return self.g, {name: done for name in ("sa1", "sa2", "sa3", "sa4", "fp")}


def _record_on_main(g, main):
    """g: what a geometry chain left (SAGeometry / FPGeometry records, the proposal layer's FPS indices).  Tensors born on a side stream
    are consumed on the main stream."""
    for v in g.values():
        for t in (v,) if isinstance(v, torch.Tensor) else v.tensors():
            t.record_stream(main)


class PrefetchEntry(NamedTuple):
    """One prefetched batch: the tensors the chain saw (and their versions then), what it left (g, ev as _geometry_chain fills them),
    the GeometryGraph that holds the result (None: launches) and that graph's generation at the hand-out."""
    x: torch.Tensor
    version: int
    g: dict
    ev: dict
    graph: object
    generation: int
    feats: torch.Tensor = None
    feats_version: int = 0


class GeometryPrefetch:
    """The prefetch state of one net (net._geometry): the pool of batches whose geometry is under way or done, the rings of
    GeometryGraphs per input shape, the graph whose buffers the running pass reads, the two prefetch streams.
    chain: the net's _geometry_chain; side_stream(): its geometry stream (the first of the two prefetch streams); prop_npoint: the
    proposal layer's sample count (the chain runs its FPS: part of a ring's key)."""

    def __init__(self, chain, side_stream, device, prop_npoint):
        self.chain, self.side_stream, self.device, self.prop_npoint = chain, side_stream, device, prop_npoint
        self.pool = {}           # id(x) -> PrefetchEntry, oldest first.  Cleared and mutated in place, NEVER rebound: the net's _prefetched is this dict
        self.rings = {}          # (shape, configuration) -> dict(graphs=[GeometryGraph ...], turn, warm)
        self.evictions = 0       # times a third shape / configuration threw the rings away
        self.graphs_off = False  # too many of those: the chain is enqueued launch by launch from then on
        self.current = None      # the GeometryGraph whose buffers serve the pass being enqueued (None: fresh tensors)
        self.streams = None      # the two prefetch streams, used alternately; created on first use (a CPU-only net never gets there)
        self.turn = 0

    def prefetch(self, next_x, next_feats=None):
        """VoteNetHotPath.prefetch_geometry (next_feats checked: None for a net without point features)."""
        had = self.pool.get(id(next_x))
        if had is not None and had.x is next_x and had.version == next_x._version and (
                next_feats is None or (had.feats is next_feats and had.feats_version == next_feats._version)):
            return
        main = torch.cuda.current_stream()
        if self.streams is None:
            self.streams = [self.side_stream(), torch.cuda.Stream(device=self.device, priority=SIDE_PRIORITY)]
        side = self.streams[self.turn]
        self.turn ^= 1
        gg = self.next_graph(next_x, side, next_feats)
        g, ev = {}, {}
        start = torch.cuda.Event()
        start.record(main)  # next_x may have been produced on the main stream; a graph's buffers may still serve the step before
        with torch.cuda.stream(side):
            side.wait_event(start)
            if gg is not None:
                g, ev = gg.replay(next_x, side, next_feats)
            else:
                self.chain(next_x, g, ev, ("sa1", "sa2", "sa3", "sa4"), next_feats)
        if gg is None:
            _record_on_main(g, main)
        while len(self.pool) >= (GEOMETRY_RING - 1 if gg is not None else 4):  # never picked up: drop the oldest
            self.pool.pop(next(iter(self.pool)))
        self.pool[id(next_x)] = PrefetchEntry(next_x, next_x._version, g, ev, gg, gg.generation if gg is not None else 0,
                                              next_feats, next_feats._version if next_feats is not None else 0)

    def next_graph(self, x, side, feats=None):
        """The next graph of the ring for inputs shaped like x (captured on first use), or None when the chain is enqueued launch by
        launch: graphs off, the deterministic mode (its inverse indices ride on tensors as attributes), a capture under way, per-launch
        profiling events switched on."""
        if not GEOMETRY_GRAPHS or M.DETERMINISTIC or self.graphs_off or torch.cuda.is_current_stream_capturing():
            return None
        if P.tf_sampling.PROFILE_EVENTS is not None or P.tf_grouping.PROFILE_EVENTS is not None:
            return None  # HIP events around single launches of the chain are wanted (bench.py's roofline legs): they need the launches
        key = (tuple(x.shape), x.dtype, P.HALF_GROUPS, P.ASSEMBLE_INLINE, self.prop_npoint) + ((tuple(feats.shape),) if feats is not None else ())
        ring = self.rings.get(key)
        if ring is None:
            if len(self.rings) >= 2:  # another shape / configuration: the old graphs' buffers go
                self.rings.clear()
                self.evictions += 1
                if self.evictions > GEOMETRY_MAX_EVICTIONS:  # shapes keep changing: every capture is a device synchronise
                    import warnings
                    warnings.warn("VoteNetHotPath: the input shape / configuration changed %d times: the prefetched geometry chain is "
                                  "enqueued launch by launch from now on (model.GEOMETRY_GRAPHS)" % self.evictions)
                    self.graphs_off = True
                    return None
            ring = self.rings[key] = dict(graphs=[], turn=0, warm=0)
        if len(ring["graphs"]) < GEOMETRY_RING:
            # the chain has run launch by launch before (sizes its scratch, loads its code objects): at least once per shape
            if ring["warm"] < 1:
                ring["warm"] += 1
                return None
            ring["graphs"].append(GeometryGraph(self.chain, x, side, *([feats] if feats is not None else [])))  # (without features: the three arguments it always took)
            return ring["graphs"][-1]
        gg = ring["graphs"][ring["turn"]]
        ring["turn"] = (ring["turn"] + 1) % GEOMETRY_RING
        if gg is self.current:  # its buffers serve the pass being enqueued (a lookahead beyond the ring)
            return None
        return gg

    def take(self, x, feats=None):
        """The (g, ev) prefetched for exactly this batch, or None: the point tensor AND the feature tensor must be the objects the
        prefetch saw, unchanged since (_version) -- sa1's narrow rows were built from the features -- and the graph that holds the
        result must not have served another batch.  Sets `current` to that graph (None otherwise)."""
        pf = self.pool.pop(id(x), None)
        self.current = None
        if pf is not None and pf.x is x and pf.version == x._version and (pf.graph is None or pf.graph.generation == pf.generation) and \
                pf.feats is feats and (feats is None or pf.feats_version == feats._version):
            self.current = pf.graph
            return pf.g, pf.ev
        return None

    def drop(self):
        """Forget the captured graphs and what was prefetched on them."""
        self.rings.clear()
        self.pool.clear()
        self.current = None


GRAM_EARLY = ()          # levels whose Gram matrix is launched at the start of the levels' backward pass (see _grams_early): measured below
GRAMS_AHEAD = False      # train_step launches the Gram matrices of the levels' pooled layers (forward data only) on the weight-gradient stream under the stretch instead of beside the levels' backward GEMMs.  Measured (tools/probe/variant_step.py, three alternations): 3.78-3.81 -> 3.86-3.89 ms -- the stretch is a chain of tiny latency-bound kernels ON the critical path, and 0.27 ms of GPU-filling kernels beside it cost it more than they save the backward pass.  Off.
INLINE_WGRAD_TAIL = False  # experiment (see _levels_backward): the weight gradients of sa2 / sa1 on the main stream
STRETCH_GRAPH = True     # train_step replays its static stretch (fp1 forward ... fp1 backward: ~85 launches) as HIP graph segments (StretchGraph)
STRETCH_SEGMENTS = True  # the stretch's input-gradient chain cut into graphs at the modules' ends, the weight gradients launched between them (False: two graphs around the loss, weight gradients inline)
STRETCH_MAX_GRAPHS = 4   # captures kept per net (one per input shape / configuration; least recently replayed goes first)


class _PrivateArena:
    """`with _PrivateArena(buf, nd):` every zero-initialised scratch request of mlp._StatsArena comes out of `buf` (nd doubles of fp64
    region, the rest fp32) instead of the step's arena; the enclosing pass's arena state is restored on exit.  The owner clears buf."""
    FIELDS = ("buf", "nd", "off", "cap32", "off32", "want32", "zeroed32", "depth", "active", "whole_step")

    def __init__(self, buf, nd):
        self.buf, self.nd = buf, nd

    def __enter__(self):
        a = M._StatsArena
        self.saved = {k: getattr(a, k) for k in self.FIELDS}
        a.buf, a.nd, a.off, a.off32, a.want32 = self.buf, self.nd, 0, 0, 0
        a.cap32 = a.zeroed32 = (self.buf.numel() - self.nd) * 2
        a.depth, a.active, a.whole_step = 1, True, True
        return self

    def __exit__(self, *exc):
        a = M._StatsArena
        self.used = (a.off, a.want32)
        for k, v in self.saved.items():
            setattr(a, k, v)
        return False


class _StretchOutputs(dict):
    """What a replayed train step returns: the forward results in the capture's memory pool, which the NEXT replay of that capture
    overwrites.  Reading an entry after that raises instead of handing out another batch's values (clone what has to outlive the step)."""

    def __init__(self, tensors, graph):
        super().__init__(tensors)
        self._graph, self._stamp = graph, graph.replays

    def _check(self, key="them"):
        if self._graph.replays != self._stamp:
            raise M.L.VotenetError("train_step outputs: the stretch graph that holds %r has been replayed for a later step (the tensors a "
                                   "replayed step returns are valid until the next step: clone them to keep them)" % key)

    def __getitem__(self, key):
        self._check(key)
        return super().__getitem__(key)

    def get(self, key, default=None):
        self._check(key)
        return super().get(key, default)

    def items(self):
        self._check()
        return super().items()

    def values(self):
        self._check()
        return super().values()


class StretchGraph:
    """The static stretch of a train step -- feature propagation, voting and the proposal module forward (model.py:48-61,89-93), the
    moving averages, the loss graph (model.py:61-84,141-231), and the backward pass of all of it down to the gradients of the level
    outputs: ~85 launches of 5-40 us on static shapes -- captured ONCE and replayed per step.  What it buys is host time: the host
    enqueued this stretch in 1.7 ms against 1.17 ms of GPU time, i.e. the GPU waited for the host here (tools/probe/stretch_time.py).

    Segments.  The input-gradient chain is captured as FOUR graphs sharing one memory pool, cut where a module's backward ends (proposal |
    voting | fp2 | fp1); the weight-gradient launches of a segment (14 in all) are not captured but recorded as thunks and run launch by
    launch on the weight-gradient stream after their segment's graph, beside the next segment -- where they ran before.  (One graph
    with the weight gradients on a side branch replays its branches concurrently -- tools/probe/graph_branches.py -- but the branch's
    internal stream shared a hardware queue with the geometry prefetch and the graph waited for the sampling kernel: 3.94 -> 5.8 ms per
    step; inline on the one branch: 4.27 ms; tools/probe/stretch_modes.py.)

    Inputs arrive at changing addresses (level outputs from the allocator, geometry from a ring of GeometryGraphs, the batch's ground
    truth): ONE copy launch (votenet_copy_segments) moves them into the graph's fixed input buffers.  Scratch that kernels accumulate
    into comes from a private arena cleared by a fill node of the first graph.  Outputs (the forward results, the losses, d_l2p / d_l3p /
    d_l4p) live in the pool: valid until the next replay."""

    def __init__(self, net, ins, tape_levels, arena_demand):
        dev = net.device
        self.names = list(ins)
        self.fixed = {k: torch.empty_like(v) for k, v in ins.items()}
        nd = (int(arena_demand[0] * 1.25) + 4096 + 1) & ~1
        n32 = int(arena_demand[1] * 1.25) + (1 << 18)
        self.nd = nd
        self.arena = torch.empty(nd + (n32 + 1) // 2, dtype=torch.float64, device=dev)
        self.segments = []  # (graph, [(thunk, tensors) ...]) in replay order
        self.head = net.head  # (the loss launch of every replay reads its nh / ns / nc)
        self._losses = torch.empty(12, dtype=torch.float32, device=dev)
        self._loss_ring = [torch.empty(12, dtype=torch.float32, device=dev) for _ in range(8)]
        self.replays = 0
        self.last_used = 0
        if getattr(net, "_capture_stream", None) is None:
            net._capture_stream = torch.cuda.Stream(device=dev)
        cs = net._capture_stream
        net.store._fresh_wait()  # the wait for this step's W^T copies happens OUTSIDE the graphs (train_step repeats it before a replay)
        self.copy_inputs(ins)    # (the capture executes nothing; this keeps the buffers defined)
        import gc
        torch.cuda.synchronize(dev)
        gc.collect()
        pool = torch.cuda.graph_pool_handle()
        keep, defer = [], []
        cur = [None]

        def begin():
            cur[0] = torch.cuda.CUDAGraph()
            cur[0].capture_begin(pool=pool, capture_error_mode="thread_local")  # thread_local: see GeometryGraph

        def end():
            cur[0].capture_end()
            self.segments.append((cur[0], list(defer)))
            defer.clear()
            cur[0] = None

        def cut():
            if STRETCH_SEGMENTS:
                end()
                begin()

        def loss_hook(out):
            # the loss graph (two launches on the batch's ground truth: its shape -- the padded box count -- varies per batch) is NOT
            # captured: it runs between the forward segment and the first backward segment, into buffers the latter reads at fixed
            # addresses (a carve-out of the private arena: cleared by the first segment's fill)
            from . import loss as VL
            end()
            self.loss_bufs = VL.loss_buffers(out, losses=self._losses)  # (the losses vector: allocated on the caller's stream, below)
            self.loss_at = len(self.segments)  # the loss runs before this segment
            # the cotangents at their fixed addresses: what every replay's loss launch and the launches behind it write
            self.cot, _ = VL.cotangent_views(out["votes_xyz"], out["proposals_xyz"], out["proposals_output"], self.loss_bufs[1])
            begin()
            return self.loss_bufs[0], self.cot
        cs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cs), P.WGRAD.capturing(keep, defer if STRETCH_SEGMENTS else None):
            begin()
            try:
                self.arena.zero_()
                with _PrivateArena(self.arena, nd) as pa:
                    self.out, self.losses, self.grads = net._stretch_body(self.fixed, tape_levels, None, cut=cut, loss_hook=loss_hook)
            finally:
                if cur[0] is not None:
                    end()
        self.arena_used = pa.used
        self.keep = keep

    def copy_inputs(self, ins):
        M.copy_segments([(self.fixed[k], ins[k]) for k in self.names])

    def replay(self, ins, gt, wgrad_stream=None, after_loss=None):
        """One copy launch, then the segments in order -- the loss graph on gt as launches where it belongs --; a segment's
        weight-gradient thunks go to wgrad_stream (None: the current one) behind its graph.  The caller joins the weight-gradient stream
        (pointnet2.wgrad_join) before it reads the gradient bucket.  after_loss(out, gt, losses, self.cot): called behind the loss launch
        (VoteNetHotPath._after_loss: launches between two segments like the loss, no graph is captured again or gets a node)."""
        from . import loss as VL
        self.copy_inputs(ins)
        with P.WGRAD.on(wgrad_stream):
            for i, (graph, thunks) in enumerate(self.segments):
                if i == self.loss_at:
                    # the loss launch is not captured and no captured kernel reads the 12 losses: each replay writes them into the next
                    # vector of a small ring, so a handle to last_losses kept across a few steps still shows ITS step (no copy launch)
                    losses = self._loss_ring[self.replays % len(self._loss_ring)]
                    VL.votenet_loss(self.out, gt, buffers=(losses, self.loss_bufs[1]), head=self.head)
                    if after_loss is not None:
                        after_loss(self.out, gt, losses, self.cot)
                graph.replay()
                if thunks and wgrad_stream is not None:
                    P.WGRAD.hand_over([f for f, _ in thunks])  # (their tensors live in the graphs' pool: nothing for the allocator to track)
                else:
                    for f, _ in thunks:
                        f()
        self.replays += 1
        return _StretchOutputs(self.out, self), losses, self.grads


class _Load:
    """VoteNetHotPath.load, both ways.  net.load(path, strict=True): restore a file written by save() in place, between two train_step
    calls or before predict.  VoteNetHotPath.load(path, device, **kw): a new net built for the file -- its head (NH and the size
    templates of the header; a file without templates has the default ones), its npoints and, from sa1's first kernel, its
    point_features -- with the file restored into it."""

    def __get__(self, net, cls):
        if net is not None:
            return lambda path, strict=True: checkpoint.load(net, path, strict)
        return lambda path, device, strict=True, **kw: checkpoint.load_new(cls, path, device, strict, **kw)


SPLIT_BF16 = True  # fused GEMMs on bf16 x 3 split operands (fp32-accurate products, six bf16 MFMAs per k-step; mlp.SplitImages)


class VoteNetHotPath:
    def __init__(self, device, seed=0, npoints=(2048, 1024, 512, 256), point_features=0, head=None):
        """head: the dataset's detection head (head.HeadConfig: heading bins, classes, size templates); None: the reference's,
        HeadConfig.sunrgbd().  The proposal module's last layer has head.width columns, and the loss, the decode, predict, the monitors
        and the checkpoint header read net.head.  A net has one head for life.
        point_features: 0 -- the reference's network: sa1's input features are the coordinates themselves (model.py:36,39) --, or c in
        1..5: sa1 takes c features per point beside the coordinates (height above the floor, colour, intensity:
        input_pipeline.subsample_augment_features), handed to forward / predict / train_step as feats (B, n, c).  3 + c <= 8, so sa1
        keeps its narrow first layer (csrc/narrow.hip); sa1/conv0/W then has 3 + c input rows."""
        self.device = device
        if head is not None and not isinstance(head, H.HeadConfig):
            raise M.L.InvalidArgumentError("VoteNetHotPath: head must be a head.HeadConfig, got %r" % type(head).__name__)
        self.head = head if head is not None else H.HeadConfig.sunrgbd()
        c = int(point_features)
        if not 0 <= c <= 5:
            raise M.L.InvalidArgumentError("VoteNetHotPath: point_features must be in [0, 5] (sa1's narrow first layer serves 3 + c <= 8 "
                                           "grouped channels), got %r" % (point_features,))
        self.point_features = c
        self.overlap_wgrad = True  # weight gradients on a second stream, next to the input-gradient chain
        self._wgrad_stream = None
        s = P.ParamStore(device)
        self.store = s
        n1, n2, n3, n4 = npoints
        self.sa1 = P.SAModule(s, "sa1", n1, 0.2, 64, c if c else 3, [64, 64, 128], leaf=True)  # model.py:39 (l0_points = xyz, C=3)
        self.sa2 = P.SAModule(s, "sa2", n2, 0.4, 64, 128, [128, 128, 256])  # model.py:41
        self.sa3 = P.SAModule(s, "sa3", n3, 0.8, 64, 256, [128, 128, 256])  # model.py:43
        self.sa4 = P.SAModule(s, "sa4", n4, 1.2, 64, 256, [128, 128, 256])  # model.py:45
        self.fp1 = P.FPModule(s, "fp1", 256, 256, [256, 256])               # model.py:48
        self.fp2 = P.FPModule(s, "fp2", 256, 256, [256, 256])               # model.py:49
        self.voting = P.make_mlp(s, "voting", 259, [256, 256, 259], "fc", last_plain=True)  # model.py:53-57
        self.proposal = P.SAModule(s, "proposal", PROPOSAL_NUM, 0.3, 64, 256, [128, 128, 128],
                                   mlp2=[128, 128, self.head.width])       # model.py:89-93 (79 for the default head)
        s.materialize(seed)
        s.enable_split(SPLIT_BF16)  # forward() refreshes the images at its start, refresh_transposes() those of the copies
        self._geometry = GeometryPrefetch(self._geometry_chain, lambda: self._side_stream(), device, self.proposal.npoint)
        self._prefetched = self._geometry.pool  # (the benchmark's legs and the tools empty / refill the pool through this name)

    def _wgrad_side(self):
        """The weight-gradient stream; None with overlap_wgrad off: weight gradients then run on the chain's own stream."""
        if self.overlap_wgrad and self._wgrad_stream is None:
            self._wgrad_stream = torch.cuda.Stream(device=self.device, priority=WGRAD_PRIORITY)
        return self._wgrad_stream if self.overlap_wgrad else None

    # ---- forward pieces -------------------------------------------------------------
    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device, priority=SIDE_PRIORITY)
        return self._side

    def _sa1_points(self, x, feats, what="forward"):
        """sa1's input features for the batch x: the coordinates themselves (model.py:39), or feats (B, n, point_features) checked."""
        c = getattr(self, "point_features", 0)
        if not c:
            if feats is not None:
                raise M.L.InvalidArgumentError("%s: feats given to a network built without point features (VoteNetHotPath(point_features=0))" % what)
            return x
        if feats is None:
            raise M.L.InvalidArgumentError("%s: this network was built with point_features=%d: pass feats (B, n, %d)" % (what, c, c))
        if not torch.is_tensor(feats) or feats.dtype != torch.float32 or feats.device != x.device or tuple(feats.shape) != tuple(x.shape[:2]) + (c,):
            raise M.L.InvalidArgumentError("%s: feats must be a float32 tensor of shape %s on %s, got %s" % (
                what, tuple(x.shape[:2]) + (c,), x.device, (tuple(feats.shape), feats.dtype, feats.device) if torch.is_tensor(feats) else type(feats)))
        if not feats.is_contiguous():
            raise M.L.InvalidArgumentError("%s: feats must be contiguous" % what)
        return feats

    @staticmethod
    def _feats_kw(feats, next_feats):
        """The feature arguments of an inner call: none at all for a network without point features (the call it always made)."""
        return {} if feats is None and next_feats is None else dict(feats=feats, next_feats=next_feats)

    @staticmethod
    def _pair_next(next_x, next_feats):
        """next_x / next_feats as given to forward() (None, a tensor, or a list of them) -> [(x, feats or None) ...]."""
        xs = list(next_x) if isinstance(next_x, (list, tuple)) else ([next_x] if next_x is not None else [])
        fs = list(next_feats) if isinstance(next_feats, (list, tuple)) else ([next_feats] if next_feats is not None else [])
        if fs and len(fs) != len(xs):
            raise M.L.InvalidArgumentError("next_feats must match next_x: %d batches, %d feature tensors" % (len(xs), len(fs)))
        return list(zip(xs, fs if fs else [None] * len(xs)))

    def _geometry_chain(self, x, g, ev, levels, feats=None):
        """FPS / ball query of `levels`, the proposal layer's FPS (it samples the SEEDS, utils.py:42-43) and both three_nn on
        the current stream; an event per level so that a consumer waits only for what it needs."""
        xyz = x if "sa1" in levels else g["sa1"].new_xyz
        for name in levels:
            # sa1's input features are the coordinates (model.py:39), or the caller's feats (point_features)
            g[name] = getattr(self, name).geometry(xyz, points=(feats if feats is not None else x) if name == "sa1" else None)
            xyz = g[name].new_xyz
            if name == "sa2":  # seeds = l2_xyz: the proposal layer's FPS can start as soon as they exist
                g["prop_fps"] = P.tf_sampling.farthest_point_sample(self.proposal.npoint, xyz)
            if ev is not None:  # None: the chain is being captured (GeometryGraph) -- one event after the replay stands for all
                ev[name] = torch.cuda.Event()
                ev[name].record()
        g["fp1"] = P.FPModule.geometry(g["sa3"].new_xyz, g["sa4"].new_xyz)
        g["fp2"] = P.FPModule.geometry(g["sa2"].new_xyz, g["sa3"].new_xyz)
        if ev is not None:
            ev["fp"] = torch.cuda.Event()
            ev["fp"].record()

    def geometry_ahead(self, x, feats=None):
        """Every FPS / ball query / three_nn of the backbone depends on coordinates only, never on features.
        Level 1 stays on the caller's stream (the sa1 MLP needs it first); levels 2-4, both three_nn and the
        proposal layer's FPS run on a side HIP stream underneath the MLP GEMMs -- they are latency-bound chains on 8
        workgroups and leave the other CUs to the matrix work."""
        main = torch.cuda.current_stream()
        side = self._side_stream()
        g, ev = {}, {}
        g["sa1"] = self.sa1.geometry(x, points=self._sa1_points(x, feats, "geometry_ahead"))
        start = torch.cuda.Event()
        start.record(main)
        with torch.cuda.stream(side):
            side.wait_event(start)
            self._geometry_chain(x, g, ev, ("sa2", "sa3", "sa4"))
        _record_on_main(g, main)
        return g, ev

    def prefetch_geometry(self, next_x, next_feats=None):
        """Software pipelining across steps: the WHOLE coordinate-only part of an upcoming batch (all four FPS + ball queries,
        the proposal FPS, both three_nn) is launched now on a side stream, underneath this step's GEMMs -- FPS is a
        latency chain on one workgroup per scene (8 of 256 CUs), the one thing a step cannot hide from itself because
        everything waits for sa1's centres.  backbone(next_x) picks the result up; every step still computes one full
        geometry.  With GEOMETRY_GRAPHS the chain is one graph launch (GeometryGraph) and its results live in one of GEOMETRY_RING
        fixed sets of buffers: the geometry a pass picked up -- and a tape recorded on it -- is valid until GEOMETRY_RING - 1
        further batches have been prefetched (a training step consumes its tape before the next one starts).  Several batches may be in flight (two prefetch streams, used alternately): a forward-only pass is shorter
        than one geometry chain, so it wants a lookahead of two.  The input pipeline knows the next batches ahead (the
        reference prefetches them through QueueInput, run.py:121-122)."""
        pts = self._sa1_points(next_x, next_feats, "prefetch_geometry")
        self._geometry.prefetch(next_x, pts if pts is not next_x else None)  # (sa1's narrow rows and their moments are built ahead from the features)

    def backbone(self, x, tape=None, overlap=True, next_x=None, feats=None, next_feats=None):
        """model.py:35-50.  x (B,n,3) -> seeds_xyz (B,1024,3), seeds_points (B,1024,256)."""
        lv, g = self.backbone_levels(x, tape, overlap, next_x, feats, next_feats)
        l3_p2 = self.fp1.forward(lv["l3_xyz"], lv["l4_xyz"], lv["l3_p"], lv["l4_p"], tape=tape, geom=g.get("fp1"))
        seeds_p = self.fp2.forward(lv["l2_xyz"], lv["l3_xyz"], lv["l2_p"], l3_p2, tape=tape, geom=g.get("fp2"))
        return lv["l2_xyz"], seeds_p

    def backbone_levels(self, x, tape=None, overlap=True, next_x=None, feats=None, next_feats=None):
        """The four set-abstraction levels of model.py:39-45 (the part of the pass whose row counts depend on the data: the piece layout).
        -> (dict l2_xyz, l2_p, l3_xyz, l3_p, l4_xyz, l4_p; the geometry dict g with the feature-propagation taps "fp1" / "fp2" and the
        proposal layer's "prop_fps" when they were computed ahead).  The current stream has waited for all of g."""
        main = torch.cuda.current_stream()
        pts = self._sa1_points(x, feats)
        feats = pts if pts is not x else None
        pf = self._geometry.take(x, feats)
        if pf is not None:
            g, ev = pf
            main.wait_event(ev["sa1"])
        elif overlap:
            g, ev = self.geometry_ahead(x, feats)
        else:
            g, ev = {}, {}
        nexts = self._pair_next(next_x, next_feats)
        if PREFETCH_AFTER < 0:
            for nx, nf in nexts:
                self.prefetch_geometry(nx, nf)
        overlap = overlap or pf is not None
        def launch_prefetch(after):
            if PREFETCH_AFTER == after:
                for nx, nf in nexts:
                    self.prefetch_geometry(nx, nf)
        l1_xyz, l1_p, _ = self.sa1.forward(x, pts, tape=tape, geom=g.get("sa1"))
        launch_prefetch(1)
        if overlap:
            main.wait_event(ev["sa2"])
        l2_xyz, l2_p, _ = self.sa2.forward(l1_xyz, l1_p, tape=tape, geom=g.get("sa2"))
        launch_prefetch(2)
        if overlap:
            main.wait_event(ev["sa3"])
        l3_xyz, l3_p, _ = self.sa3.forward(l2_xyz, l2_p, tape=tape, geom=g.get("sa3"))
        launch_prefetch(3)
        if overlap:
            main.wait_event(ev["sa4"])
        l4_xyz, l4_p, _ = self.sa4.forward(l3_xyz, l3_p, tape=tape, geom=g.get("sa4"))
        launch_prefetch(4)
        if overlap:
            main.wait_event(ev["fp"])
        return dict(l2_xyz=l2_xyz, l2_p=l2_p, l3_xyz=l3_xyz, l3_p=l3_p, l4_xyz=l4_xyz, l4_p=l4_p), g

    def vote(self, seeds_xyz, seeds_points, tape=None, seeds_copy=None):
        """model.py:53-61: votes = [seeds_xyz, seeds_points] + FC(...).  seeds_copy (b, n, 3): also receives a copy of seeds_xyz (the
        launch that builds the voting input reads those rows anyway; forward() hands the caller that copy when seeds_xyz lives in a
        geometry graph's buffers)."""
        b, n = seeds_xyz.shape[:2]
        rows = b * n
        # [seeds_xyz | seeds_points | 0]: the concat of model.py:53 and the zero padding of the ragged 259-wide input in ONE launch
        # (csrc/glue.hip) instead of cat + fill + copy; votes = x + offset and its split into xyz / features in another one
        pad = (self.voting[0].cin_pad if (self.voting[0].cin_pad and P.PAD_RAGGED_IN) else 259)
        xp = torch.empty((rows, pad), dtype=torch.float32, device=seeds_xyz.device)
        segs = [(xp[:, :3], seeds_xyz.reshape(rows, 3), None), (xp[:, 3:259], seeds_points.reshape(rows, 256), None)]
        if pad > 259:
            segs.append((xp[:, 259:], None, None))
        if seeds_copy is not None:
            segs.append((seeds_copy.view(rows, 3), seeds_xyz.reshape(rows, 3), None))
        M.row_segments(rows, segs)
        x = xp[:, :259]
        recs = []
        off, _ = P.mlp_chain_forward(self.voting, rows, P.DenseInput(x, xp if pad > 259 else None), recs)
        if self.vote_features == "unit":
            from . import unit_votes as UV  # (the only place of a forward pass that loads libvotenet_unitvote.so)
            v_xyz, v_p, norm = UV.unit_votes(x, off[:, :259])  # the same sum, each vote's features divided by their L2 norm: ONE launch too
            if tape is not None:  # (the record owns y and norm: the captured stretch's backward reads them at these addresses)
                tape.append(dict(op="vote", recs=recs, b=b, n=n, unit=dict(y=v_p, norm=norm)))
            return v_xyz.view(b, n, 3), v_p.view(b, n, 256)
        v_xyz = torch.empty((b, n, 3), dtype=torch.float32, device=x.device)
        v_p = torch.empty((b, n, 256), dtype=torch.float32, device=x.device)
        M.row_segments(rows, [(v_xyz.view(rows, 3), x[:, :3], off[:, :3]), (v_p.view(rows, 256), x[:, 3:], off[:, 3:])])
        if tape is not None:
            tape.append(dict(op="vote", recs=recs, b=b, n=n))
        return v_xyz, v_p

    def propose(self, votes_xyz, votes_points, seeds_xyz, tape=None, prop_fps=None):
        """model.py:89-93: SA on votes with FPS on the seeds -> proposals_xyz (B,256,3), output (B,256,79).
        prop_fps: the FPS indices of THESE seeds when they were computed ahead (side stream); None: the seeds are sampled here.
        With enable_proposal_sampling("vote_fps") in force seeds_xyz and prop_fps are not read: the votes themselves are sampled
        (vote_sampling.cluster_votes, one launch), and the tape carries their fps_idx."""
        geom = None
        if self.proposal_sampling == "vote_fps":
            from . import vote_sampling as VSAMP  # (the only place of a pass that loads libvotenet_votesamp.so)
            pr = self.proposal
            geom = pr.geometry(votes_xyz, grouped=VSAMP.cluster_votes(votes_xyz, pr.npoint, pr.radius, pr.nsample))
        elif prop_fps is not None:
            geom = self.proposal.geometry(votes_xyz, fps_idx=prop_fps, ahead=False)  # the votes exist only now
        p_xyz, p_out, _ = self.proposal.forward(votes_xyz, votes_points, sample_xyz=seeds_xyz, tape=tape, geom=geom)
        return p_xyz, p_out

    def forward(self, x, tape=None, next_x=None, feats=None, next_feats=None):
        """next_x: the batch of the NEXT call (or a list of the next few), if known: their geometry is computed underneath this
        pass (prefetch_geometry).  feats (B, n, point_features) float32: sa1's input features, for a network built with them (an
        error otherwise, and an error when missing); next_feats: those of next_x (a list when next_x is one)."""
        self._sa1_points(x, feats)  # (before anything is enqueued)
        self.store.refresh_split()  # bf16 x 3 images of the weights as they are NOW (one launch; no-op unless enable_split())
        M.arena_begin(self.device)  # one fill for all BatchNorm statistics of the pass
        try:
            lv, g = self.backbone_levels(x, tape, next_x=next_x, feats=feats, next_feats=next_feats)
            self._stamp_tape(tape)
            out = self._head_forward(lv, g.get("fp1"), g.get("fp2"), g.get("prop_fps"), tape,
                                     copy_seeds=self._geometry.current is not None)
        finally:
            M.arena_end()
        return out

    def _stamp_tape(self, tape):
        """The geometry of this pass lives in a GeometryGraph's fixed buffers, which a later replay overwrites: the tape is stamped with
        (graph, generation) so that backward() refuses a tape whose geometry is gone."""
        gg = self._geometry.current
        if gg is not None and tape:
            tape[0]["geometry_stamp"] = (gg, gg.generation)

    def _head_forward(self, lv, fp1_geom, fp2_geom, prop_fps, tape, copy_seeds=False):
        """Everything of the forward pass behind the four levels -- feature propagation (model.py:48-49), voting (:53-61), the proposal
        module (:89-93) -- all of it on static shapes.  copy_seeds: seeds_xyz (= sa2's centres) is handed to the caller as a copy (it
        lives in a geometry graph's buffers)."""
        l3_p2 = self.fp1.forward(lv["l3_xyz"], lv["l4_xyz"], lv["l3_p"], lv["l4_p"], tape=tape, geom=fp1_geom)
        seeds_p = self.fp2.forward(lv["l2_xyz"], lv["l3_xyz"], lv["l2_p"], l3_p2, tape=tape, geom=fp2_geom)
        seeds_xyz = lv["l2_xyz"]
        seeds_out = torch.empty_like(seeds_xyz) if copy_seeds else None
        v_xyz, v_p = self.vote(seeds_xyz, seeds_p, tape, seeds_copy=seeds_out)
        p_xyz, p_out = self.propose(v_xyz, v_p, seeds_xyz, tape, prop_fps)
        return dict(seeds_xyz=seeds_out if seeds_out is not None else seeds_xyz, seeds_points=seeds_p, votes_xyz=v_xyz, votes_points=v_p,
                    proposals_xyz=p_xyz, proposals_output=p_out)

    # ---- inference tail: box decode (caller side, torch glue) + 3D NMS (hot path) ------
    def decode_boxes(self, proposals_xyz, proposals_output):
        """model.py:100-129 (votenet_decode_boxes): -> bboxes (B,N,8,3) in get_3d_bbox's corner order, class score (B,N)."""
        from . import loss as VL
        return VL.decode_boxes(proposals_xyz, proposals_output, head=self.head, mean_sizes=self._mean_sizes_device(proposals_xyz.device))

    def _mean_sizes_device(self, device):
        """The head's size templates (nc, 3) float32 on `device`: uploaded once per net, not per decode."""
        t = self.__dict__.get("_mean_sizes_dev")
        if t is None or t.device != device:
            t = self._mean_sizes_dev = torch.from_numpy(self.head.mean_sizes_f32.copy()).to(device).contiguous()
        return t

    # ---- BatchNorm moving averages (training) and the inference-mode BatchNorm built from them ----------------------
    BN_MOMENTUM = 0.9  # Tensorpack BatchNorm default (`momentum=0.9`, epsilon 1e-5); Tensorpack is not in the reference tree

    def _bn_layers(self):
        mods = [self.sa1, self.sa2, self.sa3, self.sa4, self.fp1, self.fp2, self.proposal]
        layers = [L for m in mods for L in m.mlp + (getattr(m, "mlp2", None) or [])] + list(self.voting)
        return [L for L in layers if L.bn]

    def _ema_state(self):
        """name -> (4, c) tensor [unused | unused | moving_mean | moving_var] (the layout of PendingBN.out, so that one
        multi-tensor launch updates every layer); initial values 0 / 1 as TensorFlow initialises them.  Kept OUTSIDE the
        gradient bucket: the moving averages are not trained and never all-reduced (statistics stay per replica)."""
        if getattr(self, "_ema", None) is None:
            self._ema = {}
            st = self.store
            # one flat buffer in the layout of ParamStore.bn_flat (the blocks the consumers' prologues fill): one launch updates all
            self._ema_flat = torch.zeros_like(st.bn_flat) if st.bn_flat is not None else None
            base = st.bn_flat.data_ptr() if st.bn_flat is not None else 0
            for L in self._bn_layers():
                blk = st._bn_views.get(L.name)
                if blk is not None and self._ema_flat is not None:
                    o = (blk.data_ptr() - base) // 4
                    t = self._ema_flat[o:o + 4 * L.cout].view(4, L.cout)
                else:
                    t = torch.zeros((4, L.cout), dtype=torch.float32, device=self.device)
                t[3].fill_(1.0)
                self._ema[L.name] = t
            self._ema_fac = {}
            self._ema_fac_flat = None
            self._ema_fac_by_rows = {}
            self._ema_version = 0
        return self._ema

    @staticmethod
    def _bn_records(tape):
        for t in tape:
            for r in t.get("recs", []) + t.get("recs2", []):
                if r.get("bn_out") is not None:
                    yield r

    def update_moving_averages(self, tape):
        """moving = momentum * moving + (1 - momentum) * batch for the mean and the UNBIASED batch variance (what
        tf.nn.fused_batch_norm hands to the moving-average update) of every BatchNorm layer of this forward pass: two
        multi-tensor launches per step on the (scale | shift | mean | var) blocks the consumers' prologues left behind."""
        ema = self._ema_state()
        recs = list(self._bn_records(tape))
        for r in recs:
            P.check_bn_block(r)  # the blocks read below are the ones THIS tape's pass wrote
        st = self.store
        blocks = st._bn_views
        if self._ema_flat is not None and self._ema_flat.is_cuda and len(recs) == len(blocks) and \
                all(r["bn_out"] is blocks.get(r["layer"].name) for r in recs):
            # every BatchNorm layer of the model ran once and left its block in the persistent buffer: ONE launch (csrc/glue.hip)
            key = tuple(r["rows"] for r in recs)
            if self._ema_fac_flat is None or self._ema_fac_flat[0] != key:
                # One factor tensor per rows key, kept for the life of the model: a StretchGraph captured at another batch shape has
                # this tensor's ADDRESS baked into its votenet_ema_update node, so it must never go back to the allocator while a
                # graph may still be replayed (a handful of shapes x 0.1 MB).
                f = self._ema_fac_by_rows.get(key)
                if f is None:
                    f = torch.full_like(st.bn_flat, 1.0 - self.BN_MOMENTUM)
                    base = st.bn_flat.data_ptr()
                    for r in recs:
                        c, rows = r["layer"].cout, r["rows"]
                        o = (blocks[r["layer"].name].data_ptr() - base) // 4
                        f[o + 3 * c:o + 4 * c] *= rows / max(rows - 1.0, 1.0)
                    self._ema_fac_by_rows[key] = f
                self._ema_fac_flat = (key, f)
            from . import _lib as L_
            with L_.device_guard(self.device):
                L_.check(L_.lib().votenet_ema_update(st.bn_flat.numel(), self.BN_MOMENTUM, L_.ptr(self._ema_flat), L_.ptr(st.bn_flat),
                                                     L_.ptr(self._ema_fac_flat[1]), L_.stream_ptr()))
            self._ema_version += 1
            return
        dst, src, fac = [], [], []
        for r in recs:
            name, rows = r["layer"].name, r["rows"]
            key = (name, rows)
            if key not in self._ema_fac:
                f = torch.full((4, r["layer"].cout), 1.0 - self.BN_MOMENTUM, dtype=torch.float32, device=self.device)
                f[3].mul_(rows / max(rows - 1.0, 1.0))
                self._ema_fac[key] = f
            dst.append(ema[name])
            src.append(r["bn_out"])
            fac.append(self._ema_fac[key])
        if dst:
            torch._foreach_mul_(dst, self.BN_MOMENTUM)
            torch._foreach_addcmul_(dst, src, fac)
            self._ema_version += 1

    def inference_bn(self):
        """name -> mlp.FrozenBN (scale = gamma rsqrt(moving_var + eps), shift = beta - moving_mean scale); rebuilt only when
        the parameters or the moving averages changed since the last call."""
        ema = self._ema_state()
        key = (self._ema_version, self.store.generation, self.store.flat._version)  # generation: bumped by the optimizer's raw-pointer update
        if getattr(self, "_frozen_key", None) != key:
            self._frozen = {}
            for L in self._bn_layers():
                e = ema[L.name]
                sc = L.p("gamma") * torch.rsqrt(e[3] + M.BN_EPS)
                self._frozen[L.name] = M.FrozenBN(torch.stack([sc, L.p("beta") - e[2] * sc]).contiguous())
            self._frozen_key = key
        return self._frozen

    def predict(self, x, iou_threshold=0.25, next_x=None, sync=True, batch_statistics=False, feats=None, next_feats=None,
                protocol="reference", min_points=0, nms_overlap="rotated", nms_measure="iou"):
        """Predict tower of model.py:98-139: forward -> decode -> NMS3D(bboxes, max class logit, objectness, 0.25), every
        BatchNorm in inference mode (moving averages, as the reference's BNReLU under `not is_training`): a scene's
        detections do not depend on its batch-mates.  batch_statistics=True normalises with the current batch instead
        (what a model without trained moving averages needs, e.g. random-init benchmarks).
        next_x: the batch(es) of the next call(s), as in forward().  sync=False: nms_idx stays padded on the device with its
        length in nms_count (no host synchronisation: calls pipeline).  feats / next_feats: as in forward().
        protocol: "reference" is the above.  "per_class" (the VoteNet paper's protocol: detections.PAPER with this call's
        iou_threshold) or a dict of any of iou_threshold / conf_thresh / class_nms / per_class runs detections.class_nms3d in NMS3D's
        place: det_rows / det_offset instead of nms_idx, on the device; that mode never synchronises, whatever `sync` says.
        min_points > 0 (box_points.PAPER_MIN_POINTS = 5 is the paper's remove_empty_box): the points of x inside every decoded box are
        counted on the device (point_counts (B,N) int32 in the result) and a box with fewer is no candidate of the NMS of either
        protocol, which sees a gated copy of the objectness logits; proposals_output stays the network's own.  0: the launches and the
        keys of a call without it.
        nms_overlap: the overlap the per-class NMS suppresses by.  "rotated" is detections.class_nms3d, the rotated-box IoU.  "aabb3d"
        (aabb_nms.PAPER_OVERLAP, the paper's) and "bev" run aabb_nms.class_nms_aabb in its place, on the same boxes and the same,
        possibly gated, objectness: the overlap of the boxes' axis-aligned hulls, in 3D or on the ground plane; the same keys.
        nms_measure: "iou", or "over_later" (the paper's use_old_type_nms: intersection over the later box) with those two.  The
        reference's protocol has the rotated-box IoU only."""
        from . import aabb_nms, detections, tf_nms3d
        params = detections.protocol_params(protocol, iou_threshold)
        aabb_nms.check_overlap(protocol, nms_overlap, nms_measure, "predict")
        if isinstance(min_points, bool) or not isinstance(min_points, int) or min_points < 0:
            raise M.L.InvalidArgumentError("predict: min_points must be an int >= 0, got %r" % (min_points,))
        self._sa1_points(x, feats, "predict")
        if not batch_statistics and self._ema_state() is not None and self._ema_version == 0 and not getattr(self, "_warned_ema", False):
            import warnings
            warnings.warn("VoteNetHotPath.predict: no training step has updated the BatchNorm moving averages yet (mean 0, variance 1): "
                          "pass batch_statistics=True for a freshly initialised model", stacklevel=2)
            self._warned_ema = True
        with P.frozen_bn(None if batch_statistics else self.inference_bn()):
            out = self.forward(x, next_x=next_x, **self._feats_kw(feats, next_feats))
        boxes, score = self.decode_boxes(out["proposals_xyz"], out["proposals_output"])
        objectness = lambda: out["proposals_output"][..., :2].contiguous()
        gate = {}
        if min_points > 0:  # (the only place that loads libvotenet_boxpts.so)
            from . import box_points
            gate = dict(point_counts=box_points.box_point_counts(boxes, x))
            gated = box_points.gate_objectness(objectness(), gate["point_counts"], min_points)
            objectness = lambda: gated
        if params is not None:
            cls = out["proposals_output"][..., self.head.sem].contiguous()
            if nms_overlap == "rotated":
                det = detections.class_nms3d(boxes, objectness(), cls, **params)
            else:  # (the only place that loads libvotenet_aabb.so)
                det = aabb_nms.class_nms_aabb(boxes, objectness(), cls, overlap=nms_overlap, measure=nms_measure, **params)
            return dict(bboxes=boxes, scores=score, class_scores=cls, **gate, **det, **out)
        keep = tf_nms3d.NMS3D(boxes, score, objectness(), iou_threshold, padded=not sync)
        extra = dict(gate) if sync else dict(nms_count=keep[1], **gate)
        return dict(bboxes=boxes, scores=score, nms_idx=keep if sync else keep[0], class_scores=out["proposals_output"][..., self.head.sem].contiguous(),
                    **extra, **out)

    # ---- backward / training --------------------------------------------------------
    def make_cotangents(self, b, seed=0):
        """Fixed upstream gradients (tests of the backward pass, scenes without ground truth): d loss / d proposals_output
        (B,256,79) and d loss / d votes_xyz (B,1024,3).  Training uses the loss graph instead (train_step(gt=...))."""
        g = torch.Generator(device="cpu").manual_seed(1234 + seed)
        n_seed = self.sa2.npoint
        return dict(proposals_output=(torch.randn(b, PROPOSAL_NUM, self.head.width, generator=g) / (b * PROPOSAL_NUM)).to(self.device),
                    votes_xyz=(torch.randn(b, n_seed, 3, generator=g) / (b * n_seed)).to(self.device))

    def backward(self, tape, cot):
        """Reverse sweep over the tape of forward(); parameter gradients accumulate into store.grad."""
        self.check_tape(tape)
        M.arena_begin(self.device)  # one fill for all BatchNorm-backward reductions of the pass
        try:
            with P.WGRAD.on(self._wgrad_side()):
                self._backward(tape, cot)
                P.wgrad_join()  # the optimizer (and the next pass's arena fill) come after every weight gradient
        finally:
            M.arena_end()

    @staticmethod
    def check_tape(tape):
        """A tape recorded on prefetched geometry reads a GeometryGraph's buffers (idx, pts_cnt, the compact rows, fps_idx, the piece
        layouts): valid until that graph replays for another batch -- GEOMETRY_RING - 1 further prefetches.  Raises instead of
        differentiating through another batch's neighbour lists."""
        stamp = tape[0].get("geometry_stamp") if tape else None
        if stamp is not None and stamp[0].generation != stamp[1]:
            raise M.L.VotenetError("backward(): the geometry buffers this tape was recorded on have been overwritten by %d later prefetch(es) "
                                   "(model.GeometryGraph; a tape on prefetched geometry is valid until GEOMETRY_RING - 1 = %d further "
                                   "batches have been prefetched)" % (stamp[0].generation - stamp[1], GEOMETRY_RING - 1))

    def _backward(self, tape, cot):
        d_l2p, d_l3p, d_l4p = self._head_backward(tape[4:8], cot)
        self._levels_backward(tape[:4], d_l2p, d_l3p, d_l4p)

    def _head_backward(self, tail, cot, cut=None):
        """The backward pass of _head_forward (proposal, voting, fp2, fp1): -> the gradients of the level outputs d_l2p, d_l3p, d_l4p.
        cut: called where a module's backward ends (StretchGraph cuts its segments there)."""
        fp1, fp2, vote, prop = tail
        cut = cut if cut is not None else (lambda: None)
        # proposal layer: gradients reach the vote features AND the vote xyz (grouped xyz, gathered centres)
        d_vp, d_vx = self.proposal.backward(prop, cot["proposals_output"], need_feat_grad=True, need_xyz_grad=True)
        P.wgrad_flush()  # the module's weight gradients go to their stream together, underneath the next module's chain
        cut()
        if cot.get("proposals_xyz") is not None:  # proposals_xyz = gather(votes_xyz, fps_idx), utils.py:42-47: accumulated in place
            d_vx = P.tf_sampling.gather_point_grad_raw(d_vx.shape[1], prop["fps_idx"], cot["proposals_xyz"], into=d_vx.contiguous())
        # voting: votes = x + FC(x), x = [seeds_xyz, seeds_points].  d_votes = [d_vx (+ the loss's pull on the votes) | d_vp | 0]: the
        # concat, the sum and the zero padding of the ragged 259-wide layer in ONE launch (csrc/glue.hip)
        b, n = vote["b"], vote["n"]
        rows = b * n
        last = self.voting[-1]
        padw = last.cout_pad if last.cout_pad else 259
        d_votes_p = torch.empty((rows, padw), dtype=torch.float32, device=d_vp.device)
        cv = cot.get("votes_xyz")
        segs = [(d_votes_p[:, :3], d_vx.reshape(rows, 3), cv.reshape(rows, 3) if cv is not None else None),
                (d_votes_p[:, 3:259], d_vp.reshape(rows, 256), None)]
        if padw > 259:
            segs.append((d_votes_p[:, 259:], None, None))
        if vote.get("unit") is not None:
            # unit-length vote features: d_vp is the gradient of y = u / |u|; the same buffer receives the gradient of the sum u,
            # [d_vx + cot | (d_vp - y (y . d_vp)) / |u| | 0], in ONE launch too -- everything below consumes it as it always did
            from . import unit_votes as UV
            UV.unit_votes_backward(d_vx, cv, d_vp, vote["unit"]["y"], vote["unit"]["norm"], d_votes_p)
        else:
            M.row_segments(rows, segs)
        d_votes = d_votes_p[:, :259]
        d_in = P.mlp_chain_backward(vote["recs"], d_votes, "plain", need_input_grad=True, g_padded=d_votes_p if padw > 259 else None)
        P.wgrad_flush()
        cut()
        # d x = d_votes + d_in; only its feature columns go on (the seeds' coordinates carry no gradient in the backbone)
        d_seeds_p = torch.empty((b, n, 256), dtype=torch.float32, device=d_vp.device)
        M.row_segments(rows, [(d_seeds_p.view(rows, 256), d_votes[:, 3:], d_in[:, 3:259])])
        # feature propagation
        d_l2p, d_l3p2 = self.fp2.backward(fp2, d_seeds_p)
        P.wgrad_flush()
        cut()
        d_l3p, d_l4p = self.fp1.backward(fp1, d_l3p2)
        P.wgrad_flush()
        return d_l2p, d_l3p, d_l4p

    def _levels_backward(self, levels, d_l2p, d_l3p, d_l4p):
        """The backward pass of the four levels, sa4 ... sa1 (xyz carries no gradient in the backbone: the cloud is the input)."""
        sa1, sa2, sa3, sa4 = levels
        self._grams_early(dict(sa1=sa1, sa2=sa2, sa3=sa3, sa4=sa4))
        g3, _ = self.sa4.backward(sa4, d_l4p)
        P.wgrad_flush()
        d_l3p = P.add_rows(d_l3p, g3)
        g2, _ = self.sa3.backward(sa3, d_l3p)
        P.wgrad_flush()
        d_l2p = P.add_rows(d_l2p, g2)
        # every gradient of sa3 ... proposal (the tail of the flat bucket) is enqueued: its all-reduce runs on the
        # communication stream underneath the backward pass of sa2 and sa1 (dp.GradSync; a no-op on one GPU)
        if getattr(self, "_gsync", None) is not None:
            self._gsync.start_tail([P.WGRAD.stream])
        # inline_wgrad_tail (experiment, default off): the weight gradients of the two largest modules on the MAIN stream -- by the time
        # their backward runs the next batch's sampling kernel has finished, and pairs of GPU-filling kernels gain nothing from two streams
        with P.WGRAD.on(None if getattr(self, "inline_wgrad_tail", INLINE_WGRAD_TAIL) else P.WGRAD.stream):
            g1, _ = self.sa2.backward(sa2, d_l2p)
            P.wgrad_flush()
            with P.WGRAD.fine():  # the last module: nothing follows to hide its weight gradients under, so they start layer by layer
                self.sa1.backward(sa1, g1, need_feat_grad=False)

    # ---- the static stretch of a train step as one HIP graph (StretchGraph) -------------------------------------------------------
    def _stretch_eligible(self, x, cot, gt):
        # (per-launch events around the GEMMs -- mlp.PROFILE_EVENTS -- need the launches; events around the sampling / ball-query launches
        # -- bench.py's roofline legs -- concern the geometry chain only: a captured stretch still replays, see _train_step_stretch)
        return bool(STRETCH_GRAPH and gt is not None and cot is None and x.is_cuda and not M.DETERMINISTIC and PREFETCH_AFTER < 5
                    and M.PROFILE_EVENTS is None and P._FROZEN.table is None and not getattr(self, "_stretch_off", False)
                    and not torch.cuda.is_current_stream_capturing())

    @staticmethod
    def _stretch_inputs(lv, g):
        """name -> tensor: everything the captured segments read that lives at an address of this step's making (the ground truth is
        not among them: the loss runs as launches between two segments)."""
        ins = dict(lv)
        for name in ("fp1", "fp2"):
            idx = g[name].idx
            ins[name + "_idx"], ins[name + "_w"] = idx, g[name].weight
            inv = getattr(idx, "_inv", None)
            if inv is not None:
                ins[name + "_inv0"], ins[name + "_inv1"] = inv
        ins["prop_fps"] = g["prop_fps"]
        return ins

    def _stretch_body(self, I, tape_levels, wgrad_stream, gt=None, cut=None, loss_hook=None, copy_seeds=False):
        """The stretch on the tensors of I (StretchGraph captures this on its fixed buffers; the first step of a shape runs it eagerly):
        forward head, moving averages, loss (on gt, or through loss_hook(out) -> (losses, cotangents) when captured), backward head.
        -> (out, losses, (d_l2p, d_l3p, d_l4p))."""
        from . import loss as VL

        def geom(name):
            idx = I[name + "_idx"]
            if name + "_inv0" in I:
                idx._inv = (I[name + "_inv0"], I[name + "_inv1"])
            return P.FPGeometry(idx, I[name + "_w"])
        tail = []
        lv = {k: I[k] for k in ("l2_xyz", "l2_p", "l3_xyz", "l3_p", "l4_xyz", "l4_p")}
        out = self._head_forward(lv, geom("fp1"), geom("fp2"), I["prop_fps"], tail, copy_seeds=copy_seeds)
        self.update_moving_averages(list(tape_levels) + tail)
        losses, cot = loss_hook(out) if loss_hook is not None else VL.votenet_loss(out, gt, head=self.head)
        if loss_hook is None:  # (captured: the loss and what runs behind it are launches of every replay, StretchGraph.replay)
            self._after_loss(out, gt, losses, cot)
        with P.WGRAD.on(wgrad_stream):
            grads = self._head_backward(tail, cot, cut=cut)
            if cut is None:
                P.wgrad_join()
        self._stretch_tail = tail  # (kept: the records own the tensors the captured kernels read)
        return out, losses, grads

    def _train_step_stretch(self, x, gt, tape, next_x, feats=None, next_feats=None):
        """train_step's middle with the stretch replayed as a graph: levels forward (launches: their row counts are the data's) ->
        ONE copy launch + ONE graph launch -> levels backward (launches)."""
        self.store.refresh_split()
        lv, g = self.backbone_levels(x, tape, next_x=next_x, feats=feats, next_feats=next_feats)
        self._stamp_tape(tape)
        self._keep_seed_levels(tape)
        self._grams_ahead(tape)
        if not all(k in g for k in ("fp1", "fp2", "prop_fps")):  # geometry computed without the taps (overlap off): the launch path
            g = dict(g)
            g.setdefault("fp1", P.FPModule.geometry(lv["l3_xyz"], lv["l4_xyz"]))
            g.setdefault("fp2", P.FPModule.geometry(lv["l2_xyz"], lv["l3_xyz"]))
            g.setdefault("prop_fps", P.tf_sampling.farthest_point_sample(self.proposal.npoint, lv["l2_xyz"]))
        ins = self._stretch_inputs(lv, g)
        key = tuple((k, tuple(v.shape), v.dtype) for k, v in ins.items()) + (P.HALF_GROUPS, P.ASSEMBLE_FIRST, P.ASSEMBLE_INLINE, P.POOL_GRAM_BACKWARD, P.ASSEMBLED_DECOMPOSED,
                                                                             self.overlap_wgrad, STRETCH_SEGMENTS, M.SPLIT_K, M.COEF_TAIL, P.WGRAD_BATCH, P.POOL_IN_EPILOGUE,
                                                                             self.store.split, bool(getattr(self, "inline_wgrad_tail", INLINE_WGRAD_TAIL)), M.FORWARD_H2, M.ADHOC_H2,
                                                                             self.proposal_sampling or "seed_fps", self.vote_features or "sum", M.CONFIG_EPOCH)  # (the modes before the epoch: dkey below carries them too)
        graphs = self.__dict__.setdefault("_stretch_graphs", {})
        sg = graphs.get(key)
        self._gsync.begin()
        if sg is None:
            dkey = key[:-1]  # what the stretch asks of the arena does not depend on library switches: one measurement serves
            demand = self.__dict__.setdefault("_stretch_demand", {}).get(dkey)
            geometry_events = P.tf_sampling.PROFILE_EVENTS is not None or P.tf_grouping.PROFILE_EVENTS is not None
            if demand is None or geometry_events:
                # first step of this shape: the stretch launch by launch, measuring what it asks of the arena (also while somebody records
                # events around the geometry launches: the proposal module's ball query sits in the stretch -- no capture then)
                a = M._StatsArena
                off0, want0 = a.off, a.want32
                self.check_tape(tape)
                # (launch by launch on the live inputs: seeds_xyz would alias sa2's centres inside a GeometryGraph buffer that a later
                # prefetch overwrites -- handed out as a copy, as forward() does)
                out, self.last_losses, grads = self._stretch_body(ins, tape, self._wgrad_side(), gt=gt,
                                                                  copy_seeds=self._geometry.current is not None)
                self._stretch_demand[dkey] = (a.off - off0, a.want32 - want0)
                self._backward_levels_pass(tape, grads)
                return out
            while len(graphs) >= STRETCH_MAX_GRAPHS:  # the least recently replayed graph (and its pool) goes
                graphs.pop(min(graphs, key=lambda k: graphs[k].last_used))
            sg = graphs[key] = StretchGraph(self, ins, tape, demand)
        self._stretch_clock = getattr(self, "_stretch_clock", 0) + 1
        sg.last_used = self._stretch_clock
        self.store._fresh_wait()
        out, self.last_losses, grads = sg.replay(ins, gt, self._wgrad_side(),  # (a vector of the graph's ring: rewritten eight replays later)
                                                 after_loss=self._after_loss)
        self._ema_version += 1  # (the replay ran votenet_ema_update: inference_bn() must not serve a table built before it)
        self._backward_levels_pass(tape, grads)
        return out

    def _grams_early(self, levels):
        """GRAM_EARLY: the Gram matrices of the named levels (forward data only) go to the weight-gradient stream at the START of the
        levels' backward pass instead of beside their own level's backward GEMMs.  The step's tail is sa1's backward, where the chain
        (arg-max scatter, dense input gradient, narrow input gradient: 0.31 ms alone) and the weight-gradient stream (Gram matrix, sparse
        gather, narrow weight gradient: 0.28 ms alone) run beside each other at 0.45 ms: sa1's matrix ahead takes a third of that
        stream's tail away and runs beside sa4's / sa3's smaller kernels instead."""
        if not GRAM_EARLY or M.DETERMINISTIC or P.WGRAD.stream is None:
            return
        todo = [levels[n]["recs"][-1] for n in GRAM_EARLY if n in levels]
        todo = [r for r in todo if r.get("gram_form") and r.get("in_affine") is not None and "gram_ahead" not in r]
        if not todo:
            return

        def run():
            for r in todo:
                r["gram_ahead"] = M.gram(r["x"], r["in_affine"][:2], r["in_relu"], half=r.get("half"))
        P.on_wgrad_stream(run, *[r["x"] for r in todo])
        P.wgrad_flush()

    def _grams_ahead(self, tape):
        """The Gram matrix a^T a of a pooled layer's input (pool_bwd.hip) depends on forward data only.  Launched here -- behind the
        levels' forward pass, on the weight-gradient stream -- the four of sa1..sa4 (0.27 ms of kernels) run under the static stretch,
        whose own kernels leave most of the GPU idle, instead of beside the backward GEMMs of their levels."""
        if not GRAMS_AHEAD or M.DETERMINISTIC or not self.overlap_wgrad or not torch.cuda.is_available():
            return
        todo = [t["recs"][-1] for t in tape[:4] if t.get("op") == "sa" and t["recs"][-1].get("gram_form") and t["recs"][-1].get("in_affine") is not None]
        if not todo:
            return

        def run():
            for r in todo:
                r["gram_ahead"] = M.gram(r["x"], r["in_affine"][:2], r["in_relu"], half=r.get("half"))
        with P.WGRAD.on(self._wgrad_side()):
            P.on_wgrad_stream(run, *[r["x"] for r in todo])

    def _backward_levels_pass(self, tape, grads):
        """backward() for the four levels only (the head's gradients given)."""
        self.check_tape(tape)
        M.arena_begin(self.device)
        try:
            with P.WGRAD.on(self._wgrad_side()):
                self._levels_backward(tape[:4], *grads)
                P.wgrad_join()
        finally:
            M.arena_end()

    def drop_graphs(self):
        """Forget every captured graph (geometry rings, stretch graphs): after a configuration change the captures do not key on
        (library debug switches, hand-edited module state)."""
        self.__dict__.pop("_stretch_graphs", None)
        self.__dict__.pop("_stretch_demand", None)
        self._geometry.drop()

    # ---- training summaries on the device (monitors.py): off unless asked for --------------------------------------------------
    monitors = None          # a monitors.Monitors while enable_monitors is in force
    last_accuracies = None   # (2,) f32 on the device: obj_accuracy, sem_accuracy of the last monitored step

    def enable_monitors(self, window=100, tensors_every=0):
        """From now on every train_step(..., gt=...) runs one more launch behind its loss launch: obj_accuracy / sem_accuracy of the step
        (model.py:164-166, 215-216) into self.last_accuracies and, with the total cost, into a device ring of `window` rows (run.py:127);
        every tensors_every-th step (0: never) two more behind the optimizer: rms, extrema and histogram of every parameter and gradient
        tensor (model.py:236, 250).  Nothing is read back until self.monitors.read().  A step with fixed cotangents (cot=) has no loss
        and is not monitored.  -> the Monitors object."""
        from . import monitors
        self.monitors = monitors.Monitors(self, window, tensors_every)
        self.last_accuracies = None
        return self.monitors

    def disable_monitors(self):
        """Back to the launches of an unmonitored step (the default)."""
        self.monitors = None
        self.last_accuracies = None

    # ---- vote supervision as in the VoteNet paper (vote_supervision.py): off unless asked for ------------------------------------
    vote_supervision = None  # the mode while enable_vote_supervision is in force (vote_supervision.MODES); a setting of the run, not checkpoint state

    def enable_vote_supervision(self, mode="paper"):
        """From now on every train_step(..., gt=...) supervises the votes by `mode`.  "paper": one more launch behind the loss launch
        (vote_supervision.paper_vote_loss) overwrites the whole vote cotangent, last_losses[1] (vote_reg_loss) and re-forms
        last_losses[0]: a seed votes for the centres of the boxes that contain it, up to three targets, the closest is charged, the
        mean is over the supervised seeds.  "reference": the rule of votenet_loss itself, no launch.  Everything else of the step --
        the other ten loss values, the other two cotangents, the graphs (none is captured again), the guard, the data-parallel
        exchange, the optimizer -- is what it was.  A step with fixed cotangents (cot=) has no loss and is not touched."""
        from . import vote_supervision as VS
        if mode not in VS.MODES:
            raise M.L.InvalidArgumentError("enable_vote_supervision: mode must be one of %s, got %r" % (", ".join(VS.MODES), mode))
        if mode == "paper" and self.instance_votes == "instance":
            raise M.L.InvalidArgumentError("enable_vote_supervision: \"paper\" and enable_instance_votes() both write the vote term: "
                                           "disable_instance_votes() first")
        self.vote_supervision = mode

    def disable_vote_supervision(self):
        """Back to the launches of a step with the reference's vote supervision (the default)."""
        self.vote_supervision = None

    # ---- vote supervision from instance labels (instance_votes.py): off unless asked for -----------------------------------------
    instance_votes = None  # the mode while enable_instance_votes is in force (instance_votes.MODES); a setting of the run, not checkpoint state

    def enable_instance_votes(self, mode="instance"):
        """From now on every train_step(..., gt=...) supervises the votes by `mode`.  "instance": one more launch behind the loss launch
        (instance_votes.instance_vote_loss, in the place the paper-vote launch has) overwrites the whole vote cotangent, last_losses[1]
        (vote_reg_loss) and re-forms last_losses[0]: a seed votes for the centre of the box of ITS OWN instance, a seed on an unlabelled
        point is not supervised, the mean is over the supervised seeds.  gt["point_box"] (B, n points) int32 on the device is required
        then (input_pipeline.build_batch_from_labels(..., point_box=True)); the link from a seed to its cloud point is the fps_idx of
        sa1 and sa2, which the step keeps from its tape.  "reference": the rule of votenet_loss itself, no launch.  Everything else of
        the step -- the other ten loss values, the other two cotangents, the graphs (none is captured again), the guard, the
        data-parallel exchange, the optimizer -- is what it was.  "instance" and enable_vote_supervision("paper") exclude each other
        (both write the vote term).  A step with fixed cotangents (cot=) has no loss and is not touched."""
        from . import instance_votes as IV
        if mode not in IV.MODES:
            raise M.L.InvalidArgumentError("enable_instance_votes: mode must be one of %s, got %r" % (", ".join(IV.MODES), mode))
        if mode == "instance" and self.vote_supervision == "paper":
            raise M.L.InvalidArgumentError("enable_instance_votes: enable_vote_supervision(\"paper\") is in force and both write the vote "
                                           "term: disable_vote_supervision() first")
        self.instance_votes = mode

    def disable_instance_votes(self):
        """Back to the launches of a step with the reference's vote supervision (the default)."""
        self.instance_votes = None
        self.__dict__.pop("_seed_levels", None)

    def _check_point_box(self, x, gt):
        """train_step with the instance mode on: gt must carry the cloud's box rows (before anything is zeroed or enqueued)."""
        pb = gt.get("point_box") if hasattr(gt, "get") else None
        want = tuple(x.shape[:2])
        if not (torch.is_tensor(pb) and pb.dtype == torch.int32 and pb.device == x.device and tuple(pb.shape) == want and pb.is_contiguous()):
            raise M.L.InvalidArgumentError(
                "train_step: enable_instance_votes() is in force: gt[\"point_box\"] must be a contiguous int32 tensor of shape %s on %s "
                "(input_pipeline.build_batch_from_labels(..., point_box=True)), got %s"
                % (want, x.device, (tuple(pb.shape), pb.dtype, pb.device) if torch.is_tensor(pb) else type(pb).__name__))

    def _keep_seed_levels(self, tape):
        """The link from a seed to the cloud point it is: the fps_idx of the tape's first two sa records (sa1's picks into the cloud,
        sa2's picks into sa1's centres), kept on the net for the launch behind the loss (_after_loss's signature stays what it was).
        With prefetched geometry both tensors live in a GeometryGraph's buffers, which that graph's next replay overwrites.  They are
        still THIS step's when the launch runs: the launch is enqueued on the main stream inside this step; the graph is next replayed
        for the batch GEOMETRY_RING = 3 prefetches on (GeometryPrefetch.next_graph never hands out the graph that serves the pass being
        enqueued), that prefetch is issued from a later step, and its stream first waits for an event recorded on the main stream
        then -- behind every launch of this step.  The graph and its generation are kept beside them and compared at the launch."""
        if self.instance_votes != "instance":
            return
        sa = [t for t in tape[:2] if t.get("op") == "sa" and t.get("fps_idx") is not None]
        if len(sa) != 2:
            raise M.L.VotenetError("enable_instance_votes: the tape does not start with sa1's and sa2's records")
        gg = self._geometry.current
        self._seed_levels = (sa[0]["fps_idx"], sa[1]["fps_idx"], gg, gg.generation if gg is not None else 0)

    # ---- objectness and centre supervision as in the VoteNet paper (proposal_supervision.py): off unless asked for ----------------
    proposal_supervision = None  # the mode while enable_proposal_supervision is in force (proposal_supervision.MODES); a setting of the run, not checkpoint state

    def enable_proposal_supervision(self, mode="paper"):
        """From now on every train_step(..., gt=...) supervises objectness and centre by `mode`.  "paper": one more launch behind the
        loss launch (proposal_supervision.paper_proposal_loss; after the paper-vote launch when that mode is on too, before the
        monitors') overwrites columns 0..4 of the proposals_output cotangent, the whole proposals_xyz cotangent, last_losses[2]
        (obj_cls_loss) and last_losses[3] (center_loss) and re-forms last_losses[9] and last_losses[0]: one cross-entropy weighted 0.2 /
        0.8 over all proposals outside the grey zone, and a Chamfer distance between the predicted and the real ground-truth centres.
        "reference": the rule of votenet_loss itself, no launch.  Everything else of the step -- the other loss values, the other
        columns, the vote cotangent, the graphs (none is captured again), the guard, the data-parallel exchange, the optimizer -- is
        what it was.  A step with fixed cotangents (cot=) has no loss and is not touched."""
        from . import proposal_supervision as PS
        if mode not in PS.MODES:
            raise M.L.InvalidArgumentError("enable_proposal_supervision: mode must be one of %s, got %r" % (", ".join(PS.MODES), mode))
        self.proposal_supervision = mode

    def disable_proposal_supervision(self):
        """Back to the launches of a step with the reference's objectness and centre terms (the default)."""
        self.proposal_supervision = None

    # ---- the launches behind the loss: the launch path, the eager first step of a shape and every replay come here --------------------
    def _after_loss(self, out, gt, losses, cot):
        """Behind votenet_loss(out, gt) -> losses, cot and before the backward pass reads cot, in this order, each only while its mode is on
        (a mode that is off imports and loads nothing): the paper's vote term or the instance labels' (they exclude each other), the
        paper's objectness and centre terms (all overwrite their parts of cot and losses in place), the monitors' accuracy launch (last:
        its ring records the re-formed total)."""
        if self.vote_supervision == "paper":
            from . import vote_supervision as VS  # (the only place of a train step that loads libvotenet_votesup.so)
            work, supervised = self._loss_tail_buffers(VS, out["votes_xyz"].shape[0], 1)
            VS.paper_vote_loss(out, gt, losses, d_votes=cot["votes_xyz"], supervised=supervised, work=work)
        if self.instance_votes == "instance":
            from . import instance_votes as IV  # (the only place of a train step that loads libvotenet_instvote.so)
            idx1, idx2, gg, generation = self._seed_levels  # (this step's: _keep_seed_levels)
            if gg is not None and gg.generation != generation:
                raise M.L.VotenetError("instance votes: the geometry buffers that hold this step's fps_idx have been overwritten by a later prefetch")
            work, counts = self._loss_tail_buffers(IV, out["votes_xyz"].shape[0], 2)
            IV.instance_vote_loss(out, gt, losses, (idx1, idx2), d_votes=cot["votes_xyz"], counts=counts, work=work)
        if self.proposal_supervision == "paper":
            from . import proposal_supervision as PS  # (the only place of a train step that loads libvotenet_propsup.so)
            work, counts = self._loss_tail_buffers(PS, out["proposals_xyz"].shape[0], 3)
            PS.paper_proposal_loss(out, gt, losses, d_xyz=cot["proposals_xyz"], d_out=cot["proposals_output"], counts=counts, work=work,
                                   head=self.head)
        if self.monitors is not None:
            self.last_accuracies = self.monitors.after_loss(out, gt, losses)

    def _loss_tail_buffers(self, mod, b, ncounts):
        """-> (workspace, count tensor) of supervision module mod for b scenes; zeroed once, every launch leaves the workspace zero."""
        work = self.__dict__.setdefault("_loss_tail_work", {})  # (a net that never ran a paper mode has none)
        if (mod, b) not in work:
            work[mod, b] = (mod.workspace(b, self.device), torch.empty(ncounts, dtype=torch.int32, device=self.device))
        return work[mod, b]

    # ---- proposals sampled on the votes as in the VoteNet paper (vote_sampling.py): off unless asked for ---------------------------
    proposal_sampling = None  # the mode while enable_proposal_sampling is in force (vote_sampling.MODES); a setting of the run, not checkpoint state

    def enable_proposal_sampling(self, mode="vote_fps"):
        """From now on every pass -- forward, predict, evaluate, train_step (launch path and replayed graphs) and their backward --
        picks the proposal module's cluster centres by `mode`.  "vote_fps": farthest-point sampling on the VOTES, the paper's rule: one
        launch (vote_sampling.cluster_votes) between the voting MLP and the proposal MLP samples the votes, gathers the centres and
        runs the ball query; propose() no longer reads seeds_xyz or prop_fps, and the tape carries the votes' fps_idx, so a
        proposals_xyz cotangent is scattered to the sampled votes.  "seed_fps": the reference's rule (the votes of the seeds that
        farthest-point sampling picks among the seeds), the default, no launch of this library.
        The geometry chain, its ring and its prop_fps stay what they were: with the mode on the seeds' sampling still runs a batch
        ahead on the side stream and is not read -- the seeds are in farthest-point order, so it is the confirmed-prefix case and runs
        no round --, and the captured geometry graphs need no second form.  The stretch graphs key on the mode: the first step in a
        new mode runs launch by launch, each mode keeps its own capture, switching back replays the old one.
        The mode is a setting of the run, not checkpoint state, and it applies to inference as much as to training: evaluate a network
        under the mode it was trained in.  "vote_fps" on a network whose seed count or proposal shape the kernel refuses
        (vote_sampling.supported) is an InvalidArgumentError here, not in the step."""
        from . import vote_sampling as VSAMP
        if mode not in VSAMP.MODES:
            raise M.L.InvalidArgumentError("enable_proposal_sampling: mode must be one of %s, got %r" % (", ".join(VSAMP.MODES), mode))
        if mode == "vote_fps":
            n, pr = self.sa2.npoint, self.proposal
            if pr.knn or pr.group_all or not VSAMP.supported(n, pr.npoint, pr.nsample):
                raise M.L.InvalidArgumentError(
                    "enable_proposal_sampling: vote_fps takes 1 to %d votes, 1 to %d clusters and 1 to %d votes per ball-query cluster; "
                    "this network has %d seeds and a proposal module of npoint %r, nsample %r, knn %r, group_all %r"
                    % (VSAMP.MAX_N, VSAMP.MAX_M, VSAMP.MAX_NSAMPLE, n, pr.npoint, pr.nsample, pr.knn, pr.group_all))
        self.proposal_sampling = mode

    def disable_proposal_sampling(self):
        """Back to the launches of a pass with the reference's proposal sampling (the default)."""
        self.proposal_sampling = None

    # ---- unit-length vote features as in the authors' VoteNet (unit_votes.py): off unless asked for --------------------------------------
    vote_features = None  # the mode while enable_vote_features is in force (unit_votes.MODES); a setting of the run, not checkpoint state

    def enable_vote_features(self, mode="unit"):
        """From now on every pass -- forward, predict, evaluate, train_step (launch path and replayed graphs) and their backward --
        forms the vote features by `mode`.  "unit": each vote's 256 features (seed features + the voting MLP's residual) divided by
        their L2 norm, as the authors' VoteNet does before its proposal module; the reference, and the default here, hand the sum on
        as it is.  vote() runs unit_votes.unit_votes in the place of its last glue launch and the backward of the head runs
        unit_votes.unit_votes_backward in the place of the glue launch that builds the voting chain's output gradient: two launches
        for two launches, the tape's "vote" record carries the unit features and the norms between them.  votes_xyz, the voting
        chain and everything behind its backward are what they were.  No epsilon, as in the authors' code: a vote whose features
        are all zero becomes NaN.
        The stretch graphs key on the mode: the first step in a new mode runs launch by launch, each mode keeps its own capture,
        switching back replays the old one.  The mode is independent of every other one (vote supervision, instance votes, proposal
        supervision, proposal sampling, point features, monitors, the step guard).  It is a setting of the run, not checkpoint
        state, and it applies to inference as much as to training: evaluate a network under the mode it was trained in."""
        from . import unit_votes as UV
        if mode not in UV.MODES:
            raise M.L.InvalidArgumentError("enable_vote_features: mode must be one of %s, got %r" % (", ".join(UV.MODES), mode))
        self.vote_features = mode

    def disable_vote_features(self):
        """Back to the launches of a pass with the reference's un-normalised vote features (the default)."""
        self.vote_features = None

    # ---- the step guard (step_guard.py): off unless asked for ------------------------------------------------------------------
    step_guard = None        # a step_guard.StepGuard while enable_step_guard is in force

    def enable_step_guard(self):
        """From now on the optimizer of every train_step runs behind a verdict on the device (step_guard.py): a step whose gradient is
        not finite leaves parameters, Adam moments and BatchNorm moving averages bit for bit as they were and is counted; a good step
        is the unguarded update bit for bit.  One launch more per step; nothing is read back until self.step_guard.read().  The
        optimizer must exist (init_optimizer / a loaded checkpoint); the counters start at zero, the snapshot of the moving averages is
        taken now.  -> the StepGuard."""
        from . import step_guard
        self.step_guard = step_guard.StepGuard(self)
        return self.step_guard

    def disable_step_guard(self):
        """Back to the launches of an unguarded step (the default)."""
        self.step_guard = None

    def init_optimizer(self, lr=LEARNING_RATE):
        s = self.store
        base = s.flat.data_ptr()
        seg = []
        for name, shape, _ in s._specs:  # [start, end) of every tensor inside the flat bucket
            a = (s.views[name].data_ptr() - base) // 4
            seg += [a, a + math.prod(shape)]
        self._seg = torch.tensor(seg, dtype=torch.int64, device=self.device)
        self._sumsq = torch.zeros(M.SUMSQ_SLICES * (len(seg) // 2), dtype=torch.float32, device=self.device)  # ordered partials per tensor
        self._m = torch.zeros_like(s.flat)
        self._v = torch.zeros_like(s.flat)
        self._step = 0
        self._lr = lr

    def set_lr(self, lr):
        """The rate of the following Adam steps (the reference's ScheduledHyperParamSetter('learning_rate', ...), run.py:113); it is
        part of the optimizer state a checkpoint keeps, so a resumed run continues the schedule."""
        lr = float(lr)
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError("set_lr: the learning rate must be finite and >= 0, got %r" % lr)
        if not hasattr(self, "_seg"):
            self.init_optimizer(lr)
        self._lr = lr

    # ---- checkpoints (checkpoint.py: the reference's variable names, restored in place) ---------------------------------------
    def state_dict(self, optimizer=True):
        """Reference variable name -> numpy array: parameters, BatchNorm moving averages and (optimizer=True) the Adam moments,
        global_step and learning_rate."""
        return checkpoint.state_dict(self, optimizer)

    def load_state_dict(self, sd, strict=True):
        """Copy a state_dict() into this model's live buffers in place; ValueError (model untouched) when it does not fit."""
        checkpoint.load_state_dict(self, sd, strict)

    def save(self, path, optimizer=True):
        """Write the state to an .npz file at `path` (numeric arrays + a JSON header)."""
        checkpoint.save(self, path, optimizer)

    load = _Load()

    def train_step(self, x, cot=None, world=1, gt=None, next_x=None, feats=None, next_feats=None):
        """forward + loss + backward + (world>1: the RCCL all-reduce of the flat gradient bucket, its tail overlapped with the
        backward pass of sa2 / sa1: dp.GradSync) + clip/Adam.
        gt: ground truth on the device (loss.gt_to_device): the reference's total cost (model.py:228) drives the backward
        pass, its components are left in self.last_losses (device, loss.NAMES).  cot: fixed cotangents instead (tests).
        feats / next_feats: sa1's input features of x / next_x, for a network built with point_features (forward())."""
        self._sa1_points(x, feats, "train_step")  # (before anything is zeroed or enqueued)
        if self.instance_votes == "instance" and gt is not None:
            self._check_point_box(x, gt)
        if not hasattr(self, "_seg"):
            self.init_optimizer()
        self.store.grad.zero_()
        # every W^T of the backward pass's input-gradient GEMMs: one launch on the geometry stream, under the sa1 FPS
        self.store.refresh_transposes(self._side_stream())
        tape = []
        # ONE zero fill for every accumulator and scatter target of the step (mlp._StatsArena): forward() and backward() join it
        M.arena_begin(self.device, whole_step=True)
        try:
            if getattr(self, "_gsync", None) is None:
                self._gsync = dp.GradSync(self.store, self.store.offset_of("sa3/"))
            if self._stretch_eligible(x, cot, gt):
                out = self._train_step_stretch(x, gt, tape, next_x, **self._feats_kw(feats, next_feats))
            else:
                out = self.forward(x, tape, next_x=next_x, **self._feats_kw(feats, next_feats))
                self._grams_ahead(tape)
                self.update_moving_averages(tape)
                if gt is not None:
                    from . import loss as VL
                    self._keep_seed_levels(tape)
                    self.last_losses, cot = VL.votenet_loss(out, gt, head=self.head)
                    self._after_loss(out, gt, self.last_losses, cot)
                self._gsync.begin()
                if PREFETCH_AFTER >= 5:  # the next batch's geometry chain under the BACKWARD pass
                    for nx, nf in self._pair_next(next_x, next_feats):
                        self.prefetch_geometry(nx, nf)
                self.backward(tape, cot)            # world > 1: starts the all-reduce of the bucket's tail after sa3's backward
        finally:
            M.arena_end()
        self.store.invalidate_transposes()      # the optimizer changes W
        gscale = self._gsync.finish()           # head all-reduce + wait for both; 1/world goes to the optimizer
        self._step += 1
        if self.step_guard is not None:
            self.step_guard.apply(self, gscale)  # the same update behind the verdict on this gradient (step_guard.py)
        else:
            M.clip_adam(self._seg, self._sumsq, self.store.flat, self.store.grad, self._m, self._v, self._lr, self._step,
                        grad_scale=gscale)
        if self.monitors is not None:
            self.monitors.after_optimizer(self, gscale, 0.5)  # (0.5: clip_adam's clip_by_average_norm, model.py:249)
        return out
