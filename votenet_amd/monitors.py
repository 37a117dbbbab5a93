"""The summaries a training run of the reference prints and records, kept on the device (opt-in: VoteNetHotPath.enable_monitors).

    obj_accuracy, sem_accuracy, total_cost    model.py:164-166, 215-216, 222, 233; their moving averages over 100 steps, run.py:127
                                              (SimpleMovingAverage): one launch behind the loss (votenet_accuracies)
                                              that also appends the step's row to a device ring -- no read-back per step
    rms / histogram of every weight matrix    model.py:236 (add_param_summary) and model.py:250 (gradproc.SummaryGradient): one
    and of every gradient                     launch per bucket (votenet_tensor_stats), every `tensors_every` steps

Both entries live in libvotenet_monitors.so (csrc/monitors/monitors.hip, include/votenet_monitors.h), loaded when first used.
Monitors.read() is the only call that synchronises with the device.  The ring and the counters are run-time state, not part of a
checkpoint (tensorpack's MovingAverageSummary callback is not either): a resumed run starts with an empty window.  Under data
parallelism every rank reports its own shard (as BatchNorm statistics are per replica); nothing is exchanged.

Departures from the reference: the histogram is exact integer counts by sign and binary exponent, not TensorBoard's
1.1-ratio display buckets; the gradient summarised is the one votenet_clip_adam reads (all-reduced, grad_scale applied), with the
factor tf.clip_by_average_norm applies reported beside it -- the clipped gradient is never stored here."""
import math

import numpy as np
import torch

from . import _lib as L
from . import loss as VL

HIST_BINS = 130        # VOTENET_TENSOR_HIST_BINS
STATS_FLOATS = 5       # VOTENET_TENSOR_STATS_FLOATS: sum, sum of squares, min, max, clip factor
STATS_INTS = 1 + HIST_BINS  # VOTENET_TENSOR_STATS_INTS: non-finite count, then the bins
EXP_MIN, EXP_MAX = -40, 23
RING_NAMES = ("obj_accuracy", "sem_accuracy", "total_cost", "n_pos", "n_neg")


def hist_bin(x):
    """The histogram bin of every element of x (float32), on the host: 0 zeros and subnormals; 1 + (e + 40) positive values of unbiased
    binary exponent e clamped to [-40, 23]; 65 + (e + 40) negative ones; 129 inf and NaN.  (What votenet_tensor_stats counts.)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    ex = (u >> 23) & 0xFF
    e = np.clip(ex - 127, EXP_MIN, EXP_MAX)
    out = 1 + (e - EXP_MIN) + np.where(u >> 31, EXP_MAX - EXP_MIN + 1, 0)
    out = np.where(ex == 0, 0, out)
    return np.where(ex == 0xFF, HIST_BINS - 1, out)


def hist_bin_label(i):
    """'0', '+2^e', '-2^e' or 'nonfinite' for bin i (the end bins take everything beyond them)."""
    if i == 0:
        return "0"
    if i == HIST_BINS - 1:
        return "nonfinite"
    n = EXP_MAX - EXP_MIN + 1
    return "%s2^%d" % ("+" if i <= n else "-", (i - 1) % n + EXP_MIN)


def tensor_stats(seg, x, scale=1.0, clip=0.0, out=None):
    """votenet_tensor_stats over the flat bucket x (float32, device) with the segment table seg (int64, device: [start, end) per
    tensor, as votenet_clip_adam's) -> stats (T, 5) f32, hist (T, 131) int32 on the device.  One launch, nothing read back."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise L.InvalidArgumentError("tensor_stats: the bucket must be a contiguous float32 device tensor")
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda and seg.dtype == torch.int64 and seg.is_contiguous() and seg.numel() % 2 == 0
            and seg.numel() > 0):
        raise L.InvalidArgumentError("tensor_stats: seg must be 2 * ntensors int64 offsets on the device")
    nt = seg.numel() // 2
    if out is None:
        out = (torch.empty((nt, STATS_FLOATS), dtype=torch.float32, device=x.device),
               torch.empty((nt, STATS_INTS), dtype=torch.int32, device=x.device))
    stats, hist = out
    if tuple(stats.shape) != (nt, STATS_FLOATS) or tuple(hist.shape) != (nt, STATS_INTS):
        raise L.InvalidArgumentError("tensor_stats: output buffers made for another table")
    with L.device_guard(x.device):
        L.check(L.side_lib("monitors").votenet_tensor_stats(nt, L.ptr(seg), L.ptr(x), float(scale), float(clip), L.ptr(stats), L.ptr(hist), L.stream_ptr()), side="monitors")
    return stats, hist


# ---- the host side of read(): plain numpy in, plain Python out ----------------------------------------------------------------

def summarize_ring(ring, steps):
    """ring (window, 5) as the device holds it after `steps` steps -> (last row, mean over the filled rows) as dicts keyed by RING_NAMES;
    the mean is the arithmetic mean of min(steps, window) rows, a NaN row makes its column's mean NaN (SimpleMovingAverage averages
    what it was fed).  No step yet: (None, None)."""
    ring = np.asarray(ring, dtype=np.float32)
    window = ring.shape[0]
    if steps <= 0:
        return None, None
    filled = ring[:min(steps, window)]
    last = ring[(steps - 1) % window]
    mean = filled.astype(np.float64).mean(axis=0)
    return ({k: float(v) for k, v in zip(RING_NAMES, last)}, {k: float(v) for k, v in zip(RING_NAMES, mean)})


def tensor_table(names, numel, stats, hist):
    """The per-tensor table of one bucket from the launch's two outputs: name -> dict(numel, nonfinite, sum, sumsq, mean, rms, min,
    max, clip_factor, hist).  mean and rms (tensorpack's rms summary: sqrt(mean(x^2))) are over the finite elements."""
    out = {}
    for i, name in enumerate(names):
        bad = int(hist[i][0])
        n = int(numel[i]) - bad
        s, ss = float(stats[i][0]), float(stats[i][1])
        out[name] = dict(numel=int(numel[i]), nonfinite=bad, sum=s, sumsq=ss, mean=s / n if n else math.nan,
                         rms=math.sqrt(ss / n) if n else math.nan, min=float(stats[i][2]), max=float(stats[i][3]),
                         clip_factor=float(stats[i][4]), hist=np.asarray(hist[i][1:], dtype=np.int64).copy())
    return out


def tensor_names(net):
    """The reference's variable name (checkpoint.py; tests/golden/votenet_variable_names.txt) of every segment of the optimizer's
    table, in its order."""
    from . import checkpoint
    key_of = {src: key for key, _, kind, src in checkpoint._entries(net, optimizer=False) if kind == "param"}
    return [key_of[name] for name, _, _ in net.store._specs]


class Monitors:
    """The device state behind VoteNetHotPath.enable_monitors: the ring, the step's accuracies and counts, the tensor tables."""

    def __init__(self, net, window=100, tensors_every=0):
        window, tensors_every = int(window), int(tensors_every)
        if window < 1 or tensors_every < 0:
            raise ValueError("monitors: window >= 1 and tensors_every >= 0 expected, got %d, %d" % (window, tensors_every))
        dev = net.device
        self.window, self.tensors_every = window, tensors_every
        self.head = getattr(net, "head", None)  # the accuracy launch reads its nh / ns / nc (None: the default head's)
        self.steps = 0          # accuracy launches so far: the next one writes ring row steps % window
        self.ring = torch.zeros((window, VL.RING_COLS), dtype=torch.float32, device=dev)
        self.accuracies = torch.zeros(2, dtype=torch.float32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int32, device=dev)
        self._work = torch.zeros(8, dtype=torch.int32, device=dev)
        self._tables = None     # (param stats, param hist, grad stats, grad hist) once collected
        self.tensors_step = None

    def after_loss(self, out, gt, losses):
        """The accuracy launch of one step, behind its loss launch on the same stream."""
        VL.votenet_accuracies(out, gt, losses=losses, ring=self.ring, ring_row=self.steps % self.window,
                              buffers=(self.accuracies, self.counts, self._work), head=self.head)
        self.steps += 1
        return self.accuracies

    def after_optimizer(self, net, grad_scale, clip):
        """Every tensors_every-th step: the two tensor-summary launches, behind the optimizer."""
        if not self.tensors_every or net._step % self.tensors_every:
            return
        seg = net._seg
        if self._tables is None:
            nt = seg.numel() // 2
            mk = lambda: (torch.empty((nt, STATS_FLOATS), dtype=torch.float32, device=net.device),
                          torch.empty((nt, STATS_INTS), dtype=torch.int32, device=net.device))
            self._tables = mk() + mk()
        tensor_stats(seg, net.store.flat, 1.0, 0.0, out=self._tables[:2])
        tensor_stats(seg, net.store.grad, grad_scale, clip, out=self._tables[2:])
        self.tensors_step = net._step
        self._net = net

    def read(self):
        """-> dict(steps, window, filled, last, mean, tensors, tensors_step).  last / mean: dicts of obj_accuracy, sem_accuracy,
        total_cost, n_pos, n_neg (last also n_obj_correct, n_sem_correct as integers); tensors: reference variable name ->
        dict(param=..., grad=...) of tensor_table rows, or None.  The one call that waits for the device."""
        ring = self.ring.cpu().numpy()
        last, mean = summarize_ring(ring, self.steps)
        if last is not None:
            c = self.counts.cpu().tolist()
            last.update({k: int(v) for k, v in zip(VL.ACCURACY_COUNTS, c)})
        tensors = None
        if self.tensors_step is not None:
            net = self._net
            names = tensor_names(net)
            seg = net._seg.cpu().numpy()
            numel = seg[1::2] - seg[0::2]
            ps, ph, gs, gh = [t.cpu().numpy() for t in self._tables]
            p, g = tensor_table(names, numel, ps, ph), tensor_table(names, numel, gs, gh)
            tensors = {n: dict(param=p[n], grad=g[n]) for n in names}
        return dict(steps=self.steps, window=self.window, filled=min(self.steps, self.window), last=last, mean=mean, tensors=tensors,
                    tensors_step=self.tensors_step)
