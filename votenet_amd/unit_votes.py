"""Unit-length vote features, as in the authors' VoteNet, on the device (libvotenet_unitvote.so, include/votenet_unit_votes.h).

The authors' network (models/votenet.py, behind voting_module.py) forms the vote features as seed_features + residual and then divides
each vote's 256-vector by its L2 norm -- features.div(torch.norm(features, p=2, dim=1)) --; the proposal module reads the result.  The
reference hands the un-normalised sum on (model.py:60, 85), and so does VoteNetHotPath.vote() by default.

unit_votes is one launch: the sum votes = x + offset, its split into xyz and features and the normalisation, in the place of the glue
launch (mlp.row_segments) that forms the same two buffers without it.  unit_votes_backward is one launch in the place of the glue launch
that builds the voting chain's output gradient [d_vx + cot | d_vp | 0]: it writes [d_vx + cot | (d_vp - y (y . d_vp)) / norm | 0], the
gradient of the un-normalised sum, which everything behind it already consumes.  VoteNetHotPath.enable_vote_features("unit") puts both
into every pass; the launch count of a pass does not change.  The rule is stated once, in the header; tests/unit_votes_ref.py restates
it in numpy.  There is no epsilon, as in the authors' code: a vote whose features are all zero gives NaN."""
import torch

from . import _lib as L

MODES = ("unit",)  # None (no mode): the reference's un-normalised vote features, the default, no launch of this library
MIN_C, MAX_C = 64, 512  # the kernel's limits (the header's): channels in multiples of 64


def supported(c):
    """True when the kernels take rows of c feature channels."""
    return bool(MIN_C <= c <= MAX_C and c % 64 == 0)


def _rows(t, name, width=None):
    """(tensor, row pitch in elements) of a 2-D float32 device view with unit column stride, as mlp.row_segments takes its operands
    (a column slice of a wider tensor is fine: its pitch is used)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise L.InvalidArgumentError("%s: a 2-D row-major view with unit column stride expected" % name)
    if not t.is_cuda:
        raise L.VotenetError("%s must live on the GPU (no CPU fallback in votenet_amd)" % name)
    if t.dtype != torch.float32:
        raise L.InvalidArgumentError("%s must be float32" % name)
    if width is not None and t.shape[1] != width:
        raise L.InvalidArgumentError("%s expects %d columns, got shape %s" % (name, width, tuple(t.shape)))
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


def _flat(t, name, rows, width):
    """A contiguous float32 device tensor of rows * width elements (any shape that holds them)."""
    t = L.dev_f32(t, name)
    if t.numel() != rows * width:
        raise L.InvalidArgumentError("%s expects %d x %d elements, got shape %s" % (name, rows, width, tuple(t.shape)))
    return t


def unit_votes(x, off):
    """x, off (rows, 3 + c) f32 views (the voting input and the voting MLP's output; row pitches taken from the views) ->
    votes_xyz (rows, 3) = x[:, :3] + off[:, :3], votes_points (rows, c) = u / |u| with u = x[:, 3:] + off[:, 3:], norm (rows) = |u|.
    One launch, nothing is read back."""
    x, xp = _rows(x, "unit_votes: x")
    rows, w = x.shape
    off, op = _rows(off, "unit_votes: off", w)
    if off.shape[0] != rows:
        raise L.InvalidArgumentError("unit_votes: x and off must have equally many rows, got %d and %d" % (rows, off.shape[0]))
    c = w - 3
    dev = x.device
    v_xyz = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    v_p = torch.empty((rows, max(c, 0)), dtype=torch.float32, device=dev)
    norm = torch.empty((rows,), dtype=torch.float32, device=dev)
    with L.device_guard(dev):
        L.check(L.side_lib("unitvote").votenet_unit_votes(rows, c, L.ptr(x), xp, L.ptr(off), op, L.ptr(v_xyz), L.ptr(v_p), L.ptr(norm),
                                                          L.stream_ptr()), side="unitvote")
    return v_xyz, v_p, norm


def unit_votes_backward(d_xyz, cot_xyz, d_points, votes_points, norm, d_votes):
    """d_votes (rows, d_width) f32 view (row pitch taken from the view) <- [d_xyz (+ cot_xyz) | (g - y (y . g)) / norm | 0] with
    g = d_points, y = votes_points and norm as unit_votes left them; cot_xyz may be None.  The other operands are contiguous, of
    rows x 3, rows x c and rows elements.  One launch; -> d_votes."""
    d_votes, dp = _rows(d_votes, "unit_votes_backward: d_votes")
    rows, dw = d_votes.shape
    norm = _flat(norm, "unit_votes_backward: norm", rows, 1)
    c = votes_points.shape[-1] if isinstance(votes_points, torch.Tensor) and votes_points.dim() else 0
    y = _flat(votes_points, "unit_votes_backward: votes_points", rows, c)
    g = _flat(d_points, "unit_votes_backward: d_points", rows, c)
    dx = _flat(d_xyz, "unit_votes_backward: d_xyz", rows, 3)
    cv = _flat(cot_xyz, "unit_votes_backward: cot_xyz", rows, 3) if cot_xyz is not None else None
    with L.device_guard(d_votes.device):
        L.check(L.side_lib("unitvote").votenet_unit_votes_backward(rows, c, L.ptr(dx), L.ptr(cv), L.ptr(g), L.ptr(y), L.ptr(norm),
                                                                   L.ptr(d_votes), dp, dw, L.stream_ptr()), side="unitvote")
    return d_votes
