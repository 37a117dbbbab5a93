"""Vote supervision from instance labels, on the device (libvotenet_instvote.so, include/votenet_instance_votes.h).

Both rules the project had decide a seed's target by geometry: votenet_loss sends a seed that lies in some box to the nearest box,
vote_supervision.paper_vote_loss to the centres of the boxes that contain it.  On ground truth made from instance-labelled points
(input_pipeline.build_batch_from_labels) the boxes are the axis-aligned hulls of the instances: they overlap -- a chair under a table
-- and they hold points that belong to nothing -- the floor under a bed.  The VoteNet paper supervises a point on an object towards
the centre of ITS OWN instance's box and leaves every unlabelled point alone.  The seeds are cloud points bit for bit (sa2's centres
are picked from sa1's centres, which are picked from the cloud), so a seed's instance is two index tensors and one label row away:
levels = (sa1's fps_idx, sa2's fps_idx) and gt["point_box"] (build_batch_from_labels(..., point_box=True)).

instance_vote_loss is one launch behind loss.votenet_loss: it overwrites the whole of d_votes_xyz, losses[1] (vote_reg_loss) and
re-forms losses[0]; everything else of the step is what it was.  VoteNetHotPath.enable_instance_votes() runs it in every train step.
The rule is stated once, in the header; tests/instance_votes_ref.py restates it in numpy."""
import torch

from . import _lib as L
from .loss import check_losses

MODES = ("reference", "instance")  # "reference": the rule of votenet_loss itself, no launch of this library
MAX_BOXES = 256                    # LOSS_MAXBOX, as votenet_loss


def _idx(t, name, who, rank=2):
    """A contiguous int32 device tensor of the given rank, as it is (no copy: the launch reads the caller's memory)."""
    if not isinstance(t, torch.Tensor):
        raise L.InvalidArgumentError("%s: %s must be a torch.Tensor" % (who, name))
    if not t.is_cuda:
        raise L.VotenetError("%s: %s must live on the GPU (no CPU fallback in votenet_amd)" % (who, name))
    if t.dtype != torch.int32:
        raise L.InvalidArgumentError("%s: %s must be int32, got %s" % (who, name, t.dtype))
    if t.dim() != rank:
        raise L.InvalidArgumentError("%s: %s expects rank %d, got shape %s" % (who, name, rank, tuple(t.shape)))
    if not t.is_contiguous():
        raise L.InvalidArgumentError("%s: %s must be contiguous" % (who, name))
    return t


def _levels(levels, who):
    """levels = (idx1 (b, n1), idx2 (b, n)) -> idx1, idx2, (b, n1, n): validated, on one device."""
    try:
        idx1, idx2 = levels
    except (TypeError, ValueError):
        raise L.InvalidArgumentError("%s: levels must be the pair (idx1, idx2): sa1's and sa2's fps_idx" % who) from None
    idx1, idx2 = _idx(idx1, "idx1", who), _idx(idx2, "idx2", who)
    if idx1.shape[0] != idx2.shape[0] or idx1.device != idx2.device:
        raise L.InvalidArgumentError("%s: idx1 %s and idx2 %s must hold the same scenes on one device"
                                     % (who, tuple(idx1.shape), tuple(idx2.shape)))
    return idx1, idx2, (int(idx1.shape[0]), int(idx1.shape[1]), int(idx2.shape[1]))


def seed_points(idx1, idx2, n0):
    """idx1 (b, n1) int32: sa1's picks into a cloud of n0 points; idx2 (b, n) int32: sa2's picks into sa1's centres -> (b, n) int32:
    the cloud point every seed is, -1 where an index of the chain is out of range.  One launch, nothing synchronises; for inspection."""
    idx1, idx2, (b, n1, n) = _levels((idx1, idx2), "seed_points")
    out = torch.empty((b, n), dtype=torch.int32, device=idx1.device)
    with L.device_guard(idx1.device):
        L.check(L.side_lib("instvote").votenet_seed_points(b, int(n0), n1, n, L.ptr(idx1), L.ptr(idx2), L.ptr(out), L.stream_ptr()),
                side="instvote")
    return out


def workspace(b, device):
    """The zeroed workspace of instance_vote_loss for b scenes; every launch leaves it zero, so one allocation serves a run."""
    return torch.zeros(int(L.side_lib("instvote").votenet_instvote_workspace_bytes(b)) // 4, dtype=torch.int32, device=device)


def instance_vote_loss(out, gt, losses, levels, d_votes=None, counts=None, work=None):
    """out: the dict VoteNetHotPath.forward returns (votes_xyz is read); gt: device tensors, of which bboxes_xyz (b, bb, 3) and
    point_box (b, n0) int32 -- the row of every cloud point's box within its scene, negative for none -- are read; levels = (idx1,
    idx2): sa1's and sa2's fps_idx of this pass; losses: the 12 floats votenet_loss returned, changed IN PLACE: losses[1] becomes the
    vote_reg_loss towards the seeds' own instances, losses[0] the total re-formed with it.  d_votes: the (B,n,3) buffer that receives
    the cotangent, written in full (votenet_loss's votes_xyz cotangent, to replace it); None: a fresh tensor.  counts: a two-element
    int32 device tensor for P, the supervised seeds, and Q, the seeds whose chain or box row was out of range; None: a fresh one.
    work: workspace(B, device) of a caller that keeps it.  -> d_votes, counts.  One launch, nothing is read back."""
    who = "instance_vote_loss"
    idx1, idx2, (b, n1, n) = _levels(levels, who)
    dev = idx1.device
    votes = L.dev_f32(out["votes_xyz"].detach(), "%s votes_xyz" % who, 3, 3)
    xyz = L.dev_f32(gt["bboxes_xyz"], "%s bboxes_xyz" % who, 3, 3)
    if "point_box" not in gt:
        raise L.InvalidArgumentError("%s: gt has no point_box (input_pipeline.build_batch_from_labels(..., point_box=True) makes it)" % who)
    point_box = _idx(gt["point_box"], "point_box", who)
    if tuple(votes.shape) != (b, n, 3) or xyz.shape[0] != b or point_box.shape[0] != b:
        raise L.InvalidArgumentError("%s: votes_xyz %s, bboxes_xyz %s and point_box %s for %d scenes of %d seeds"
                                     % (who, tuple(votes.shape), tuple(xyz.shape), tuple(point_box.shape), b, n))
    if any(t.device != dev for t in (votes, xyz, point_box)):
        raise L.InvalidArgumentError("%s: levels, votes and ground truth live on different devices" % who)
    n0, bb = int(point_box.shape[1]), int(xyz.shape[1])
    check_losses(losses, dev, who)
    if d_votes is None:
        d_votes = torch.empty_like(votes)
    if not (isinstance(d_votes, torch.Tensor) and d_votes.is_cuda and d_votes.dtype == torch.float32 and d_votes.is_contiguous()
            and tuple(d_votes.shape) == (b, n, 3) and d_votes.device == dev):
        raise L.InvalidArgumentError("%s: d_votes must be a contiguous float32 device tensor of votes_xyz's shape" % who)
    if counts is None:
        counts = torch.empty(2, dtype=torch.int32, device=dev)
    counts = _idx(counts, "counts", who, 1)
    lib = L.side_lib("instvote")
    if work is None:
        work = workspace(b, dev)
    if not (isinstance(work, torch.Tensor) and work.is_cuda and work.dtype == torch.int32 and work.is_contiguous() and work.device == dev
            and work.numel() * 4 >= int(lib.votenet_instvote_workspace_bytes(b)) and counts.numel() == 2 and counts.device == dev):
        raise L.InvalidArgumentError("%s: buffers of the wrong size (workspace(b, device); two int32 for counts)" % who)
    with L.device_guard(dev):
        L.check(lib.votenet_instance_vote_loss(b, n0, n1, n, bb, L.ptr(idx1), L.ptr(idx2), L.ptr(point_box), L.ptr(votes), L.ptr(xyz),
                                               L.ptr(losses), L.ptr(d_votes), L.ptr(counts), L.ptr(work), L.stream_ptr()), side="instvote")
    return d_votes, counts
