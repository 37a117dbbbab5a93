"""Vote supervision as in the VoteNet paper, on the device (libvotenet_votesup.so, include/votenet_vote_supervision.h).

The reference (model.py:62-84, csrc/loss.hip) sends every seed that lies in some ground-truth box to the centre of the NEAREST box and
divides the sum by all B * n seeds.  The paper supervises differently: a seed votes for the centres of the boxes that CONTAIN it, a
seed in several boxes keeps up to three targets and is charged the closest, and the sum is divided by the number of supervised seeds.
The seeds are points of the cloud, bit for bit, so which boxes hold a seed is decided at the seed, inside the loss, from the
seeds_xyz and the ground truth votenet_loss already receives: no label tensor, no seed index.

paper_vote_loss is one launch behind loss.votenet_loss: it overwrites the whole of d_votes_xyz (nothing but the vote term reaches it),
losses[1] (vote_reg_loss) and re-forms losses[0]; everything else of the step is what it was.  VoteNetHotPath.enable_vote_supervision
("paper") runs it in every train step.  The rule is stated once, in the header; tests/vote_supervision_ref.py restates it in numpy."""
import torch

from . import _lib as L
from .loss import check_losses

MODES = ("reference", "paper")  # "reference": the rule of votenet_loss itself, no launch of this library
MAX_BOXES = 256                 # LOSS_MAXBOX, as votenet_loss


def _scene(seeds_xyz, gt, who):
    """-> seeds, (xyz, lwh, roty), (b, n, bb): validated, contiguous, on one device."""
    seeds = L.dev_f32(seeds_xyz.detach(), "%s seeds_xyz" % who, 3, 3)
    b, n = seeds.shape[:2]
    xyz = L.dev_f32(gt["bboxes_xyz"], "%s bboxes_xyz" % who, 3, 3)
    lwh = L.dev_f32(gt["bboxes_lwh"], "%s bboxes_lwh" % who, 3, 3)
    roty = L.dev_f32(gt["bboxes_roty"], "%s bboxes_roty" % who, 2)
    bb = xyz.shape[1]
    if xyz.shape[0] != b or tuple(lwh.shape) != tuple(xyz.shape) or tuple(roty.shape) != (b, bb):
        raise L.InvalidArgumentError("%s: ground truth of %s / %s / %s boxes for %d scenes"
                                     % (who, tuple(xyz.shape), tuple(lwh.shape), tuple(roty.shape), b))
    if any(t.device != seeds.device for t in (xyz, lwh, roty)):
        raise L.InvalidArgumentError("%s: seeds and ground truth live on different devices" % who)
    return seeds, (xyz, lwh, roty), (b, n, bb)


def vote_targets(seeds_xyz, gt):
    """(B,n,3) f32 seeds, gt: device tensors (loss.gt_to_device) -> slots (B,n,3) int32: the box indices of the seed's three targets
    (the first, the second and the LAST of the boxes that contain it, in index order; the first again where there are fewer; all -1
    where there is none), inside_count (B,n) int32: how many boxes contain it.  One launch, nothing synchronises; for inspection."""
    seeds, (xyz, lwh, roty), (b, n, bb) = _scene(seeds_xyz, gt, "vote_targets")
    slots = torch.empty((b, n, 3), dtype=torch.int32, device=seeds.device)
    count = torch.empty((b, n), dtype=torch.int32, device=seeds.device)
    with L.device_guard(seeds.device):
        L.check(L.side_lib("votesup").votenet_vote_targets(b, n, bb, L.ptr(seeds), L.ptr(xyz), L.ptr(lwh), L.ptr(roty), L.ptr(slots),
                                                           L.ptr(count), L.stream_ptr()), side="votesup")
    return slots, count


def workspace(b, device):
    """The zeroed workspace of paper_vote_loss for b scenes; every launch leaves it zero, so one allocation serves a run."""
    return torch.zeros(int(L.side_lib("votesup").votenet_votesup_workspace_bytes(b)) // 4, dtype=torch.int32, device=device)


def paper_vote_loss(out, gt, losses, d_votes=None, supervised=None, work=None):
    """out: the dict VoteNetHotPath.forward returns (seeds_xyz, votes_xyz are read); gt: device tensors; losses: the 12 floats
    votenet_loss returned, changed IN PLACE: losses[1] becomes the paper's vote_reg_loss, losses[0] the total re-formed with it.
    d_votes: the (B,n,3) buffer that receives the cotangent, written in full (votenet_loss's votes_xyz cotangent, to replace it);
    None: a fresh tensor.  supervised: a one-element int32 device tensor for the number of supervised seeds, or None: a fresh one.
    work: workspace(B, device) of a caller that keeps it.  -> d_votes, supervised.  One launch, nothing is read back."""
    seeds, (xyz, lwh, roty), (b, n, bb) = _scene(out["seeds_xyz"], gt, "paper_vote_loss")
    votes = L.dev_f32(out["votes_xyz"].detach(), "paper_vote_loss votes_xyz", 3, 3)
    dev = seeds.device
    if tuple(votes.shape) != (b, n, 3) or votes.device != dev:
        raise L.InvalidArgumentError("paper_vote_loss: votes_xyz of shape %s for seeds of shape %s" % (tuple(votes.shape), tuple(seeds.shape)))
    check_losses(losses, dev, "paper_vote_loss")
    if d_votes is None:
        d_votes = torch.empty_like(votes)
    if not (isinstance(d_votes, torch.Tensor) and d_votes.is_cuda and d_votes.dtype == torch.float32 and d_votes.is_contiguous()
            and tuple(d_votes.shape) == (b, n, 3) and d_votes.device == dev):
        raise L.InvalidArgumentError("paper_vote_loss: d_votes must be a contiguous float32 device tensor of votes_xyz's shape")
    if supervised is None:
        supervised = torch.empty(1, dtype=torch.int32, device=dev)
    supervised = L.dev_i32(supervised, "paper_vote_loss supervised", 1)
    lib = L.side_lib("votesup")
    if work is None:
        work = workspace(b, dev)
    if not (work.is_cuda and work.dtype == torch.int32 and work.is_contiguous() and work.device == dev
            and work.numel() * 4 >= int(lib.votenet_votesup_workspace_bytes(b)) and supervised.numel() == 1):
        raise L.InvalidArgumentError("paper_vote_loss: buffers of the wrong size (workspace(b, device); one int32 for supervised)")
    with L.device_guard(dev):
        L.check(lib.votenet_paper_vote_loss(b, n, bb, L.ptr(seeds), L.ptr(votes), L.ptr(xyz), L.ptr(lwh), L.ptr(roty), L.ptr(losses),
                                            L.ptr(d_votes), L.ptr(supervised), L.ptr(work), L.stream_ptr()), side="votesup")
    return d_votes, supervised
