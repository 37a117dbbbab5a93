"""Objectness and centre supervision as in the VoteNet paper, on the device (libvotenet_propsup.so,
include/votenet_proposal_supervision.h).

The reference (model.py:157-182, csrc/loss.hip) forms the objectness loss as mean over positives(CE) + mean over negatives(CE), NaN where
a set is empty, and the centre loss as a Huber loss of the predicted offset against the box assigned by the cluster POSITION, plus the
same Huber for each ground-truth row's nearest cluster position, averaged over all B * BB padded rows.  The paper supervises differently:
one class-weighted cross-entropy (0.2 no object, 0.8 object) over all proposals outside the grey zone, divided by their number, and a
Chamfer distance between the PREDICTED centres and the ground-truth centres -- squared L2, each positive proposal to its nearest real
centre, each real box to its nearest predicted centre among all proposals.  Ground truth padded by repeating a scene's last box counts
that box once (the rule of evaluator.gt_for_eval).  The labels stay the reference's.

paper_proposal_loss is one launch behind loss.votenet_loss: it overwrites columns 0..4 of every row of d_proposals_output and the whole of
d_proposals_xyz (nothing but the objectness and centre terms reaches them), losses[2] (obj_cls_loss) and losses[3] (center_loss), and
re-forms losses[9] and losses[0]; everything else of the step is what it was.  VoteNetHotPath.enable_proposal_supervision("paper") runs
it in every train step.  The rule is stated once, in the header; tests/proposal_supervision_ref.py restates it in numpy.

Not taken over from the paper (out of scope here): its size-residual term as the mean, not the sum, over the three axes (a factor of
1/3); its overall x 10; the BatchNorm momentum schedule; its matching against zero-padded box slots.  (Proposals sampled by FPS on the
votes instead of on the seeds are a mode of their own: vote_sampling.py, VoteNetHotPath.enable_proposal_sampling.)"""
import torch

from . import _lib as L
from .head import resolve as _head_bins
from .loss import NEGATIVE_THRES, POSITIVE_THRES, check_losses
from .synth import NC, NH, NS

MODES = ("reference", "paper")  # "reference": the rule of votenet_loss itself, no launch of this library
OBJ_WEIGHTS = (0.2, 0.8)        # the class weights of the objectness cross-entropy: no object, object


def _scene(out, gt, who, width=None):
    """-> proposals_xyz, proposals_output (rows with unit column stride, read in place), bboxes_xyz, (b, p, bb): validated, on one device."""
    pxyz = L.dev_f32(out["proposals_xyz"], "%s proposals_xyz" % who, 3, 3)
    pout = L.dev_f32_rows(out["proposals_output"], "%s proposals_output" % who)
    b, p = pxyz.shape[:2]
    if tuple(pout.shape[:2]) != (b, p) or (width is not None and pout.shape[2] != width) or pout.shape[2] < 5:
        raise L.InvalidArgumentError("%s: proposals_output has shape %s, expected (%d, %d, %s)"
                                     % (who, tuple(pout.shape), b, p, width if width is not None else ">= 5"))
    gxyz = L.dev_f32(gt["bboxes_xyz"], "%s bboxes_xyz" % who, 3, 3)
    if gxyz.shape[0] != b:
        raise L.InvalidArgumentError("%s: ground truth of %s boxes for %d scenes" % (who, tuple(gxyz.shape), b))
    if pout.device != pxyz.device or gxyz.device != pxyz.device:
        raise L.InvalidArgumentError("%s: proposals and ground truth live on different devices" % who)
    return pxyz, pout, gxyz, (b, p, gxyz.shape[1])


def proposal_targets(out, gt, pos_thr=POSITIVE_THRES, neg_thr=NEGATIVE_THRES, head=None):
    """out: proposals_xyz (B,P,3), proposals_output (B,P,W) (columns 2..4 are read); gt: device tensors (loss.gt_to_device) -> int32
    tensors label (B,P): 1 positive, 0 negative, -1 grey; near_box (B,P): the nearest real box of a positive's PREDICTED centre, else
    -1; dual_prop (B,BB): the proposal whose predicted centre is nearest to real box j, -1 for a padding row; real_boxes (B,): the
    scene's boxes without the repetitions of the last.  One launch, nothing synchronises; for inspection.  head: a HeadConfig whose
    width proposals_output must have (None: any width >= 5)."""
    nh, ns, nc = _head_bins(head, 0, 0, 0)
    pxyz, pout, gxyz, (b, p, bb) = _scene(out, gt, "proposal_targets", 5 + 2 * nh + 4 * ns + nc if head is not None else None)
    dev = pxyz.device
    label = torch.empty((b, p), dtype=torch.int32, device=dev)
    near = torch.empty((b, p), dtype=torch.int32, device=dev)
    dual = torch.empty((b, bb), dtype=torch.int32, device=dev)
    real = torch.empty((b,), dtype=torch.int32, device=dev)
    with L.device_guard(dev):
        L.check(L.side_lib("propsup").votenet_proposal_targets(b, p, bb, L.ptr(pxyz), L.ptr(pout), pout.stride(1), L.ptr(gxyz), pos_thr,
                                                               neg_thr, L.ptr(label), L.ptr(near), L.ptr(dual), L.ptr(real),
                                                               L.stream_ptr()), side="propsup")
    return label, near, dual, real


def workspace(b, device):
    """The zeroed workspace of paper_proposal_loss for b scenes; every launch leaves it zero, so one allocation serves a run."""
    return torch.zeros(int(L.side_lib("propsup").votenet_propsup_workspace_bytes(b)) // 4, dtype=torch.int32, device=device)


def paper_proposal_loss(out, gt, losses, d_xyz=None, d_out=None, counts=None, work=None, nh=NH, ns=NS, nc=NC,
                        pos_thr=POSITIVE_THRES, neg_thr=NEGATIVE_THRES, head=None):
    """out: the dict VoteNetHotPath.forward returns (proposals_xyz, proposals_output are read); gt: device tensors; losses: the 12 floats
    votenet_loss returned, changed IN PLACE: losses[2] becomes the paper's obj_cls_loss, losses[3] its center_loss, losses[9] and
    losses[0] are re-formed with them.  d_xyz (B,P,3), d_out (B,P,W) contiguous: votenet_loss's proposals_xyz / proposals_output
    cotangents; d_xyz is written in full, of d_out columns 0..4 of every row (the rest keeps its bits); None: fresh tensors (d_out zero
    beyond column 4).  counts: a three-element int32 device tensor for Np, Nn and the number of real boxes, or None: a fresh one.  work:
    workspace(B, device) of a caller that keeps it.  head: the net's HeadConfig (its nh / ns / nc in place of the keywords').
    -> d_xyz, d_out, counts.  One launch, nothing is read back."""
    nh, ns, nc = _head_bins(head, nh, ns, nc)
    width = 5 + 2 * nh + 4 * ns + nc
    pxyz, pout, gxyz, (b, p, bb) = _scene(out, gt, "paper_proposal_loss", width)
    dev = pxyz.device
    check_losses(losses, dev, "paper_proposal_loss")
    if d_xyz is None:
        d_xyz = torch.empty((b, p, 3), dtype=torch.float32, device=dev)
    if d_out is None:
        d_out = torch.zeros((b, p, width), dtype=torch.float32, device=dev)
    for t, shape, name in ((d_xyz, (b, p, 3), "d_xyz"), (d_out, (b, p, width), "d_out")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
                and t.device == dev):
            raise L.InvalidArgumentError("paper_proposal_loss: %s must be a contiguous float32 device tensor of shape %s" % (name, shape))
    if counts is None:
        counts = torch.empty(3, dtype=torch.int32, device=dev)
    counts = L.dev_i32(counts, "paper_proposal_loss counts", 1)
    lib = L.side_lib("propsup")
    if work is None:
        work = workspace(b, dev)
    if not (work.is_cuda and work.dtype == torch.int32 and work.is_contiguous() and work.device == dev
            and work.numel() * 4 >= int(lib.votenet_propsup_workspace_bytes(b)) and counts.numel() == 3 and counts.device == dev):
        raise L.InvalidArgumentError("paper_proposal_loss: buffers of the wrong size (workspace(b, device); three int32 for counts)")
    with L.device_guard(dev):
        L.check(lib.votenet_paper_proposal_loss(b, p, bb, nh, ns, nc, L.ptr(pxyz), L.ptr(pout), pout.stride(1), L.ptr(gxyz), pos_thr, neg_thr,
                                                L.ptr(losses), L.ptr(d_xyz), L.ptr(d_out), L.ptr(counts), L.ptr(work), L.stream_ptr()),
                side="propsup")
    return d_xyz, d_out, counts
