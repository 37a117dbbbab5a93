"""The reference's loss graph on the device: one kernel (votenet_loss, csrc/loss.hip) for the total cost of model.py:228
and its cotangents with respect to the three tensors through which it reaches the hot path."""
import torch

from . import _lib as L
from .head import resolve as _head_bins
from .synth import NC, NH, NS

POSITIVE_THRES, NEGATIVE_THRES = 0.3, 0.6  # config.py
NAMES = ("total_cost", "vote_reg_loss", "obj_cls_loss", "center_loss", "heading_cls_loss", "heading_residual_loss",
         "size_cls_loss", "size_residual_loss", "sem_cls_loss", "box_loss", "n_pos", "n_neg")
GT_KEYS = ("bboxes_xyz", "bboxes_lwh", "bboxes_roty", "semantic_labels", "heading_labels", "heading_residuals", "size_labels",
           "size_residuals")


def gt_to_device(gt, device):
    """numpy ground-truth dict (synth.room_gt) -> contiguous device tensors."""
    return {k: torch.from_numpy(gt[k]).contiguous().to(device) for k in GT_KEYS}


def loss_buffers(out, losses=None):
    """The output buffers of votenet_loss for the tensors of `out`, allocated once by a caller that wants them at fixed addresses
    (model.StretchGraph: the segments captured behind the loss read the cotangents there): -> (losses (12,), flat).  flat holds the three
    cotangents and the kernel's workspace and must be ZERO when votenet_loss(..., buffers=) runs (here: a carve-out of the pass's arena)."""
    from . import mlp as M
    votes, pxyz, pout = out["votes_xyz"], out["proposals_xyz"], out["proposals_output"]
    nws = int(L.lib().votenet_loss_workspace_floats(votes.shape[0]))
    if losses is None:
        losses = torch.empty(12, dtype=torch.float32, device=votes.device)
    return losses, M._zeros_f32((votes.numel() + pxyz.numel() + pout.numel() + nws,), votes.device)


def cotangent_views(votes, pxyz, pout, flat):
    """The layout of flat (loss_buffers), stated once: votes | proposals_xyz | proposals_output | workspace.  votes, pxyz, pout: tensors
    of the cotangents' shapes.  -> the three cotangents as views of flat, keyed like out, and the workspace tail."""
    nv, npx, npo = votes.numel(), pxyz.numel(), pout.numel()
    cot = dict(votes_xyz=flat[:nv].view_as(votes), proposals_xyz=flat[nv:nv + npx].view_as(pxyz),
               proposals_output=flat[nv + npx:nv + npx + npo].view_as(pout))
    return cot, flat[nv + npx + npo:]


def check_losses(losses, dev, who):
    """losses must be the 12 contiguous float32 values of votenet_loss on device dev (the launches behind it change them in place)."""
    if not (isinstance(losses, torch.Tensor) and losses.is_cuda and losses.dtype == torch.float32 and losses.numel() == 12
            and losses.is_contiguous() and losses.device == dev):
        raise L.InvalidArgumentError("%s: losses must be the 12 floats of votenet_loss on the device" % who)


def votenet_loss(out, gt, nh=NH, ns=NS, nc=NC, buffers=None, head=None):
    """out: the dict VoteNetHotPath.forward returns; gt: device tensors (gt_to_device).  head: the net's HeadConfig (its nh / ns / nc in
    place of the keywords'; None: the keywords, whose defaults are the default head's).
    -> losses (12,) f32 on the device (NAMES), cotangents dict(votes_xyz, proposals_xyz, proposals_output).
    buffers: (losses, flat) from loss_buffers(out), flat zeroed by the caller -- the results land there instead of in fresh tensors."""
    nh, ns, nc = _head_bins(head, nh, ns, nc)
    seeds = L.dev_f32(out["seeds_xyz"], "loss seeds_xyz", 3, 3)
    votes = L.dev_f32(out["votes_xyz"], "loss votes_xyz", 3, 3)
    pxyz = L.dev_f32(out["proposals_xyz"], "loss proposals_xyz", 3, 3)
    pout = L.dev_f32_rows(out["proposals_output"], "loss proposals_output")
    b, n = seeds.shape[:2]
    p = pxyz.shape[1]
    bb = gt["bboxes_xyz"].shape[1]
    if pout.shape[2] != 5 + 2 * nh + 4 * ns + nc:
        raise L.InvalidArgumentError("loss: proposals_output has %d channels, expected %d" % (pout.shape[2], 5 + 2 * nh + 4 * ns + nc))
    dev = seeds.device
    # the three cotangents and the kernel's workspace are ONE buffer cleared by ONE fill
    total = votes.numel() + pxyz.numel() + pout.numel() + int(L.lib().votenet_loss_workspace_floats(b))
    from . import mlp as M
    if buffers is not None:
        losses, flat = buffers
        if flat.numel() != total or losses.numel() != 12:
            raise L.InvalidArgumentError("loss: the buffers were made for other shapes (loss_buffers(out))")
    else:
        losses = torch.empty(12, dtype=torch.float32, device=dev)
        flat = M._zeros_f32((total,), dev)  # inside a train step: a carve-out of the pass's one zero fill
    cot, ws = cotangent_views(votes, pxyz, pout, flat)
    with L.device_guard(dev):
        L.check(L.lib().votenet_loss_pitched(b, n, p, bb, nh, ns, nc, L.ptr(seeds), L.ptr(votes), L.ptr(pxyz), L.ptr(pout), pout.stride(1),
                                     L.ptr(gt["bboxes_xyz"]), L.ptr(gt["bboxes_lwh"]), L.ptr(gt["bboxes_roty"]),
                                     L.ptr(gt["semantic_labels"]), L.ptr(gt["heading_labels"]), L.ptr(gt["heading_residuals"]),
                                     L.ptr(gt["size_labels"]), L.ptr(gt["size_residuals"]), POSITIVE_THRES, NEGATIVE_THRES,
                                     L.ptr(losses), L.ptr(cot["votes_xyz"]), L.ptr(cot["proposals_xyz"]), L.ptr(cot["proposals_output"]),
                                     L.ptr(ws), L.stream_ptr()))
    return losses, cot


ACCURACY_COUNTS = ("n_obj_correct", "n_sem_correct", "n_pos", "n_neg")
RING_COLS = 5  # VOTENET_MONITOR_RING_COLS (include/votenet_monitors.h): obj_accuracy, sem_accuracy, total_cost, n_pos, n_neg


def votenet_accuracies(out, gt, nh=NH, ns=NS, nc=NC, losses=None, ring=None, ring_row=0, buffers=None, head=None):
    """obj_accuracy and sem_accuracy of one step (model.py:164-166, 215-216) on the device, one launch (votenet_accuracies of
    libvotenet_monitors.so, csrc/monitors/monitors.hip).
    out, gt: as votenet_loss takes them.  -> accuracies (2,) f32, counts (4,) int32 (ACCURACY_COUNTS), both on the device; nothing is
    read back.  losses: the vector votenet_loss returned; with ring (window, RING_COLS) f32 the launch also writes row ring_row of it:
    (obj_accuracy, sem_accuracy, losses[0], n_pos, n_neg).  buffers: (accuracies, counts, workspace) of a caller that keeps them
    (monitors.Monitors; the workspace is 8 int32 zeros, left zero by every launch).  head: as votenet_loss takes it."""
    nh, ns, nc = _head_bins(head, nh, ns, nc)
    pxyz = L.dev_f32(out["proposals_xyz"], "accuracies proposals_xyz", 3, 3)
    pout = L.dev_f32_rows(out["proposals_output"], "accuracies proposals_output")
    b, p = pxyz.shape[:2]
    if pout.shape[2] != 5 + 2 * nh + 4 * ns + nc or tuple(pout.shape[:2]) != (b, p):
        raise L.InvalidArgumentError("accuracies: proposals_output has shape %s, expected (%d, %d, %d)"
                                     % (tuple(pout.shape), b, p, 5 + 2 * nh + 4 * ns + nc))
    gxyz, sem = L.dev_f32(gt["bboxes_xyz"], "accuracies bboxes_xyz", 3, 3), L.dev_i32(gt["semantic_labels"], "accuracies semantic_labels", 2)
    if gxyz.shape[0] != b or tuple(sem.shape) != tuple(gxyz.shape[:2]):
        raise L.InvalidArgumentError("accuracies: ground truth of %s boxes / %s labels for %d scenes" % (tuple(gxyz.shape), tuple(sem.shape), b))
    dev = pxyz.device
    if buffers is not None:
        acc, counts, work = buffers
    else:
        acc = torch.empty(2, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        work = torch.zeros(8, dtype=torch.int32, device=dev)
    if acc.numel() != 2 or counts.numel() != 4 or work.numel() < 8:
        raise L.InvalidArgumentError("accuracies: buffers of the wrong size")
    rows = 0
    if ring is not None:
        ring = L.dev_f32(ring, "accuracies ring", 2, RING_COLS)
        rows = ring.shape[0]
        if not 0 <= ring_row < rows:
            raise L.InvalidArgumentError("accuracies: row %d outside a ring of %d rows" % (ring_row, rows))
    if losses is not None and (losses.numel() != 12 or losses.dtype != torch.float32 or not losses.is_cuda):
        raise L.InvalidArgumentError("accuracies: losses must be the 12 floats of votenet_loss on the device")
    with L.device_guard(dev):
        L.check(L.side_lib("monitors").votenet_accuracies(b, p, gxyz.shape[1], nh, ns, nc, L.ptr(pxyz), L.ptr(pout), pout.stride(1), L.ptr(gxyz), L.ptr(sem),
                                           POSITIVE_THRES, NEGATIVE_THRES, L.ptr(losses), L.ptr(ring), rows, ring_row, L.ptr(acc),
                                           L.ptr(counts), L.ptr(work), L.stream_ptr()), side="monitors")
    return acc, counts


def decode_boxes(proposals_xyz, proposals_output, nh=NH, ns=NS, nc=NC, head=None, mean_sizes=None):
    """model.py:100-129 on the device: -> bboxes (B,P,8,3), scores (B,P) = max class logit (the inputs of NMS3D).
    head: the HeadConfig whose bins and size templates decode (None: the keywords' bins and the default head's templates).
    mean_sizes: the templates as an (ns, 3) float32 tensor already on the device (a net keeps one: VoteNetHotPath.decode_boxes)."""
    nh, ns, nc = _head_bins(head, nh, ns, nc)
    pxyz = L.dev_f32(proposals_xyz, "decode_boxes proposals_xyz", 3, 3)
    pout = L.dev_f32(proposals_output, "decode_boxes proposals_output", 3)
    b, p = pxyz.shape[:2]
    if pout.shape[2] != 5 + 2 * nh + 4 * ns + nc:
        raise L.InvalidArgumentError("decode_boxes: proposals_output has %d channels" % pout.shape[2])
    if mean_sizes is not None:
        mean = L.dev_f32(mean_sizes, "decode_boxes mean_sizes", 2, 3)
        if mean.device != pxyz.device:
            raise L.InvalidArgumentError("decode_boxes: mean_sizes live on another device than the proposals")
    else:
        from .synth import MEAN_SIZES
        mean = torch.tensor(head.mean_sizes_f32 if head is not None else MEAN_SIZES, dtype=torch.float32, device=pxyz.device).contiguous()
    if mean.shape[0] < ns:
        raise L.InvalidArgumentError("decode_boxes: %d size templates for ns = %d" % (mean.shape[0], ns))
    boxes = torch.empty((b, p, 8, 3), dtype=torch.float32, device=pxyz.device)
    scores = torch.empty((b, p), dtype=torch.float32, device=pxyz.device)
    with L.device_guard(pxyz.device):
        L.check(L.lib().votenet_decode_boxes(b, p, nh, ns, nc, L.ptr(pxyz), L.ptr(pout), L.ptr(mean), L.ptr(boxes), L.ptr(scores),
                                             L.stream_ptr()))
    return boxes, scores
