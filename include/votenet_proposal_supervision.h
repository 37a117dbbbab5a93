/*
 * votenet_proposal_supervision.h -- C ABI of libvotenet_propsup.so: the objectness and centre supervision of the VoteNet paper on the
 * MI355X (gfx950), one launch behind votenet_loss (votenet_hip.h).  A library of its own, as libvotenet_monitors.so ...
 * libvotenet_votesup.so are: the other libraries export what they did, and a training run that does not ask for the mode never loads this
 * one.  Beyond the reference, whose objectness (model.py:157-163) is mean over positives(CE) + mean over negatives(CE), NaN where a set
 * is empty, and whose centre term (model.py:168-182) is a Huber loss of the predicted offset against the box assigned by the cluster
 * POSITION plus the same Huber for each ground-truth row's nearest cluster position, averaged over all b * bb padded rows; here the
 * objectness is one class-weighted cross-entropy over all proposals outside the grey zone, and the centre term a Chamfer distance between
 * the PREDICTED centres and the real ground-truth centres.  Conventions as in votenet_hip.h: extern "C", an explicit stream (hipStream_t
 * as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error; text via
 * votenet_propsup_last_error()), the caller owns every buffer, no launcher allocates or synchronises, nothing is read back.
 *
 * The rule.  All tensors float32: proposals_xyz (b, p, 3) contiguous; proposals_output rows of width W = 5 + 2 nh + 4 ns + nc,
 * output_pitch >= W floats apart, read in place as votenet_loss_pitched reads it; bboxes_xyz (b, bb, 3) contiguous.
 * 1 <= b <= 65535, 1 <= p <= 1024, 1 <= bb <= 256, 0 < nh, ns, nc <= 32, pos_thr < neg_thr as votenet_loss takes them.  All arithmetic
 * fp32, un-fused, in the order written.
 *   real boxes of scene s:  g_s = bb; while g_s > 1 and row g_s - 1's centre equals row g_s - 2's (three ==): g_s -= 1 -- the rule
 *              evaluator.gt_for_eval uses for ground truth padded by repeating the last box.  G = the sum of g_s over the batch.
 *   labels:    the reference's, by the same instructions: dmin_i over ALL bb rows by nearest_box (csrc/nearest_box.h) on
 *              proposals_xyz[s, i]; positive iff dmin_i < pos_thr, negative iff dmin_i > neg_thr, otherwise grey (a NaN is grey).
 *              Np, Nn: the batch's counts (what votenet_loss leaves in losses[10], losses[11]); M = Np + Nn;
 *              inv_m = 1.0f / (float(M) + 1e-6f), inv_p = 1.0f / (float(Np) + 1e-6f), inv_g = 1.0f / (float(G) + 1e-6f).
 *   objectness: y = 1 for a positive, 0 for a negative; w_1 = 0.8f, w_0 = 0.2f; o0, o1 = columns 0, 1;
 *              mx = max(o0, o1); e_k = expf(o_k - mx); s = e0 + e1; lse = mx + logf(s); ce = lse - o_y;
 *              obj = (the sum over positives and negatives of w_y * ce) * inv_m;
 *              cotangent of the TOTAL cost (objectness has weight 0.5 in it), with r = 1.0f / s:
 *              d_o_k = ((0.5f * w_y) * (e_k * r - [k == y])) * inv_m; a grey proposal: +0.0f in both.  M = 0: obj = 0 and zeros.
 *   centre:    c_i = proposals_xyz[s, i] + proposals_output[s, i, 2:5] per component;
 *              q_ij = ((cx - gx) * (cx - gx) + (cy - gy) * (cy - gy)) + (cz - gz) * (cz - gz) against box row j's centre;
 *              minima as nearest_box.h takes them, `first || q < best`: the first minimum in index order wins, a NaN in the first
 *              candidate sticks.  Positive i: e_i = min over j < g_s of q_ij, at j1(i).  Real box j < g_s: f_j = min over ALL i < p of
 *              q_ij, at i2(j).  center = (the sum of e_i over the positives) * inv_p + (the sum of f_j over the real boxes) * inv_g.
 *              cotangent per component k: (2.0f * (c_ik - g_{j1(i),k})) * inv_p for a positive i, +0.0f otherwise; then, for
 *              j = 0 .. g_s - 1 in ascending order, where i2(j) == i: += (2.0f * (c_ik - g_jk)) * inv_g.
 * Beside the paper: its matching against zero-padded box slots is not taken over (padding here is edge repetition, counted once).
 */
#ifndef VOTENET_PROPOSAL_SUPERVISION_H
#define VOTENET_PROPOSAL_SUPERVISION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_propsup_last_error(void);

/* The decisions of the rule, for inspection and tests, all int32 and all written in full: label (b, p): 1, 0, or -1 for grey; near_box
 * (b, p): j1(i) for a positive, else -1; dual_prop (b, bb): i2(j) for j < g_s, else -1; real_boxes (b): g_s.  Only columns 2..4 of
 * proposals_output are read (output_pitch >= 5).  One launch, one workgroup per scene. */
int votenet_proposal_targets(int b, int p, int bb, const float *proposals_xyz, const float *proposals_output, long output_pitch,
                             const float *bboxes_xyz, float pos_thr, float neg_thr, int *label, int *near_box, int *dual_prop,
                             int *real_boxes, void *stream);

/* Bytes of votenet_paper_proposal_loss's workspace for b scenes (b <= 0: the fixed part).  ZERO on entry, left zero by every launch. */
size_t votenet_propsup_workspace_bytes(int b);

/* The paper's objectness and centre terms and their cotangents, behind votenet_loss on the same stream.
 * d_proposals_output (b, p, W) DENSE: columns 0..4 of every row are overwritten (0, 1: objectness; 2..4: centre), columns 5..W are not
 * touched.  d_proposals_xyz (b, p, 3): overwritten in full with the bits of columns 2..4.  Neither may overlap the tensor it is the
 * cotangent of.  losses: the 12 floats of votenet_loss, read and written in place, in votenet_loss's expressions and order:
 *   losses[2] = obj;  losses[3] = center;
 *   losses[9] = (((losses[3] + 0.1f * losses[4]) + losses[5]) + 0.1f * losses[6]) + losses[7];
 *   losses[0] = ((losses[1] + 0.5f * losses[2]) + losses[9]) + 0.1f * losses[8];
 * losses[1], [4..8], [10], [11] are not written.  counts: NULL, or three int32 that receive Np, Nn, G.  workspace:
 * votenet_propsup_workspace_bytes(b) bytes, 4-byte aligned.
 * One launch, one workgroup per scene, a proposal per lane: every workgroup counts Np, Nn and G of the whole batch itself (integers:
 * all arrive at the same values) and scales its own scene's cotangents; the per-scene sums are formed in a fixed order and folded in
 * scene order by the last workgroup to finish (an integer ticket).  No float atomic, no scatter: two calls write the same bytes. */
int votenet_paper_proposal_loss(int b, int p, int bb, int nh, int ns, int nc, const float *proposals_xyz, const float *proposals_output,
                                long output_pitch, const float *bboxes_xyz, float pos_thr, float neg_thr, float *losses,
                                float *d_proposals_xyz, float *d_proposals_output, int *counts, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_PROPOSAL_SUPERVISION_H */
