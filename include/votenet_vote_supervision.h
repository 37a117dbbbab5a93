/*
 * votenet_vote_supervision.h -- C ABI of libvotenet_votesup.so: the vote supervision of the VoteNet paper on the MI355X (gfx950), one
 * launch behind votenet_loss (votenet_hip.h).  A library of its own, as libvotenet_monitors.so ... libvotenet_depth.so are: the other
 * libraries export what they did, and a training run that does not ask for the mode never loads this one.  Beyond the reference, whose
 * rule (model.py:62-84) sends every seed that lies in SOME box to the centre of the NEAREST box and divides by all b * n seeds; here a
 * seed votes for the centres of the boxes that contain it, an ambiguous seed keeps up to three targets and is charged the closest, and
 * the sum is divided by the number of supervised seeds.  Conventions as in votenet_hip.h: extern "C", an explicit stream (hipStream_t
 * as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error; text via
 * votenet_votesup_last_error()), the caller owns every buffer, no launcher allocates or synchronises, nothing is read back.
 *
 * The rule.  All tensors float32, contiguous: seeds (b, n, 3), votes (b, n, 3), xyz (b, bb, 3) box centres, lwh (b, bb, 3) as (l, w, h),
 * roty (b, bb).  1 <= b <= 65535, n >= 1, b * n * 3 < 2^31, 1 <= bb <= 256.
 *   per box:   c = float(cos(double(roty))), s = float(sin(double(roty)));  hl = 0.5f * l, hw = 0.5f * w, hh = 0.5f * h
 *   per seed p and box j, fp32, un-fused, in this order:
 *              qx = px - cx, qy = py - cy, qz = pz - cz;  x0 = c * qx - s * qz;  z0 = s * qx + c * qz
 *              inside  iff  |x0| <= hl && |qy| <= hh && |z0| <= hw
 * The closed box: a seed on a face is inside; a NaN fails every comparison.  (The interior of the box whose corners
 * evaluator.box_corners(centre, lwh, roty) draws.)  With j1 < j2 < ... < jk the boxes that contain the seed, in index order:
 *   slot 0 = j1;  slot 1 = j2 if k >= 2, else j1;  slot 2 = jk (the last) if k >= 3, else j1;  supervised iff k >= 1.
 * Ground truth padded by repeating a scene's last box therefore gives the same set of target centres as the unpadded lists.
 */
#ifndef VOTENET_VOTE_SUPERVISION_H
#define VOTENET_VOTE_SUPERVISION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_votesup_last_error(void);

/* The slots of every seed, for inspection and tests: slots (b, n, 3) int32, the box indices of slots 0, 1, 2 (all three -1 where
 * k = 0); inside_count (b, n) int32, the uncapped k.  Both written in full.  One launch. */
int votenet_vote_targets(int b, int n, int bb, const float *seeds, const float *xyz, const float *lwh, const float *roty, int *slots,
                         int *inside_count, void *stream);

/* Bytes of votenet_paper_vote_loss's workspace for b scenes (b <= 0: the fixed part).  ZERO on entry, left zero by every launch. */
size_t votenet_votesup_workspace_bytes(int b);

/* The paper's vote regression loss and its cotangent, behind votenet_loss on the same stream:
 *   d = (|vx - tx| + |vy - ty|) + |vz - tz| to a slot's centre t; a supervised seed takes the FIRST strict minimum over slots 0, 1, 2;
 *   P = the supervised seeds of the whole batch (an integer, exact);  inv = 1.0f / (float(P) + 1e-6f);
 *   L = (the sum of the minima over the supervised seeds) * inv;
 *   d_votes[e][k] = sgn(v_k - t_k) * inv for a supervised seed, sgn(x) = (x > 0) - (x < 0) (0 for 0 and for NaN, written 0.0f * inv);
 *   +0.0f for every other seed.  P = 0: L = 0 and an all-zero cotangent.
 * losses: the 12 floats of votenet_loss, read and written in place: losses[1] = L, losses[0] = L + 0.5f * losses[2] + losses[9] +
 * 0.1f * losses[8] (the expression and the order of votenet_loss's total); losses[2..11] are not written.  d_votes (b, n, 3): written
 * in full, may not overlap votes.  supervised: NULL, or one int32 that receives P.  workspace: votenet_votesup_workspace_bytes(b)
 * bytes, 4-byte aligned.
 * One launch, one workgroup per scene: every workgroup counts P of the whole batch itself and scales its own scene's cotangents; the
 * per-scene sums are formed in a fixed order and folded in scene order by the last workgroup to finish (an integer ticket).  No float
 * atomic: two calls write the same bytes. */
int votenet_paper_vote_loss(int b, int n, int bb, const float *seeds, const float *votes, const float *xyz, const float *lwh,
                            const float *roty, float *losses, float *d_votes, int *supervised, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_VOTE_SUPERVISION_H */
