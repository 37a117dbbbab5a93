/*
 * votenet_instance_votes.h -- C ABI of libvotenet_instvote.so: vote supervision from instance labels on the MI355X (gfx950), one launch
 * behind votenet_loss (votenet_hip.h).  A library of its own, as libvotenet_votesup.so is: the other libraries export what they did,
 * and a training run that does not ask for the mode never loads this one.  Both rules the project had decide a seed's target by
 * geometry (votenet_loss: the nearest box of a seed that lies in some box; votenet_paper_vote_loss: the boxes that contain it).  On
 * ground truth made from instance-labelled points (votenet_instance_boxes.h) the boxes are the axis-aligned hulls of the instances:
 * they overlap, and they hold points that belong to nothing.  Here a seed votes for the centre of the box of ITS OWN instance, and a
 * seed without an instance is not supervised: the paper's rule for its second benchmark.  Conventions as in votenet_hip.h: extern "C",
 * an explicit stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error; text
 * via votenet_instvote_last_error()), the caller owns every buffer, no launcher allocates or synchronises, nothing is read back, and
 * every argument is checked before any HIP call.
 *
 * The rule.  All tensors contiguous:
 *   idx1      (b, n1) int32   sa1's picks into the cloud of n0 points
 *   idx2      (b, n)  int32   sa2's picks into sa1's n1 centres: seed j of scene s is cloud point idx1[s][idx2[s][j]]
 *   point_box (b, n0) int32   the row of each cloud point's box within its scene, negative for none (votenet_instance_point_box)
 *   votes     (b, n, 3) f32;  xyz (b, bb, 3) f32 box centres (gt bboxes_xyz)
 * 1 <= b <= 65535, n, n1, n0 >= 1, b * n * 3 < 2^31, b * n0 < 2^31, 1 <= bb <= 256.
 * Per seed j of scene s:
 *   i = idx2[s][j], valid iff 0 <= i < n1;  then p = idx1[s][i], valid iff 0 <= p < n0;  then r = point_box[s][p].
 *   seed_point[s][j] = p if both are valid, else -1.
 *   supervised iff the chain is valid and 0 <= r < bb.  A seed whose chain is invalid, or whose r >= bb, is unsupervised and counted
 *   in the diagnostic count Q; a negative r is an unlabelled point and is not counted.
 * No index value (INT_MIN and INT_MAX included) addresses anything before it has been compared with its bound: an index that fails is
 * replaced by 0 and its result discarded.
 * The target of a supervised seed is t = xyz[s][r]: one target per seed.  (augment_boxes keeps the row order and pads a scene by
 * repeating its last box at the end, so r indexes the padded ground truth directly.)
 */
#ifndef VOTENET_INSTANCE_VOTES_H
#define VOTENET_INSTANCE_VOTES_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_instvote_last_error(void);

/* The cloud point every seed is, for inspection and tests: seed_point (b, n) int32, written in full (-1 where an index of the chain is
 * out of range).  One elementwise launch. */
int votenet_seed_points(int b, int n0, int n1, int n, const int *idx1, const int *idx2, int *seed_point, void *stream);

/* Bytes of votenet_instance_vote_loss's workspace for b scenes (b <= 0: the fixed part).  ZERO on entry, left zero by every launch. */
size_t votenet_instvote_workspace_bytes(int b);

/* The vote regression loss towards the seeds' own instances and its cotangent, behind votenet_loss on the same stream; the loss and
 * the cotangent are votenet_paper_vote_loss's with a single slot, operation for operation:
 *   d = (|vx - tx| + |vy - ty|) + |vz - tz|;
 *   P = the supervised seeds of the whole batch (an integer, exact);  inv = 1.0f / (float(P) + 1e-6f);
 *   L = (the sum of d over the supervised seeds) * inv;
 *   d_votes[e][k] = sgn(v_k - t_k) * inv for a supervised seed, sgn(x) = (x > 0) - (x < 0) (0 for 0 and for NaN, written 0.0f * inv);
 *   +0.0f for every other seed.  P = 0: L = 0 and an all-zero cotangent.
 * losses: the 12 floats of votenet_loss, read and written in place: losses[1] = L, losses[0] = L + 0.5f * losses[2] + losses[9] +
 * 0.1f * losses[8] (the expression and the order of votenet_loss's total); losses[2..11] are not written.  d_votes (b, n, 3): written
 * in full, may not overlap votes.  counts: NULL, or two int32 that receive P and Q.  workspace:
 * votenet_instvote_workspace_bytes(b) bytes, 4-byte aligned.
 * One launch, one workgroup per scene: every workgroup counts P of the whole batch itself and scales its own scene's cotangents; the
 * per-scene sums are formed in a fixed order and folded in scene order by the last workgroup to finish (an integer ticket).  No float
 * atomic: two calls write the same bytes. */
int votenet_instance_vote_loss(int b, int n0, int n1, int n, int bb, const int *idx1, const int *idx2, const int *point_box,
                               const float *votes, const float *xyz, float *losses, float *d_votes, int *counts, void *workspace,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_INSTANCE_VOTES_H */
