/*
 * votenet_monitors.h -- C ABI of libvotenet_monitors.so: the training summaries of a VoteNet run on the MI355X (gfx950), beside
 * libvotenet_hip.so (votenet_hip.h).  A library of its own: libvotenet_hip.so is the drop-in for the reference's op libraries and
 * exports exactly its two headers; a run that wants no summaries never loads this one.  Conventions as in votenet_hip.h: extern "C",
 * every pointer is DEVICE memory, an explicit stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok,
 * 1 = invalid argument, 2 = HIP error; text via votenet_monitors_last_error()), the caller owns every buffer, no launcher allocates
 * or synchronises.
 */
#ifndef VOTENET_MONITORS_H
#define VOTENET_MONITORS_H

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_monitors_last_error(void);

/* The accuracies a training run of the reference prints beside its cost (model.py:164-166 obj_accuracy, :215-216 sem_accuracy, their
 * moving averages run.py:127), from the tensors votenet_loss_pitched reads, in ONE launch, nothing read back.  Positives, negatives
 * and the assigned box exactly as votenet_loss decides them (model.py:148-155: min_dist < pos_thr, min_dist > neg_thr, first arg-min).
 * A positive is obj_correct when class 1 is in the top 1 of its two objectness logits, a negative when class 0 is; a positive is
 * sem_correct when its box's semantic_label is in the top 1 of the nc class logits.  tf.nn.in_top_k: correct iff the target's own
 * score is finite and no other class scores strictly higher (a tie is correct).
 *   counts (4 ints)      n_obj_correct, n_sem_correct, n_pos, n_neg -- integer sums over the workgroups: independent of scheduling;
 *                        n_pos / n_neg equal losses[10:12] of votenet_loss on the same inputs
 *   accuracies (2)       obj_accuracy = n_obj_correct / (n_pos + n_neg), sem_accuracy = n_sem_correct / n_pos (fp32 division); an empty
 *                        denominator gives NaN, as tf.reduce_mean of an empty tensor
 *   ring (may be NULL)   ring_rows x VOTENET_MONITOR_RING_COLS floats: row ring_row (the caller's step % ring_rows) receives
 *                        (obj_accuracy, sem_accuracy, total_cost, n_pos, n_neg), total_cost = losses[0] read on the device (losses: the
 *                        12 floats the loss launch wrote on the same stream; NULL: NaN) -- SimpleMovingAverage's window without a read-back
 *   workspace            VOTENET_ACCURACIES_WORKSPACE_INTS ints, zero before the FIRST launch; every launch leaves them zero. */
#define VOTENET_MONITOR_RING_COLS 5
#define VOTENET_ACCURACIES_WORKSPACE_INTS 8
int votenet_accuracies(int b, int n_prop, int n_box, int nh, int ns, int nc, const float *proposals_xyz,
                       const float *proposals_output, long output_pitch, const float *bboxes_xyz, const int *semantic_labels,
                       float pos_thr, float neg_thr, const float *losses, float *ring, int ring_rows, int ring_row,
                       float *accuracies, int *counts, int *workspace, void *stream);

/* The per-tensor summaries of model.py:236 (add_param_summary: rms and histogram of every weight matrix) and model.py:250
 * (gradproc.SummaryGradient: the same of every gradient) over one flat bucket with votenet_clip_adam's segment table (seg: 2*ntensors
 * element offsets), in ONE launch.  Every element is multiplied by scale first (a gradient bucket: votenet_clip_adam's grad_scale).
 *   stats (ntensors x VOTENET_TENSOR_STATS_FLOATS)  sum, sum of squares, minimum, maximum of the FINITE elements (none: 0, 0, +inf,
 *       -inf), and the factor tf.clip_by_average_norm applies, clip / max(sqrt(sumsq) / numel, clip) (clip_avg_norm <= 0: 1; a tensor
 *       with a non-finite element: NaN).  mean = sum / n, rms = sqrt(sumsq / n) (tensorpack's rms summary) are the caller's.  The
 *       reference summarises the gradient AFTER the clip (model.py:248-250); votenet_clip_adam never stores that one: it is this one
 *       times the factor.
 *   hist (ntensors x VOTENET_TENSOR_STATS_INTS)     [0] the number of non-finite elements, then VOTENET_TENSOR_HIST_BINS exact counts
 *       by sign and binary exponent: bin 0 zeros and subnormals; bin 1 + (e + 40) the positive values of unbiased exponent e clamped
 *       to [-40, 23]; bin 65 + (e + 40) the negative ones; bin 129 inf and NaN.
 * A tensor is summed by one workgroup in one fixed order (16 ordered partials, one per wave): the result is bit-reproducible, so
 * data-parallel replicas holding the same bucket report the same bits.  x: 16-byte aligned. */
#define VOTENET_TENSOR_HIST_BINS 130
#define VOTENET_TENSOR_STATS_FLOATS 5
#define VOTENET_TENSOR_STATS_INTS 131
int votenet_tensor_stats(int ntensors, const long *seg, const float *x, float scale, float clip_avg_norm, float *stats, int *hist,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
