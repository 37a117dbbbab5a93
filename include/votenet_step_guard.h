/*
 * votenet_step_guard.h -- C ABI of libvotenet_guard.so: the guarded optimizer step of a VoteNet run on the MI355X (gfx950), beside
 * libvotenet_hip.so (votenet_hip.h).  A library of its own, as libvotenet_monitors.so is: libvotenet_hip.so is the drop-in for the
 * reference's op libraries and exports exactly its two headers; a run that enables no guard never loads this one.  Conventions as in
 * votenet_hip.h: extern "C", every pointer is DEVICE memory, an explicit stream (hipStream_t as void*; NULL = the null stream), an int
 * status (0 = ok, 1 = invalid argument, 2 = HIP error; text via votenet_step_guard_last_error()), the caller owns every buffer, no
 * launcher allocates or synchronises, nothing is read back.
 */
#ifndef VOTENET_STEP_GUARD_H
#define VOTENET_STEP_GUARD_H

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_step_guard_last_error(void);

/* The guard's device state: VOTENET_STEP_GUARD_STATE_INTS int32 (what votenet_step_guard_state_ints() returns), zero before the first
 * guarded step.  Diagnostics: no part of a checkpoint. */
#define VOTENET_STEP_GUARD_VERDICT 0       /* the last step's verdict: 0 good, 1 bad (what the update launch reads) */
#define VOTENET_STEP_GUARD_SEEN 1          /* guarded steps seen */
#define VOTENET_STEP_GUARD_SKIPPED 2       /* ... of which skipped */
#define VOTENET_STEP_GUARD_CONSECUTIVE 3   /* skips in a row up to and including the last step; a good step resets it to 0 */
#define VOTENET_STEP_GUARD_LAST_SKIP 4     /* `step` of the last skipped step (0: none yet) */
#define VOTENET_STEP_GUARD_EMA_RESTORES 5  /* times ema was overwritten with ema_snapshot */
#define VOTENET_STEP_GUARD_STATE_INTS 8
int votenet_step_guard_state_ints(void);

/* votenet_clip_adam (votenet_hip.h: same arguments, same meaning, same arithmetic) behind a verdict on the gradient, in three
 * launches -- one more than votenet_clip_adam: the per-tensor partial sums of squares (votenet_clip_adam's own kernel, run whatever
 * clip_avg_norm is; the clip is applied only when clip_avg_norm > 0), a one-workgroup verdict launch, the update.
 *
 * Verdict.  The step is BAD iff any of the VOTENET_SUMSQ_SLICES * ntensors partial sums is NaN or +-Inf.  The partials are those of g
 * as it is handed in (in a data-parallel run: the all-reduced bucket), so replicas that hold the same g decide alike; nothing else
 * takes part -- not the loss, not ema.  A finite gradient whose squares overflow fp32 (|g| >~ 1.8e19) is bad as well.  An all-zero
 * gradient is good.
 * Bad step.   p, m and v are not written at all (the update launch returns before its first store: no x = x store, a -0.0, a
 *             denormal or a NaN payload keeps its bits).
 * Good step.  p, m and v are bit-identical to what votenet_clip_adam leaves from the same inputs and the same `step`.  `step` is the
 *             caller's count of CALLS, skipped or not (TensorFlow's global_step): after a skip Adam's bias correction runs one ahead
 *             of the number of applied updates.
 * Moving averages (ema, ema_snapshot: n_ema floats each; n_ema = 0 with NULL pointers: no such buffers, nothing done).  When the
 *             step is good AND every element of ema is finite, ema_snapshot becomes a copy of ema.  Otherwise ema becomes a copy of
 *             ema_snapshot and EMA_RESTORES counts one.  The caller fills ema_snapshot before the first step (and again whenever it
 *             rewrites ema itself).  Per replica: BatchNorm statistics are never all-reduced.
 * guard_state: see above; SEEN += 1; bad: SKIPPED += 1, CONSECUTIVE += 1, LAST_SKIP = step; good: CONSECUTIVE = 0.  One lane writes
 *             it with ordinary stores.
 * sumsq_scratch: VOTENET_SUMSQ_SLICES * ntensors floats, as votenet_clip_adam's. */
int votenet_clip_adam_guarded(int ntensors, const long *seg, float *sumsq_scratch, float *p, const float *g, float *m, float *v,
                              float lr, float beta1, float beta2, float eps, int step, float grad_scale, float clip_avg_norm,
                              float *ema, float *ema_snapshot, long n_ema, int *guard_state, void *stream);

#ifdef __cplusplus
}
#endif
#endif
