// step_guard.hip -- libvotenet_guard.so: the guarded optimizer step (include/votenet_step_guard.h), a library of its own beside
// libvotenet_hip.so (whose export list is the drop-in ABI of the reference's ops and stays what it was).
//   votenet_clip_adam_guarded   votenet_clip_adam behind a verdict on the gradient: a step whose gradient is not finite writes no
//                               parameter and no Adam moment, puts the BatchNorm moving averages back to their last good copy and is
//                               counted -- all on the device, nothing read back.
// Three launches, one more than votenet_clip_adam:
//   seg_sumsq_kernel            (sumsq.h, the text votenet_clip_adam runs) VOTENET_SUMSQ_SLICES ordered partial sums of squares per tensor
//   step_guard_verdict_kernel   ONE workgroup: any partial NaN / Inf -> bad; any moving average NaN / Inf or a bad step -> restore the
//                               averages from the snapshot, else refresh the snapshot; one lane publishes the verdict word and the
//                               counters with ordinary stores.  3 k partials + 25 k averages: one workgroup's work.
//   clip_adam_guarded_kernel    clip_adam_kernel's arithmetic statement for statement (mlp_bwd.hip; -ffp-contract=off in both), behind one
//                               load of the verdict word: a bad step returns before its first store.
// A NaN or an Inf anywhere in a tensor's gradient reaches at least one of its partials (a square is never negative: nothing cancels), so
// the partials decide; so does a finite element whose square overflows.  The verdict reads what the all-reduce left in g: replicas agree.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#pragma GCC visibility push(default)
#include "../../../include/votenet_step_guard.h"
#pragma GCC visibility pop
#include "../../../include/votenet_hip.h" // VOTENET_SUMSQ_SLICES, the status codes
#include "../error_text.h"

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_step_guard_last_error()) ----
static thread_local ErrorText g_guard_err;
static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
#define VN_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_guard_err, cond, __VA_ARGS__)

#include "../sumsq.h" // seg_sumsq_kernel, kSumsqSlices

// NaN or +-Inf: the exponent field is all ones (a test on the bits: no compiler flag can fold it away)
__device__ __forceinline__ int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

constexpr int GUARD_T = 1024;
__global__ __launch_bounds__(GUARD_T) void step_guard_verdict_kernel(const float *__restrict__ sumsq, int npartials, float *ema,
                                                                     float *snapshot, long n_ema, int step, int *state)
{
    int g_bad = 0, e_bad = 0;
    for (int i = threadIdx.x; i < npartials; i += GUARD_T) g_bad |= nonfinite(sumsq[i]);
    // the averages 16 bytes at a time where both buffers allow it, the rest one by one
    const bool vec = ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(snapshot)) & 15) == 0;
    const long n4 = vec ? n_ema / 4 : 0;
    float4 *ema4 = reinterpret_cast<float4 *>(ema), *snap4 = reinterpret_cast<float4 *>(snapshot);
    for (long i = threadIdx.x; i < n4; i += GUARD_T) {
        const float4 q = ema4[i];
        e_bad |= nonfinite(q.x) | nonfinite(q.y) | nonfinite(q.z) | nonfinite(q.w);
    }
    for (long i = 4 * n4 + threadIdx.x; i < n_ema; i += GUARD_T) e_bad |= nonfinite(ema[i]);
    const int bad = __syncthreads_or(g_bad) != 0;
    const int restore = (bad | (__syncthreads_or(e_bad) != 0)) && n_ema > 0;
    if (restore) { // the averages go back to their last good copy
        for (long i = threadIdx.x; i < n4; i += GUARD_T) ema4[i] = snap4[i];
        for (long i = 4 * n4 + threadIdx.x; i < n_ema; i += GUARD_T) ema[i] = snapshot[i];
    } else { // a good step with finite averages: they are the new good copy
        for (long i = threadIdx.x; i < n4; i += GUARD_T) snap4[i] = ema4[i];
        for (long i = 4 * n4 + threadIdx.x; i < n_ema; i += GUARD_T) snapshot[i] = ema[i];
    }
    if (threadIdx.x == 0) {
        state[VOTENET_STEP_GUARD_VERDICT] = bad;
        state[VOTENET_STEP_GUARD_SEEN] += 1;
        if (bad) {
            state[VOTENET_STEP_GUARD_SKIPPED] += 1;
            state[VOTENET_STEP_GUARD_CONSECUTIVE] += 1;
            state[VOTENET_STEP_GUARD_LAST_SKIP] = step;
        } else {
            state[VOTENET_STEP_GUARD_CONSECUTIVE] = 0;
        }
        if (restore) state[VOTENET_STEP_GUARD_EMA_RESTORES] += 1;
    }
}

// clip_adam_kernel (mlp_bwd.hip) behind the verdict word: the statements below the first are its statements
__global__ void clip_adam_guarded_kernel(const long *__restrict__ seg, const float *__restrict__ sumsq, float *__restrict__ p,
                                         const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, float lr, float b1,
                                         float b2, float eps, float bc1, float bc2, float gscale, float clip,
                                         const int *__restrict__ state)
{
    if (state[VOTENET_STEP_GUARD_VERDICT] != 0) return; // a bad step: p, m and v keep every bit
    const long a = seg[2 * blockIdx.y], b = seg[2 * blockIdx.y + 1];
    float factor = gscale;
    if (clip > 0.0f) {
        float ss = 0.0f;
#pragma unroll
        for (int t = 0; t < kSumsqSlices; t++) ss += sumsq[blockIdx.y * kSumsqSlices + t];
        const float avg = sqrtf(ss) * gscale / (float)(b - a);
        factor = gscale * clip / (avg > clip ? avg : clip);
    }
    const float lr_t = lr * sqrtf(bc2) / bc1;
    for (long i = a + (long)blockIdx.x * blockDim.x + threadIdx.x; i < b; i += (long)gridDim.x * blockDim.x) {
        const float gg = g[i] * factor;
        const float mm = b1 * m[i] + (1.0f - b1) * gg;
        const float vv = b2 * v[i] + (1.0f - b2) * gg * gg;
        m[i] = mm;
        v[i] = vv;
        p[i] -= lr_t * mm / (sqrtf(vv) + eps);
    }
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_step_guard_last_error(void) { return g_guard_err.text; }

extern "C" int votenet_step_guard_state_ints(void) { return VOTENET_STEP_GUARD_STATE_INTS; }

extern "C" int votenet_clip_adam_guarded(int ntensors, const long *seg, float *sumsq_scratch, float *p, const float *g, float *m,
                                         float *v, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                                         float clip_avg_norm, float *ema, float *ema_snapshot, long n_ema, int *guard_state,
                                         void *stream)
{
    VN_REQUIRE(ntensors > 0 && step > 0, "clip_adam_guarded expects ntensors > 0 and step >= 1");
    VN_REQUIRE(seg && sumsq_scratch && p && g && m && v, "clip_adam_guarded: null buffer");
    VN_REQUIRE(guard_state, "clip_adam_guarded: null guard_state");
    VN_REQUIRE(n_ema >= 0 && (n_ema == 0 || (ema && ema_snapshot)), "clip_adam_guarded: n_ema = %ld needs ema and ema_snapshot", n_ema);
    VN_REQUIRE(n_ema == 0 || ema != ema_snapshot, "clip_adam_guarded: ema_snapshot must be a buffer of its own");
    VN_REQUIRE((long)ntensors * kSumsqSlices <= 0x7fffffffL, "clip_adam_guarded: too many tensors");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(seg_sumsq_kernel, dim3(kSumsqSlices, ntensors), dim3(256), 0, st, g, seg, sumsq_scratch);
    hipLaunchKernelGGL(step_guard_verdict_kernel, dim3(1), dim3(GUARD_T), 0, st, sumsq_scratch, ntensors * kSumsqSlices, ema,
                       ema_snapshot, n_ema, step, guard_state);
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    hipLaunchKernelGGL(clip_adam_guarded_kernel, dim3(64, ntensors), dim3(256), 0, st, seg, sumsq_scratch, p, g, m, v, lr, beta1, beta2,
                       eps, bc1, bc2, grad_scale, clip_avg_norm, guard_state);
    return g_guard_err.check_launch("clip_adam_guarded");
}
