// monitors.hip -- libvotenet_monitors.so: the training summaries of a run (include/votenet_monitors.h), a library of its own beside
// libvotenet_hip.so (whose export list is the drop-in ABI of the reference's ops and stays what it was).
//   votenet_accuracies    obj_accuracy / sem_accuracy of a step (model.py:164-166, 215-216) + the row of the moving-average ring (run.py:127)
//   votenet_tensor_stats  rms / extrema / histogram of every weight matrix and gradient (model.py:236 add_param_summary, model.py:250
//                         gradproc.SummaryGradient; tensorpack's rms = sqrt(mean(x^2))) over one flat bucket with votenet_clip_adam's
//                         segment table: ONE launch, one workgroup per tensor.
// Tensor statistics, per tensor: sum, sum of squares, minimum and maximum of the finite elements, the number of non-finite ones, the factor
// tf.clip_by_average_norm would apply (model.py:249) and an exact histogram by sign and binary exponent (integer counts: no order, no
// rounding).  The reference's histogram is TensorBoard's display format (1.1-ratio buckets); this one is a result.
// A tensor is summed by ONE workgroup in ONE order -- thread t takes the 16-byte vectors t, t + 1024, ...; lanes are combined by
// shuffles, the sixteen waves' partials in wave order -- so two runs, and two data-parallel replicas that hold the same bucket, give
// the same bits; nothing is exchanged between workgroups.  The bucket is 3.8 MB: the launch is latency, not traffic.
#include <hip/hip_runtime.h>
#include <cstdint>
#pragma GCC visibility push(default)
#include "../../../include/votenet_monitors.h"
#pragma GCC visibility pop
#include "../error_text.h" // (with include/votenet_hip.h for the status codes only)
#include "../nearest_box.h"

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_monitors_last_error()) ----
static thread_local ErrorText g_mon_err;
static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
#define VN_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_mon_err, cond, __VA_ARGS__)

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_monitors_last_error(void) { return g_mon_err.text; }

// ---------------------------------------------------------------- the step's accuracies (model.py:164-166, 215-216; run.py:127)
namespace votenet {

constexpr int ACC_T = 256;
constexpr int ACC_MAXC = 32; // nh, ns, nc <= 32, as votenet_loss

struct AccArgs {
    int p, bb, nc;
    const float *pxyz, *pout;
    long pout_pitch;
    const float *gxyz;
    const int *sem;
    float pos_thr, neg_thr;
    const float *losses; // the loss launch's output (total_cost at [0]) or NULL
    float *ring;         // window x VOTENET_MONITOR_RING_COLS or NULL
    int ring_row;
    float *acc;          // 2
    int *counts;         // 4
    int *work;           // VOTENET_ACCURACIES_WORKSPACE_INTS: four counters, the ticket; zero between launches
    int off;             // channel of the first semantic logit
};

// tf.nn.in_top_k(predictions, target, k = 1): the target's score is finite and no other class scores strictly higher (a tie is correct)
__device__ __forceinline__ bool in_top_1(const float *lg, int c, int target)
{
    if (target < 0 || target >= c) return false;
    const float t = lg[target];
    if ((__float_as_uint(t) & 0x7F800000u) == 0x7F800000u) return false;
    bool ok = true;
    for (int i = 0; i < c; i++) ok = ok && !(lg[i] > t);
    return ok;
}

// One workgroup per scene, one proposal per thread: the assignment of votenet_loss_count_kernel (loss.hip: the same nearest_box of nearest_box.h, same thresholds),
// the two in_top_k tests, wave64 ballots for the four counts -> one integer atomic per counter and workgroup (order-independent).  The
// last workgroup to take a ticket forms the two ratios, appends the ring row and clears the counters for the next launch.  Everything
// workgroups exchange goes through agent-scope atomics (the argument of coef_tail in common.h: atomics execute at the memory side, no fence needed).
__global__ __launch_bounds__(ACC_T) void votenet_accuracies_kernel(AccArgs A)
{
    __shared__ float s_box[LOSS_MAXBOX][8];
    __shared__ int s_cnt[ACC_T / 64][4];
    __shared__ int s_last;
    const int b = blockIdx.x, tid = threadIdx.x, BB = A.bb, P = A.p;
    for (int j = tid; j < BB; j += ACC_T)
        for (int k = 0; k < 3; k++) s_box[j][k] = A.gxyz[(b * BB + j) * 3 + k];
    __syncthreads();
    int c_obj = 0, c_sem = 0, c_pos = 0, c_neg = 0; // wave-uniform
    for (int base = 0; base < P; base += ACC_T) {
        const int pq = base + tid;
        bool pos = false, neg = false, obj_ok = false, sem_ok = false;
        if (pq < P) {
            const int q = b * P + pq;
            int g;
            const float best = nearest_box(s_box, BB, A.pxyz[q * 3 + 0], A.pxyz[q * 3 + 1], A.pxyz[q * 3 + 2], g);
            const float *o = A.pout + (size_t)q * A.pout_pitch;
            pos = best < A.pos_thr;
            neg = best > A.neg_thr;
            if (pos || neg) obj_ok = in_top_1(o, 2, pos ? 1 : 0);
            if (pos) sem_ok = in_top_1(o + A.off, A.nc, A.sem[b * BB + g]);
        }
        c_obj += __popcll(__ballot(obj_ok));
        c_sem += __popcll(__ballot(sem_ok));
        c_pos += __popcll(__ballot(pos));
        c_neg += __popcll(__ballot(neg));
    }
    if ((tid & 63) == 0) {
        s_cnt[tid >> 6][0] = c_obj;
        s_cnt[tid >> 6][1] = c_sem;
        s_cnt[tid >> 6][2] = c_pos;
        s_cnt[tid >> 6][3] = c_neg;
    }
    __syncthreads();
    if (tid < 4) {
        int v = 0;
        for (int w = 0; w < ACC_T / 64; w++) v += s_cnt[w][tid];
        if (v) __hip_atomic_fetch_add(&A.work[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this workgroup's additions are acknowledged before it takes its ticket
    __syncthreads();
    if (tid == 0) s_last = (__hip_atomic_fetch_add(&A.work[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1);
    __syncthreads();
    if (!s_last || tid != 0) return;
    int c[4];
    for (int i = 0; i < 4; i++) {
        c[i] = __hip_atomic_load(&A.work[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        A.counts[i] = c[i];
    }
    for (int i = 0; i < 5; i++) __hip_atomic_store(&A.work[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float obj_acc = (float)c[0] / (float)(c[2] + c[3]); // 0 / 0 = NaN: tf.reduce_mean of an empty tensor
    const float sem_acc = (float)c[1] / (float)c[2];
    A.acc[0] = obj_acc;
    A.acc[1] = sem_acc;
    if (A.ring) {
        float *r = A.ring + (size_t)A.ring_row * VOTENET_MONITOR_RING_COLS;
        r[0] = obj_acc;
        r[1] = sem_acc;
        r[2] = A.losses ? A.losses[0] : __uint_as_float(0x7FC00000u);
        r[3] = (float)c[2];
        r[4] = (float)c[3];
    }
}

} // namespace votenet

extern "C" int votenet_accuracies(int b, int n_prop, int n_box, int nh, int ns, int nc, const float *proposals_xyz,
                                  const float *proposals_output, long output_pitch, const float *bboxes_xyz,
                                  const int *semantic_labels, float pos_thr, float neg_thr, const float *losses, float *ring,
                                  int ring_rows, int ring_row, float *accuracies, int *counts, int *workspace, void *stream)
{
    VN_REQUIRE(b > 0 && n_prop > 0 && n_box > 0, "votenet_accuracies expects b, n_prop, n_box > 0");
    VN_REQUIRE(n_box <= LOSS_MAXBOX, "votenet_accuracies expects at most 256 boxes per scene");
    VN_REQUIRE(nh > 0 && ns > 0 && nc > 0 && nh <= ACC_MAXC && ns <= ACC_MAXC && nc <= ACC_MAXC, "votenet_accuracies expects 0 < nh, ns, nc <= 32");
    VN_REQUIRE(pos_thr < neg_thr, "votenet_accuracies expects pos_thr < neg_thr (config.py)");
    VN_REQUIRE(proposals_xyz && proposals_output && bboxes_xyz && semantic_labels && accuracies && counts && workspace,
               "votenet_accuracies: null buffer");
    VN_REQUIRE(output_pitch >= 5 + 2 * nh + 4 * ns + nc, "votenet_accuracies: the pitch of proposals_output is smaller than its width");
    VN_REQUIRE(!ring || (ring_rows > 0 && ring_row >= 0 && ring_row < ring_rows), "votenet_accuracies: ring_row outside the ring");
    AccArgs a = {n_prop, n_box, nc, proposals_xyz, proposals_output, output_pitch, bboxes_xyz, semantic_labels, pos_thr, neg_thr, losses,
                 ring, ring_row, accuracies, counts, workspace, 5 + 2 * nh + 4 * ns};
    hipLaunchKernelGGL(votenet_accuracies_kernel, dim3(b), dim3(ACC_T), 0, as_stream(stream), a);
    return g_mon_err.check_launch("votenet_accuracies");
}

// ---------------------------------------------------------------- per-tensor statistics

namespace votenet {

constexpr int TS_T = 1024;
constexpr int TS_W = TS_T / 64; // the ordered partials per tensor
constexpr int TS_BINS = VOTENET_TENSOR_HIST_BINS;
static_assert(TS_BINS == 130, "1 zero bin + 2 signs x 64 exponents + 1 non-finite bin");

// a total order on fp32 bit patterns as signed integers: the minimum / maximum are exact whatever the denormal mode
__device__ __forceinline__ int order_key(unsigned u) { return (int)(u ^ (((int)u >> 31) & 0x7FFFFFFF)); }

struct TsAcc {
    float sum, sumsq;
    int kmin, kmax, bad;
};

__global__ __launch_bounds__(TS_T) void tensor_stats_kernel(const long *__restrict__ seg, const float *__restrict__ x, float scale,
                                                            float clip, float *__restrict__ stats, int *__restrict__ hist)
{
    __shared__ int s_hist[TS_W][TS_BINS];
    __shared__ float s_f[TS_W][2];
    __shared__ int s_i[TS_W][3];
    const int tid = threadIdx.x, wave = tid >> 6, t = blockIdx.x;
    const long a = seg[2 * t], b = seg[2 * t + 1];
    for (int i = tid; i < TS_W * TS_BINS; i += TS_T) (&s_hist[0][0])[i] = 0;
    __syncthreads();
    TsAcc A = {0.0f, 0.0f, order_key(0x7F800000u), order_key(0xFF800000u), 0}; // min = +inf, max = -inf: no finite element
    const bool scaled = scale != 1.0f;
    auto take = [&](float raw) {
        const float v = scaled ? raw * scale : raw;
        const unsigned u = __float_as_uint(v);
        const int ex = (int)((u >> 23) & 0xFFu);
        int bin;
        if (ex == 0xFF) {
            bin = TS_BINS - 1;
            A.bad++;
        } else {
            if (ex == 0) {
                bin = 0; // zero, or a subnormal
            } else {
                int e = ex - 127;
                e = e < -40 ? -40 : (e > 23 ? 23 : e);
                bin = 1 + (e + 40) + ((u >> 31) ? 64 : 0);
            }
            A.sum += v;
            A.sumsq += v * v;
            const int k = order_key(u);
            A.kmin = k < A.kmin ? k : A.kmin;
            A.kmax = k > A.kmax ? k : A.kmax;
        }
        atomicAdd(&s_hist[wave][bin], 1);
    };
    // [a, a4) and [b4, b): the elements outside the 16-byte aligned body (at most three each)
    long a4 = (a + 3) & ~3L, b4 = b & ~3L;
    if (a4 > b) a4 = b;
    if (b4 < a4) b4 = a4;
    const float4 *xv = reinterpret_cast<const float4 *>(x);
    for (long i = a4 / 4 + tid; i < b4 / 4; i += TS_T) {
        const float4 v = xv[i];
        take(v.x);
        take(v.y);
        take(v.z);
        take(v.w);
    }
    if (tid < 3 && a + tid < a4) take(x[a + tid]);
    if (tid >= 64 && tid < 67 && b4 + (tid - 64) < b) take(x[b4 + (tid - 64)]);
    // lanes -> wave (shuffles, fixed order) -> the waves in order
    for (int off = 32; off > 0; off >>= 1) {
        A.sum += __shfl_down(A.sum, off);
        A.sumsq += __shfl_down(A.sumsq, off);
        const int omin = __shfl_down(A.kmin, off), omax = __shfl_down(A.kmax, off);
        A.kmin = omin < A.kmin ? omin : A.kmin;
        A.kmax = omax > A.kmax ? omax : A.kmax;
        A.bad += __shfl_down(A.bad, off);
    }
    if ((tid & 63) == 0) {
        s_f[wave][0] = A.sum;
        s_f[wave][1] = A.sumsq;
        s_i[wave][0] = A.kmin;
        s_i[wave][1] = A.kmax;
        s_i[wave][2] = A.bad;
    }
    __syncthreads();
    if (tid < TS_BINS) {
        int n = 0;
        for (int w = 0; w < TS_W; w++) n += s_hist[w][tid];
        hist[(size_t)t * VOTENET_TENSOR_STATS_INTS + 1 + tid] = n;
    }
    if (tid == 0) {
        float sum = 0.0f, sumsq = 0.0f;
        int kmin = s_i[0][0], kmax = s_i[0][1], bad = 0;
        for (int w = 0; w < TS_W; w++) {
            sum += s_f[w][0];
            sumsq += s_f[w][1];
            kmin = s_i[w][0] < kmin ? s_i[w][0] : kmin;
            kmax = s_i[w][1] > kmax ? s_i[w][1] : kmax;
            bad += s_i[w][2];
        }
        float factor = 1.0f; // tf.clip_by_average_norm: clip / max(||x||_2 / numel, clip), as clip_adam_kernel forms it
        if (clip > 0.0f) {
            const float avg = sqrtf(sumsq) / (float)(b - a);
            factor = clip / (avg > clip ? avg : clip);
        }
        if (bad) factor = __uint_as_float(0x7FC00000u); // a non-finite gradient has no norm
        float *o = stats + (size_t)t * VOTENET_TENSOR_STATS_FLOATS;
        o[0] = sum;
        o[1] = sumsq;
        o[2] = __uint_as_float((unsigned)kmin ^ ((unsigned)(kmin >> 31) & 0x7FFFFFFFu));
        o[3] = __uint_as_float((unsigned)kmax ^ ((unsigned)(kmax >> 31) & 0x7FFFFFFFu));
        o[4] = factor;
        hist[(size_t)t * VOTENET_TENSOR_STATS_INTS] = bad;
    }
}

} // namespace votenet


extern "C" int votenet_tensor_stats(int ntensors, const long *seg, const float *x, float scale, float clip_avg_norm, float *stats,
                                    int *hist, void *stream)
{
    VN_REQUIRE(ntensors > 0, "tensor_stats expects ntensors > 0");
    VN_REQUIRE(seg && x && stats && hist, "tensor_stats: null buffer");
    VN_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, "tensor_stats: the bucket must be 16-byte aligned");
    hipLaunchKernelGGL(tensor_stats_kernel, dim3(ntensors), dim3(TS_T), 0, as_stream(stream), seg, x, scale, clip_avg_norm, stats, hist);
    return g_mon_err.check_launch("tensor_stats");
}
