// det_emit.h -- the part of a class-wise NMS that does not depend on its overlap: the limits, the class of a box and the launch that
// turns a scene's kept boxes into detection rows.  One text for the two translation units that compile it, detections.hip
// (libvotenet_detect.so, rotated-box IoU) and ../aabb/aabb_nms.hip (libvotenet_aabb.so, axis-aligned overlaps), as ../sumsq.h and
// ../augment_points.h are shared: both libraries write the same rows for the same kept boxes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace votenet {

constexpr int DET_MAX_N = 512;       // boxes of one scene: one thread each, the suppression rows fit LDS (512 x 8 words = 32 KiB)
constexpr int DET_MAX_NC = 64;
constexpr int DET_NMS_THREADS = 512; // >= DET_MAX_N
constexpr int DET_MAX_W = DET_MAX_N / 64;

// the first largest logit; a NaN never wins over a number (eval_match.hip's rule).  All NaN: class 0, best = NaN.
__device__ __forceinline__ int argmax_first(const float *__restrict__ cs, int nc, float &best)
{
    best = cs[0];
    int arg = 0;
    for (int c = 1; c < nc; c++) {
        const float v = cs[c];
        if (v > best || (best != best && v == v)) best = v, arg = c;
    }
    return arg;
}

// One workgroup per scene: its first row = (kept boxes of the scenes before it) x rows per box, then the scores and the rows.
__global__ __launch_bounds__(256) void det_emit_kernel(int b, int n, int nc, const float *__restrict__ obj,
                                                       const float *__restrict__ class_scores, int per_class,
                                                       const int *__restrict__ kept, const int *__restrict__ count,
                                                       uint4 *__restrict__ rows, int *__restrict__ det_offset)
{
    __shared__ float s_pobj[DET_MAX_N], s_max[DET_MAX_N], s_sum[DET_MAX_N];
    __shared__ int s_cls[DET_MAX_N], s_box[DET_MAX_N];
    __shared__ int s_before;
    const int scene = blockIdx.x, tid = threadIdx.x;
    const int R = per_class ? nc : 1;
    if (tid == 0) s_before = 0;
    __syncthreads();
    int part = 0;
    for (int s = tid; s < scene; s += 256) part += count[s];
    if (part) atomicAdd(&s_before, part); // an integer sum: the order does not matter
    __syncthreads();
    const int K = count[scene];
    const int off = s_before * R;
    if (tid == 0) {
        det_offset[scene] = off;
        if (scene == b - 1) det_offset[b] = off + K * R;
    }
    for (int k = tid; k < K; k += 256) {
        const int box = kept[(size_t)scene * n + k];
        const float *__restrict__ o = obj + ((size_t)scene * n + box) * 2;
        const float d = o[1] - o[0];
        const float *__restrict__ cs = class_scores + ((size_t)scene * n + box) * nc;
        float best;
        s_cls[k] = argmax_first(cs, nc, best);
        float sum = 0.0f;
        if (per_class)
            for (int c = 0; c < nc; c++) sum += expf(cs[c] - best);
        s_box[k] = box;
        s_pobj[k] = 1.0f / (1.0f + expf(-d));
        s_max[k] = best;
        s_sum[k] = sum;
    }
    __syncthreads();
    const int total = K * R;
    for (int r = tid; r < total; r += 256) {
        const int k = r / R, c = r - k * R;
        int cls = s_cls[k];
        float score = s_pobj[k];
        if (per_class) {
            cls = c;
            score = score * (expf(class_scores[((size_t)scene * n + s_box[k]) * nc + c] - s_max[k]) / s_sum[k]);
        }
        rows[(size_t)off + r] = make_uint4((unsigned)scene, (unsigned)s_box[k], (unsigned)cls, __float_as_uint(score));
    }
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

} // namespace votenet
