// det_emit.h -- the part of a class-wise NMS that does not depend on its overlap: the limits, the class of a box, the launch that
// turns a scene's kept boxes into detection rows and the host entry around the two launches.  One text for the two translation
// units that compile it, detections.hip (libvotenet_detect.so, rotated-box IoU) and ../aabb/aabb_nms.hip (libvotenet_aabb.so,
// axis-aligned overlaps), as ../sumsq.h and ../augment_points.h are shared: both libraries refuse the same arguments and write the
// same rows for the same kept boxes.
#pragma once
#include "../common.h"
#include "../error_text.h"

#include <climits>
#include <cstddef>
#include <cstdint>

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

// ---- the host side of votenet_class_nms3d and votenet_class_nms_aabb ----
inline size_t class_nms_workspace_bytes(int b, int n)
{
    if (b <= 0 || n <= 0) return 256;
    return align256((size_t)b * n * sizeof(int)) + align256((size_t)b * sizeof(int)); // kept boxes per scene, their counts
}

// The argument checks (`name` is the entry's, the text goes to the library's own `err`), the empty batch, the workspace's two
// arrays, launch_nms(stream, kept, count) -- the entry's own kernel -- and det_emit_kernel.
template <class LaunchNms>
inline int class_nms_entry(ErrorText &err, const char *name, int b, int n, int nc, const float *bboxes, const float *objectness,
                           const float *class_scores, float iou_threshold, float conf_logit, int class_nms, int per_class,
                           void *det_rows, long det_capacity, int *det_offset, void *workspace, size_t workspace_bytes, void *stream,
                           LaunchNms launch_nms)
{
    VN_REQUIRE_IN(err, b >= 0 && b <= 65535, "%s: batch must be in [0, 65535], got %d", name, b);
    VN_REQUIRE_IN(err, n >= 0 && n <= DET_MAX_N, "%s: at most %d boxes per scene, got n = %d", name, DET_MAX_N, n);
    VN_REQUIRE_IN(err, nc >= 1 && nc <= DET_MAX_NC, "%s: the number of classes must be in [1, %d], got %d", name, DET_MAX_NC, nc);
    VN_REQUIRE_IN(err, iou_threshold >= 0 && iou_threshold <= 1, "%s: iou_threshold must be in [0, 1], got %g", name, (double)iou_threshold);
    VN_REQUIRE_IN(err, conf_logit == conf_logit && conf_logit < __builtin_inff(),
                  "%s: conf_logit must be the logit of a confidence threshold in [0, 1): -inf <= T < +inf, got %g", name, (double)conf_logit);
    VN_REQUIRE_IN(err, (class_nms == 0 || class_nms == 1) && (per_class == 0 || per_class == 1), "%s: class_nms and per_class are 0 or 1", name);
    VN_REQUIRE_IN(err, det_offset != nullptr, "%s: det_offset is required", name);
    const long need = (long)b * n * (per_class ? nc : 1);
    VN_REQUIRE_IN(err, (long)b * n * nc <= (long)INT_MAX, "%s: b * n * nc must fit 31 bits", name);
    VN_REQUIRE_IN(err, det_capacity >= need, "%s: det_rows must hold b * n * %d = %ld rows, got %ld", name, per_class ? nc : 1, need, det_capacity);
    hipStream_t st = as_stream(stream);
    if (b == 0 || n == 0) {
        (void)hipMemsetAsync(det_offset, 0, ((size_t)b + 1) * sizeof(int), st);
        return err.check_launch(name);
    }
    VN_REQUIRE_IN(err, bboxes && objectness && class_scores && det_rows, "%s: null buffer", name);
    VN_REQUIRE_IN(err, ((uintptr_t)det_rows & 15) == 0, "%s: det_rows must be 16-byte aligned", name);
    const size_t wbytes = class_nms_workspace_bytes(b, n);
    if (workspace == nullptr || workspace_bytes < wbytes)
        return err.set(VOTENET_E_WORKSPACE, "%s: workspace of %zu bytes required, got %zu", name, wbytes, workspace ? workspace_bytes : (size_t)0);
    int *kept = (int *)workspace;
    int *count = (int *)((char *)workspace + align256((size_t)b * n * sizeof(int)));
    launch_nms(st, kept, count);
    hipLaunchKernelGGL(det_emit_kernel, dim3(b), dim3(256), 0, st, b, n, nc, objectness, class_scores, per_class, kept, count,
                       (uint4 *)det_rows, det_offset);
    return err.check_launch(name);
}

} // namespace votenet
