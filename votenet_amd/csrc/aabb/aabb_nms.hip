// aabb_nms.hip -- libvotenet_aabb.so (include/votenet_aabb_nms.h), a library of its own beside libvotenet_hip.so and
// libvotenet_detect.so (whose export lists stay what they were): the axis-aligned overlaps of the VoteNet paper's NMS.
//   votenet_aabb_overlap_matrix   every (later, earlier) overlap of a scene's boxes.  aabb_matrix_kernel: a workgroup per
//                                 (64 later boxes, scene).
//   votenet_class_nms_aabb        votenet_class_nms3d (../detect/detections.hip) deciding on those overlaps.  class_nms_aabb_kernel
//                                 (one workgroup per scene), then det_emit_kernel and the host entry of ../detect/det_emit.h:
//                                 the rows and the argument checks of libvotenet_detect.so, from one text.
// Both kernels call aabb_of and aabb_overlap below.  The rules of the header are plain fp32 arithmetic in a fixed order
// (-ffp-contract=off, as everywhere in this project): tests/aabb_nms_ref.py restates them in numpy float32 and the table is compared
// bit for bit.
#include "../detect/det_emit.h"

#pragma GCC visibility push(default)
#include "../../../include/votenet_aabb_nms.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_aabb_last_error()) ----
static thread_local ErrorText g_aabb_err;
#define AABB_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_aabb_err, cond, __VA_ARGS__)

constexpr int AABB_MAX_B = 65535;     // scenes: a grid extent
constexpr int AABB_MAX_MATRIX_N = 32768;
constexpr int AABB_TILE = 64;         // later boxes of one workgroup of the matrix kernel
constexpr int AABB_MATRIX_THREADS = 256;

// ---- the box rule and the overlap rule of the header ----
struct Aabb {
    float lox, loy, loz, hix, hiy, hiz, v;
};

// lo / hi of one coordinate over corners 0..7 in corner order; a NaN is sticky
__device__ __forceinline__ void aabb_extent(const float *__restrict__ c, float &lo, float &hi)
{
    lo = hi = c[0];
#pragma unroll
    for (int t = 1; t < 8; t++) {
        const float ct = c[t * 3];
        lo = (ct < lo || ct != ct) ? ct : lo;
        hi = (ct > hi || ct != ct) ? ct : hi;
    }
}

__device__ __forceinline__ Aabb aabb_of(const float *__restrict__ box, int mode)
{
    Aabb a;
    aabb_extent(box + 0, a.lox, a.hix);
    aabb_extent(box + 1, a.loy, a.hiy);
    aabb_extent(box + 2, a.loz, a.hiz);
    const float ex = a.hix - a.lox, ey = a.hiy - a.loy, ez = a.hiz - a.loz;
    a.v = mode == VOTENET_AABB_BEV ? ex * ez : (ex * ey) * ez;
    return a;
}

__device__ __forceinline__ float aabb_side(float loj, float hij, float loi, float hii)
{
    const float t = (hij < hii ? hij : hii) - (loj < loi ? loi : loj);
    return t > 0.0f ? t : 0.0f;
}

// the later box j first, as iou3d_pair takes its boxes
__device__ __forceinline__ float aabb_overlap(const Aabb &j, const Aabb &i, int mode, int measure)
{
    const float ix = aabb_side(j.lox, j.hix, i.lox, i.hix);
    const float iz = aabb_side(j.loz, j.hiz, i.loz, i.hiz);
    float inter;
    if (mode == VOTENET_AABB_BEV)
        inter = ix * iz;
    else
        inter = (ix * aabb_side(j.loy, j.hiy, i.loy, i.hiy)) * iz;
    return measure == VOTENET_AABB_OVER_LATER ? inter / j.v : inter / ((j.v + i.v) - inter);
}

// ---- votenet_aabb_overlap_matrix ----
// A workgroup per (tile of AABB_TILE later boxes, scene).  The tile's boxes go to LDS once; thread t then owns the earlier boxes
// t, t + 256, ...: it forms one's lo, hi and v in registers and writes out[scene][j][i] for the tile's j -- for a fixed j the
// workgroup's stores are one contiguous run of the row.
__global__ __launch_bounds__(AABB_MATRIX_THREADS) void aabb_matrix_kernel(int n, const float *__restrict__ bboxes, int mode,
                                                                          int measure, float *__restrict__ out)
{
    __shared__ Aabb s_later[AABB_TILE];
    const int scene = blockIdx.y, tid = threadIdx.x;
    const int j0 = blockIdx.x * AABB_TILE;
    const int m = n - j0 < AABB_TILE ? n - j0 : AABB_TILE;
    const float *__restrict__ base = bboxes + (size_t)scene * n * 24;
    if (tid < m) s_later[tid] = aabb_of(base + (size_t)(j0 + tid) * 24, mode);
    __syncthreads();
    float *__restrict__ o = out + ((size_t)scene * n + j0) * n;
    for (int i = tid; i < n; i += AABB_MATRIX_THREADS) {
        const Aabb e = aabb_of(base + (size_t)i * 24, mode);
        for (int jj = 0; jj < m; jj++) o[(size_t)jj * n + i] = aabb_overlap(s_later[jj], e, mode, measure);
    }
}

// ---- votenet_class_nms_aabb ----
// One workgroup per scene, thread t owns box t.  Steps (a), (b) and (d) are class_nms_kernel's (../detect/detections.hip):
//   (a) d = o1 - o0, cls, candidate = d > conf_logit;
//   (b) visit order: rank by counting over the scene's d in LDS (d descending, equal d by box index); every candidate then reads its
//       box -- 96 bytes, once -- and leaves lo, hi and v at its rank, one array per component (a lane per candidate reads
//       consecutive words);
//   (c) suppression rows: bit j of row i = candidate j comes later, (has i's class,) and aabb_overlap(box_j, box_i) > thr -- a wave
//       per row, a lane per later candidate, the word is the ballot of the comparisons; the row's own box is a broadcast read;
//   (d) wave 0 passes over the rows once: a candidate is kept iff no kept candidate has removed it.  The kept boxes go to
//       kept[scene * n ..] in visit order, their number to count[scene].
__global__ __launch_bounds__(DET_NMS_THREADS) void class_nms_aabb_kernel(int n, int nc, const float *__restrict__ bboxes,
                                                                         const float *__restrict__ obj,
                                                                         const float *__restrict__ class_scores, float thr,
                                                                         float conf_logit, int class_nms, int mode, int measure,
                                                                         int *__restrict__ kept, int *__restrict__ count)
{
    __shared__ unsigned long long s_mask[DET_MAX_N * DET_MAX_W]; // L rows x W words
    __shared__ float s_box[7][DET_MAX_N];                        // lo x y z, hi x y z, v of the r-th candidate in visit order
    __shared__ float s_d[DET_MAX_N];
    __shared__ int s_cand[DET_MAX_N];
    __shared__ int s_list[DET_MAX_N]; // box of the r-th candidate in visit order
    __shared__ int s_lcls[DET_MAX_N]; // ... and its class
    __shared__ int s_len;
    const int scene = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_len = 0;
    float d = 0.0f;
    bool cand = false;
    int cls = 0;
    if (tid < n) {
        const float *__restrict__ o = obj + ((size_t)scene * n + tid) * 2;
        d = o[1] - o[0];
        cand = d > conf_logit; // false for a NaN d
        float best;
        cls = argmax_first(class_scores + ((size_t)scene * n + tid) * nc, nc, best);
        s_d[tid] = d;
        s_cand[tid] = cand ? 1 : 0;
    }
    __syncthreads();
    if (cand) {
        int rank = 0;
        for (int e = 0; e < n; e++) {
            const float de = s_d[e];
            if (s_cand[e] && (de > d || (de == d && e < tid))) rank++;
        }
        s_list[rank] = tid;
        s_lcls[rank] = cls;
        const Aabb a = aabb_of(bboxes + ((size_t)scene * n + tid) * 24, mode);
        s_box[0][rank] = a.lox, s_box[1][rank] = a.loy, s_box[2][rank] = a.loz;
        s_box[3][rank] = a.hix, s_box[4][rank] = a.hiy, s_box[5][rank] = a.hiz;
        s_box[6][rank] = a.v;
        atomicAdd(&s_len, 1);
    }
    __syncthreads();
    const int L = s_len, W = (L + 63) / 64;
    for (int i = w; i < L; i += DET_NMS_THREADS / 64) {
        const int ci = s_lcls[i];
        const Aabb be = {s_box[0][i], s_box[1][i], s_box[2][i], s_box[3][i], s_box[4][i], s_box[5][i], s_box[6][i]};
        const int w0 = i >> 6; // the words before it hold earlier candidates only
        if (lane < w0) s_mask[(size_t)i * W + lane] = 0ull;
        for (int wd = w0; wd < W; wd++) {
            const int j = wd * 64 + lane;
            const bool need = j > i && j < L && (!class_nms || s_lcls[j] == ci);
            bool hit = false;
            if (need) {
                const Aabb bl = {s_box[0][j], s_box[1][j], s_box[2][j], s_box[3][j], s_box[4][j], s_box[5][j], s_box[6][j]};
                hit = aabb_overlap(bl, be, mode, measure) > thr; // the later box first; strict; a NaN overlap is no hit
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) s_mask[(size_t)i * W + wd] = m;
        }
    }
    __syncthreads();
    if (w == 0) { // lane wd owns word wd of the removed set
        unsigned long long removed = 0ull;
        int nk = 0;
        for (int i = 0; i < L; i++) {
            const unsigned long long cur = __shfl(removed, i >> 6);
            if (!((cur >> (i & 63)) & 1ull)) { // uniform
                if (lane < W) removed |= s_mask[(size_t)i * W + lane];
                if (lane == 0) kept[(size_t)scene * n + nk] = s_list[i];
                nk++;
            }
        }
        if (lane == 0) count[scene] = nk;
    }
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_aabb_last_error(void) { return g_aabb_err.text; }

extern "C" int votenet_aabb_overlap_matrix(int b, int n, const float *bboxes, int mode, int measure, float *out, void *stream)
{
    AABB_REQUIRE(b >= 0 && b <= AABB_MAX_B, "aabb_overlap_matrix: batch must be in [0, %d], got %d", AABB_MAX_B, b);
    AABB_REQUIRE(n >= 0 && n <= AABB_MAX_MATRIX_N, "aabb_overlap_matrix: at most %d boxes per scene, got n = %d", AABB_MAX_MATRIX_N, n);
    AABB_REQUIRE(mode == VOTENET_AABB_3D || mode == VOTENET_AABB_BEV, "aabb_overlap_matrix: mode must be 0 (3D) or 1 (bird's-eye), got %d", mode);
    AABB_REQUIRE(measure == VOTENET_AABB_IOU || measure == VOTENET_AABB_OVER_LATER,
                 "aabb_overlap_matrix: measure must be 0 (IoU) or 1 (intersection over the later box), got %d", measure);
    if (b == 0 || n == 0) return VOTENET_OK;
    AABB_REQUIRE(bboxes && out, "aabb_overlap_matrix: null buffer");
    hipLaunchKernelGGL(aabb_matrix_kernel, dim3((n + AABB_TILE - 1) / AABB_TILE, b), dim3(AABB_MATRIX_THREADS), 0, as_stream(stream), n,
                       bboxes, mode, measure, out);
    return g_aabb_err.check_launch("aabb_overlap_matrix");
}

extern "C" size_t votenet_class_nms_aabb_workspace_bytes(int b, int n, int nc)
{
    (void)nc;
    return class_nms_workspace_bytes(b, n);
}

extern "C" int votenet_class_nms_aabb(int b, int n, int nc, const float *bboxes, const float *objectness, const float *class_scores,
                                      float iou_threshold, float conf_logit, int class_nms, int per_class, int mode, int measure,
                                      void *det_rows, long det_capacity, int *det_offset, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    AABB_REQUIRE(mode == VOTENET_AABB_3D || mode == VOTENET_AABB_BEV, "class_nms_aabb: mode must be 0 (3D) or 1 (bird's-eye), got %d", mode);
    AABB_REQUIRE(measure == VOTENET_AABB_IOU || measure == VOTENET_AABB_OVER_LATER,
                 "class_nms_aabb: measure must be 0 (IoU) or 1 (intersection over the later box), got %d", measure);
    return class_nms_entry(g_aabb_err, "class_nms_aabb", b, n, nc, bboxes, objectness, class_scores, iou_threshold, conf_logit, class_nms,
                           per_class, det_rows, det_capacity, det_offset, workspace, workspace_bytes, stream,
                           [&](hipStream_t st, int *kept, int *count) {
                               hipLaunchKernelGGL(class_nms_aabb_kernel, dim3(b), dim3(DET_NMS_THREADS), 0, st, n, nc, bboxes, objectness,
                                                  class_scores, iou_threshold, conf_logit, class_nms, mode, measure, kept, count);
                           });
}
