// detections.hip -- libvotenet_detect.so (include/votenet_detections.h), a library of its own beside libvotenet_hip.so (whose export
// list is the drop-in ABI of the reference's ops and stays what it was): the VoteNet paper's detection protocol on the device.
//   votenet_class_nms3d       class-wise greedy NMS ordered by objectness, a confidence threshold, one detection per class and kept
//                             box, scored P(object) * P(class).  class_nms_kernel (one workgroup per scene), det_emit_kernel.
//   votenet_eval_match_rows   votenet_eval_match (../eval_match.hip) on those rows: one workgroup per (scene, class); the match
//                             itself is ../eval_match_steps.h, the text eval_match.hip compiles.
// The overlaps are iou3d_pair of ../iou3d.h, the one text nms3d.hip and eval_match.hip compile, under the same flags: a decision here
// is the decision votenet_iou3d_matrix / votenet_iou3d_cross would tabulate.
#include "../block_compact.h"
#include "../eval_match_steps.h"
#include "det_emit.h"

#pragma GCC visibility push(default)
#include "../../../include/votenet_detections.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_detections_last_error()) ----
static thread_local ErrorText g_det_err;
#define DET_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_det_err, cond, __VA_ARGS__)

// ---- votenet_class_nms3d (the limits, argmax_first and det_emit_kernel: det_emit.h) ----
// One workgroup per scene, thread t owns box t.
//   (a) d = o1 - o0, cls, candidate = d > conf_logit;
//   (b) visit order: rank by counting over the scene's d in LDS (d descending, equal d by box index): every candidate its own rank;
//   (c) suppression rows as nms_greedy_mask_kernel builds them -- bit j of row i = candidate j comes later, (has i's class,) and
//       iou3d_pair(box_j, box_i) > thr -- a wave per row, a lane per later candidate, the word is the ballot of the comparisons.  The
//       polygon clip runs for the pairs the class rule leaves, inside the ballot: no table;
//   (d) wave 0 passes over the rows once: a candidate is kept iff no kept candidate has removed it.  The kept boxes go to
//       kept[scene * n ..] in visit order, their number to count[scene].
__global__ __launch_bounds__(DET_NMS_THREADS) void class_nms_kernel(int n, int nc, const float *__restrict__ bboxes,
                                                                    const float *__restrict__ obj,
                                                                    const float *__restrict__ class_scores, float thr,
                                                                    float conf_logit, int class_nms, int *__restrict__ kept,
                                                                    int *__restrict__ count)
{
    __shared__ unsigned long long s_mask[DET_MAX_N * DET_MAX_W]; // L rows x W words
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
        atomicAdd(&s_len, 1);
    }
    __syncthreads();
    const int L = s_len, W = (L + 63) / 64;
    const float *__restrict__ base = bboxes + (size_t)scene * n * 24;
    for (int i = w; i < L; i += DET_NMS_THREADS / 64) {
        const int ci = s_lcls[i];
        const float *__restrict__ pe = base + (size_t)s_list[i] * 24;
        const int w0 = i >> 6; // the words before it hold earlier candidates only
        if (lane < w0) s_mask[(size_t)i * W + lane] = 0ull;
        for (int wd = w0; wd < W; wd++) {
            const int j = wd * 64 + lane;
            const bool need = j > i && j < L && (!class_nms || s_lcls[j] == ci);
            bool hit = false;
            if (need) {
                const float *__restrict__ pl = base + (size_t)s_list[j] * 24;
                float bl[24], be[24];
#pragma unroll
                for (int t = 0; t < 24; t++) {
                    bl[t] = pl[t];
                    be[t] = pe[t];
                }
                hit = iou3d_pair(bl, be) > thr; // the later box first (nms3d.hip:130-134); strict; a NaN overlap is no hit
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

// ---- votenet_eval_match_rows: votenet_eval_match (../eval_match.hip) for one (scene, class); its steps (d)-(f) are
// ../eval_match_steps.h's ----
__global__ __launch_bounds__(256) void eval_match_rows_kernel(int n, int g, int nc, const float *__restrict__ bboxes,
                                                              const int4 *__restrict__ rows, long nrows,
                                                              const int *__restrict__ det_offset,
                                                              const float *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                              const int *__restrict__ gt_count, EvalThr thr, int nthr, int scene0,
                                                              unsigned arrival0, uint4 *__restrict__ records, int capacity,
                                                              int *__restrict__ rec_count, int *__restrict__ npos,
                                                              int *__restrict__ flags)
{
    __shared__ int s_box[EVAL_MAX_DET];                // box of the d-th row of this scene and class
    __shared__ unsigned s_row[EVAL_MAX_DET];           // ... and its row index in the call
    __shared__ float s_score[EVAL_MAX_DET];            // its score (NaN -> -inf: a total order)
    __shared__ unsigned long long s_key[EVAL_MAX_DET]; // (ordered ovmax, ~jmax); 0 = no overlap seen
    __shared__ int s_nan[EVAL_MAX_DET];
    __shared__ int s_jmax[EVAL_MAX_DET];
    __shared__ int s_qmask[EVAL_MAX_DET]; // {t : ovmax > thr[t]}
    __shared__ int s_gtlist[EVAL_MAX_GT]; // the scene's valid ground-truth rows of this class
    __shared__ int s_wcnt[4], s_len, s_ngc, s_base;
    const int cls = blockIdx.x, scene = blockIdx.y, tid = threadIdx.x;
    int flag = 0;
    long lo = det_offset[scene], hi = det_offset[scene + 1];
    if (lo < 0 || hi < lo || hi > nrows) { // offsets that do not ascend inside the buffer: the scene is skipped
        flag |= EVAL_F_BAD_ROW;
        lo = hi = 0;
    }
    if (tid == 0) s_len = 0, s_ngc = 0;
    __syncthreads();
    // (a) this scene's rows of this class, in row order
    for (long start = lo; start < hi; start += 256) {
        const long p = start + tid;
        bool mine = false;
        int box = 0;
        float score = 0.0f;
        if (p < hi) {
            const int4 r = rows[p];
            if (r.x != scene || r.y < 0 || r.y >= n || r.z < 0 || r.z >= nc)
                flag |= EVAL_F_BAD_ROW;
            else if (r.z == cls)
                mine = true, box = r.y, score = __int_as_float(r.w);
        }
        const int q = block_compact<4>(mine, s_wcnt, &s_len);
        if (mine && q < EVAL_MAX_DET) {
            s_box[q] = box, s_row[q] = (unsigned)p;
            s_score[q] = score != score ? -__builtin_inff() : score;
            s_key[q] = 0ull;
            s_nan[q] = 0;
        }
    }
    int L = s_len; // (the slots are read after (b)'s barrier)
    if (L > EVAL_MAX_DET) {
        L = EVAL_MAX_DET;
        flag |= EVAL_F_SCENE;
    }
    if (flag) atomicOr(flags, flag);
    // (b) ground truth of this class: rows beyond count are padding.  Any order: the key carries j
    int ngt = g > 0 ? gt_count[scene] : 0;
    ngt = ngt < 0 ? 0 : (ngt > g ? g : ngt);
    for (int j = tid; j < ngt; j += 256)
        if (gt_labels[(size_t)scene * g + j] == cls) s_gtlist[atomicAdd(&s_ngc, 1)] = j;
    __syncthreads();
    const int ngc = s_ngc;
    if (tid == 0) {
        if (ngc) atomicAdd(&npos[cls], ngc);
        s_base = L ? atomicAdd(rec_count, L) : 0; // every record offered is counted, also the ones a full buffer drops
    }
    // (d) one overlap per (detection, ground truth of its class and scene)
    const int npair = L * ngc;
    for (int p = tid; p < npair; p += 256) {
        const int d = p / ngc;
        const int j = s_gtlist[p - d * ngc];
        eval_fold_pair(bboxes + ((size_t)scene * n + s_box[d]) * 24, gt_boxes + ((size_t)scene * g + j) * 24, d, j, s_key, s_nan);
    }
    __syncthreads();
    // (e) ovmax, jmax and the thresholds they pass
    eval_pass_masks(L, s_key, s_nan, thr, nthr, s_jmax, s_qmask);
    __syncthreads();
    // (f) the box is taken at threshold t iff an earlier detection with the same jmax passes t
    eval_write_records(L, s_base, s_score, s_jmax, s_qmask, s_row, [cls](int) { return cls; }, (unsigned)(scene0 + scene), arrival0, records,
                       capacity, flags);
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_detections_last_error(void) { return g_det_err.text; }

extern "C" size_t votenet_class_nms3d_workspace_bytes(int b, int n, int nc)
{
    (void)nc;
    return class_nms_workspace_bytes(b, n);
}

extern "C" int votenet_class_nms3d(int b, int n, int nc, const float *bboxes, const float *objectness, const float *class_scores,
                                   float iou_threshold, float conf_logit, int class_nms, int per_class, void *det_rows,
                                   long det_capacity, int *det_offset, void *workspace, size_t workspace_bytes, void *stream)
{
    return class_nms_entry(g_det_err, "class_nms3d", b, n, nc, bboxes, objectness, class_scores, iou_threshold, conf_logit, class_nms,
                           per_class, det_rows, det_capacity, det_offset, workspace, workspace_bytes, stream,
                           [&](hipStream_t st, int *kept, int *count) {
                               hipLaunchKernelGGL(class_nms_kernel, dim3(b), dim3(DET_NMS_THREADS), 0, st, n, nc, bboxes, objectness,
                                                  class_scores, iou_threshold, conf_logit, class_nms, kept, count);
                           });
}

extern "C" int votenet_eval_match_rows(int b, int n, int g, int nc, const float *bboxes, const void *det_rows, long nrows,
                                       const int *det_offset, const float *gt_boxes, const int *gt_labels, const int *gt_count,
                                       int nthr, const float *thresholds, long scene0, unsigned arrival0, void *records,
                                       int capacity, int *rec_count, int *npos, int *flags, void *stream)
{
    DET_REQUIRE(n >= 1 && n <= EVAL_MAX_DET, "eval_match_rows: 1 to %d boxes per scene, got n = %d", EVAL_MAX_DET, n);
    if (int rc = eval_match_check(g_det_err, "eval_match_rows", b, g, nc, nthr, thresholds, nrows, capacity, scene0, arrival0, records,
                                  rec_count, npos, flags, gt_boxes, gt_labels, gt_count))
        return rc;
    if (b == 0) return VOTENET_OK;
    DET_REQUIRE(bboxes && det_offset, "eval_match_rows: null prediction buffer");
    DET_REQUIRE(nrows == 0 || det_rows, "eval_match_rows: null detection rows");
    DET_REQUIRE(((uintptr_t)det_rows & 15) == 0 && ((uintptr_t)records & 15) == 0, "eval_match_rows: det_rows and records must be 16-byte aligned");
    EvalThr thr = {};
    for (int t = 0; t < nthr; t++) thr.t[t] = thresholds[t];
    hipLaunchKernelGGL(eval_match_rows_kernel, dim3(nc, b), dim3(256), 0, as_stream(stream), n, g, nc, bboxes, (const int4 *)det_rows,
                       nrows, det_offset, gt_boxes, gt_labels, gt_count, thr, nthr, (int)scene0, arrival0, (uint4 *)records, capacity,
                       rec_count, npos, flags);
    return g_det_err.check_launch("eval_match_rows");
}
