// eval_match.hip -- one batch's share of the detection evaluation (evaluator.py:76-161,224-226), on the device.
//
// The reference collects the detections of every validation scene on the host, computes the overlap of each with the ground
// truth of its class and scene by a shapely polygon loop, sorts a class's detections by confidence over the whole set and
// walks them once, marking a ground-truth box as taken by the first detection that claims it.  Only the LAST step -- the
// sort over the whole set and the cumulative sums behind the precision / recall curve -- needs more than one scene.  Whether
// a detection is a true positive is decided inside its scene:
//
//     d is a true positive at threshold t  <=>  ovmax_d > t  and no detection e of the same scene and class with
//                                               jmax_e == jmax_d and ovmax_e > t comes before d in the visit order.
//
// (=>: a true positive found its box untaken, so no earlier detection had taken it, and every earlier e with jmax_e == jmax_d
// and ovmax_e > t either takes the box or finds it taken.  <=: the first detection in the order that claims a box finds it
// untaken; only true positives ever set a taken flag, evaluator.py:142-147.)  So one launch per batch turns every kept row into
// a 16-byte record that already holds its true-positive bit for each threshold, and the host sorts records once at the end.
//
// eval_match_kernel, one workgroup per scene:
//   (a) the scene's kept rows, compacted in row order into LDS (the caller's rows need not be sorted or grouped);
//   (b) the scene's valid ground-truth boxes bucketed by class; npos[class] += the bucket sizes;
//   (c) per detection: class = first arg-max of its class scores, score = that maximum;
//   (d) the (detection, ground truth of its class) pairs spread over the lanes -- the polygon clip of iou3d.h is long and
//       divergent -- each folding its overlap into the detection's (ovmax, jmax) by ONE 64-bit integer LDS atomic max on
//       (ordered overlap bits, ~j): the largest overlap wins, among equal overlaps the smallest j, which is the first maximum
//       of the reference's strict '>' scan.  A NaN overlap marks the detection (false positive at every threshold, as
//       `ov.max() > ovthresh` decides);
//   (e) per detection: the bit mask {t : ovmax > thr[t]};
//   (f) per detection: a scan over the scene's records in LDS for an earlier claimant of the same box, then one 16-byte store.
// Visit order inside a scene: score descending, then row index ascending.  Integer atomics and vector stores only: the records
// of a launch do not depend on scheduling (their position in the buffer does; the host sorts by (score, arrival)).
// A pair of (d), (e) and (f) are eval_match_steps.h's, the text votenet_eval_match_rows (detect/detections.hip) compiles too; the
// compaction of (a) is block_compact.h's.
#include "common.h"
#include "block_compact.h"
#include "eval_match_steps.h"

namespace votenet {

__global__ __launch_bounds__(256) void eval_match_kernel(int n, int g, int nc, const float *__restrict__ bboxes,
                                                         const int *__restrict__ rows, int nrows,
                                                         const int *__restrict__ nrows_dev,
                                                         const float *__restrict__ class_scores,
                                                         const float *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                         const int *__restrict__ gt_count, EvalThr thr, int nthr, int scene0,
                                                         unsigned arrival0, uint4 *__restrict__ records, int capacity,
                                                         int *__restrict__ rec_count, int *__restrict__ npos,
                                                         int *__restrict__ flags)
{
    __shared__ int s_box[EVAL_MAX_DET];                // box of the scene's d-th kept row
    __shared__ unsigned s_row[EVAL_MAX_DET];           // ... and its row index in the call
    __shared__ float s_score[EVAL_MAX_DET];            // max class score (NaN -> -inf: a total order)
    __shared__ int s_cls[EVAL_MAX_DET];                // first arg-max
    __shared__ unsigned long long s_key[EVAL_MAX_DET]; // (ordered ovmax, ~jmax); 0 = no overlap seen
    __shared__ int s_nan[EVAL_MAX_DET];
    __shared__ int s_jmax[EVAL_MAX_DET];
    __shared__ int s_qmask[EVAL_MAX_DET];              // {t : ovmax > thr[t]}
    __shared__ int s_poff[EVAL_MAX_DET + 1];           // first pair of detection d
    __shared__ int s_gtlist[EVAL_MAX_GT];              // valid ground-truth rows, bucketed by class
    __shared__ int s_ccnt[EVAL_MAX_NC], s_cfill[EVAL_MAX_NC], s_cstart[EVAL_MAX_NC + 1];
    __shared__ int s_wcnt[4], s_len, s_base;
    const int scene = blockIdx.x, nscene = gridDim.x, tid = threadIdx.x;
    int R = nrows;
    if (nrows_dev) { // the length NMS left on the device, never beyond the rows the caller says the buffer holds
        const int c = *nrows_dev;
        R = c < 0 ? 0 : (c < R ? c : R);
    }
    if (tid == 0) s_len = 0;
    for (int c = tid; c < EVAL_MAX_NC; c += 256) s_ccnt[c] = 0, s_cfill[c] = 0;
    __syncthreads();
    // (a) this scene's kept rows, in row order
    int flag = 0;
    for (int start = 0; start < R; start += 256) {
        const int p = start + tid;
        bool mine = false;
        int box = 0;
        if (p < R) {
            const int sc = rows[p * 2], bx = rows[p * 2 + 1];
            if (sc < 0 || sc >= nscene || bx < 0 || bx >= n)
                flag |= EVAL_F_BAD_ROW;
            else if (sc == scene)
                mine = true, box = bx;
        }
        const int q = block_compact<4>(mine, s_wcnt, &s_len);
        if (mine && q < EVAL_MAX_DET) s_box[q] = box, s_row[q] = (unsigned)p;
    }
    __syncthreads(); // the last round's slots
    int L = s_len;
    if (L > EVAL_MAX_DET) {
        L = EVAL_MAX_DET;
        flag |= EVAL_F_SCENE;
    }
    if (flag) atomicOr(flags, flag);
    // (b) ground truth: rows beyond count are padding; labels outside [0, nc) belong to no class the evaluation visits
    int ngt = g > 0 ? gt_count[scene] : 0;
    ngt = ngt < 0 ? 0 : (ngt > g ? g : ngt);
    for (int j = tid; j < ngt; j += 256) {
        const int c = gt_labels[(size_t)scene * g + j];
        if (c >= 0 && c < nc) atomicAdd(&s_ccnt[c], 1);
    }
    // (c) class and score of every kept row (evaluator.py:224-226)
    for (int d = tid; d < L; d += 256) {
        const float *__restrict__ cs = class_scores + ((size_t)scene * n + s_box[d]) * nc;
        float best = cs[0];
        int arg = 0;
        for (int c = 1; c < nc; c++) {
            const float v = cs[c];
            if (v > best || (best != best && v == v)) best = v, arg = c; // first maximum; a NaN never wins over a number
        }
        s_score[d] = best != best ? -__builtin_inff() : best;
        s_cls[d] = arg;
        s_key[d] = 0ull;
        s_nan[d] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int c = 0; c < nc; c++) {
            s_cstart[c] = acc;
            acc += s_ccnt[c];
        }
        s_cstart[nc] = acc;
        acc = 0;
        for (int d = 0; d < L; d++) {
            s_poff[d] = acc;
            acc += s_ccnt[s_cls[d]];
        }
        s_poff[L] = acc;
        s_base = atomicAdd(rec_count, L); // every record offered is counted, also the ones a full buffer drops
    }
    if (tid < nc && s_ccnt[tid]) atomicAdd(&npos[tid], s_ccnt[tid]);
    __syncthreads();
    for (int j = tid; j < ngt; j += 256) {
        const int c = gt_labels[(size_t)scene * g + j];
        if (c >= 0 && c < nc) s_gtlist[s_cstart[c] + atomicAdd(&s_cfill[c], 1)] = j; // any order: the key carries j
    }
    __syncthreads();
    // (d) one overlap per (detection, ground truth of its class and scene)
    const int npair = s_poff[L];
    for (int p = tid; p < npair; p += 256) {
        int lo = 0, hi = L; // the d with poff[d] <= p < poff[d + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_poff[mid] <= p) lo = mid;
            else hi = mid;
        }
        const int d = lo;
        const int j = s_gtlist[s_cstart[s_cls[d]] + (p - s_poff[d])];
        eval_fold_pair(bboxes + ((size_t)scene * n + s_box[d]) * 24, gt_boxes + ((size_t)scene * g + j) * 24, d, j, s_key, s_nan);
    }
    __syncthreads();
    // (e) ovmax, jmax and the thresholds they pass
    eval_pass_masks(L, s_key, s_nan, thr, nthr, s_jmax, s_qmask);
    __syncthreads();
    // (f) the box is taken at threshold t iff an earlier detection with the same jmax passes t
    eval_write_records(L, s_base, s_score, s_jmax, s_qmask, s_row, [&](int d) { return s_cls[d]; }, (unsigned)(scene0 + scene), arrival0,
                       records, capacity, flags);
}

} // namespace votenet

using namespace votenet;

extern "C" int votenet_eval_match(int b, int n, int g, int nc, const float *bboxes, const int *rows, int nrows,
                                  const int *nrows_dev, const float *class_scores, const float *gt_boxes, const int *gt_labels,
                                  const int *gt_count, int nthr, const float *thresholds, long scene0, unsigned arrival0,
                                  void *records, int capacity, int *rec_count, int *npos, int *flags, void *stream)
{
    VN_REQUIRE(n >= 1, "eval_match expects (batch, n, 8, 3) predicted boxes with n >= 1, got n = %d", n);
    if (int rc = eval_match_check(error_text(), "eval_match", b, g, nc, nthr, thresholds, nrows, capacity, scene0, arrival0, records, rec_count,
                                  npos, flags, gt_boxes, gt_labels, gt_count))
        return rc;
    if (b == 0) return VOTENET_OK;
    VN_REQUIRE(bboxes && class_scores, "eval_match: null prediction buffer");
    VN_REQUIRE(nrows == 0 || rows, "eval_match: null kept rows");
    EvalThr thr = {};
    for (int t = 0; t < nthr; t++) thr.t[t] = thresholds[t];
    hipLaunchKernelGGL(eval_match_kernel, dim3(b), dim3(256), 0, as_stream(stream), n, g, nc, bboxes, rows, nrows, nrows_dev,
                       class_scores, gt_boxes, gt_labels, gt_count, thr, nthr, (int)scene0, arrival0, (uint4 *)records, capacity,
                       rec_count, npos, flags);
    return check_launch("eval_match");
}
