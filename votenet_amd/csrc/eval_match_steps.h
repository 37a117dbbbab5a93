// eval_match_steps.h -- the part of the evaluation match that does not depend on how a workgroup came by its detections: the limits,
// the record's flag bits, the (overlap, ground-truth row) key and steps (d) to (f) of eval_match.hip's header, with the argument
// checks of the two entries.  One text for the two translation units that compile it, eval_match.hip (libvotenet_hip.so, one
// workgroup per scene) and detect/detections.hip (libvotenet_detect.so, one per scene and class): the tie rule, the NaN rule and
// the record are decided here, once.
#pragma once
#include "common.h"
#include "error_text.h"
#include "iou3d.h"

#include <climits>

namespace votenet {

constexpr int EVAL_MAX_DET = 1024; // detections of one workgroup
constexpr int EVAL_MAX_GT = 4096;  // ground-truth rows of one scene
constexpr int EVAL_MAX_NC = 256;   // the class travels in 8 bits of the record
constexpr int EVAL_MAX_THR = 8;    // one bit each in the record's mask

struct EvalThr {
    float t[EVAL_MAX_THR];
};

// flags word
constexpr int EVAL_F_OVERFLOW = 1; // records dropped: the buffer was full
constexpr int EVAL_F_BAD_ROW = 2;  // a row names a scene, a box or a class outside the batch (skipped)
constexpr int EVAL_F_SCENE = 4;    // more than EVAL_MAX_DET rows for one workgroup (the rest skipped)

// float bits -> unsigned that orders like the float (no NaN reaches this)
__device__ __forceinline__ unsigned ordered_bits(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned o) { return __uint_as_float((o >> 31) ? (o & 0x7fffffffu) : ~o); }

// (d) for one pair: the overlap of detection d (box pb) with ground-truth row j (box pg), folded into s_key[d] / s_nan[d]
__device__ __forceinline__ void eval_fold_pair(const float *__restrict__ pb, const float *__restrict__ pg, int d, int j,
                                               unsigned long long *s_key, int *s_nan)
{
    float bi[24], bj[24];
#pragma unroll
    for (int t = 0; t < 24; t++) {
        bi[t] = pb[t];
        bj[t] = pg[t];
    }
    const float ov = iou3d_pair(bi, bj); // detection first, as votenet_iou3d_cross
    if (ov != ov)
        atomicOr(&s_nan[d], 1);
    else
        atomicMax(&s_key[d], ((unsigned long long)ordered_bits(ov + 0.0f) << 32) | (unsigned)(~j)); // -0 == +0 in a '>' scan
}

// (e) ovmax, jmax and the thresholds they pass.  The caller's barrier follows
__device__ __forceinline__ void eval_pass_masks(int L, const unsigned long long *s_key, const int *s_nan, const EvalThr &thr, int nthr,
                                                int *s_jmax, int *s_qmask)
{
    for (int d = threadIdx.x; d < L; d += 256) {
        const unsigned long long k = s_key[d];
        int q = 0, jm = -1;
        if (k != 0ull && !s_nan[d]) {
            const float ovmax = from_ordered_bits((unsigned)(k >> 32));
            jm = (int)~(unsigned)k;
            for (int t = 0; t < nthr; t++)
                if (ovmax > thr.t[t]) q |= 1 << t;
        }
        s_jmax[d] = jm;
        s_qmask[d] = q;
    }
}

// (f) the box is taken at threshold t iff an earlier detection with the same jmax passes t; then the record.  class_of(d): the
// class of the workgroup's d-th detection
template <class ClassOf>
__device__ __forceinline__ void eval_write_records(int L, int base, const float *s_score, const int *s_jmax, const int *s_qmask,
                                                   const unsigned *s_row, ClassOf class_of, unsigned scene_number, unsigned arrival0,
                                                   uint4 *__restrict__ records, int capacity, int *__restrict__ flags)
{
    for (int d = threadIdx.x; d < L; d += 256) {
        const int jm = s_jmax[d];
        const float sd = s_score[d];
        int taken = 0;
        if (s_qmask[d])
            for (int e = 0; e < L; e++) {
                const float se = s_score[e];
                if (s_jmax[e] == jm && (se > sd || (se == sd && e < d))) taken |= s_qmask[e];
            }
        const int tp = s_qmask[d] & ~taken;
        const long pos = (long)base + d;
        if (pos < (long)capacity)
            records[pos] = make_uint4(__float_as_uint(sd), (unsigned)class_of(d) | ((unsigned)tp << 8), scene_number, arrival0 + s_row[d]);
        else
            atomicOr(flags, EVAL_F_OVERFLOW);
    }
}

// The argument checks votenet_eval_match and votenet_eval_match_rows share (`name` is the entry's, the text goes to the library's
// own `err`); an empty batch needs no ground truth.
inline int eval_match_check(ErrorText &err, const char *name, int b, int g, int nc, int nthr, const float *thresholds, long nrows,
                            int capacity, long scene0, unsigned arrival0, const void *records, const int *rec_count, const int *npos,
                            const int *flags, const float *gt_boxes, const int *gt_labels, const int *gt_count)
{
    VN_REQUIRE_IN(err, b >= 0 && b <= 65535, "%s: batch must be in [0, 65535], got %d", name, b);
    VN_REQUIRE_IN(err, g >= 0 && g <= EVAL_MAX_GT, "%s: at most %d ground-truth rows per scene, got %d", name, EVAL_MAX_GT, g);
    VN_REQUIRE_IN(err, nc >= 1 && nc <= EVAL_MAX_NC, "%s: the number of classes must be in [1, %d], got %d", name, EVAL_MAX_NC, nc);
    VN_REQUIRE_IN(err, nthr >= 1 && nthr <= EVAL_MAX_THR, "%s: 1 to %d IoU thresholds, got %d", name, EVAL_MAX_THR, nthr);
    VN_REQUIRE_IN(err, thresholds != nullptr, "%s: null thresholds", name);
    VN_REQUIRE_IN(err, nrows >= 0 && capacity >= 0, "%s: negative row count or capacity", name);
    VN_REQUIRE_IN(err, scene0 >= 0 && scene0 + b <= (long)INT_MAX, "%s: scene numbers must fit 31 bits, got %ld + %d", name, scene0, b);
    VN_REQUIRE_IN(err, (unsigned long long)arrival0 + (unsigned long long)nrows <= 0xffffffffull, "%s: arrival numbers must fit 32 bits", name);
    VN_REQUIRE_IN(err, records && rec_count && npos && flags, "%s: null accumulator buffer", name);
    VN_REQUIRE_IN(err, b == 0 || g == 0 || (gt_boxes && gt_labels && gt_count), "%s: null ground-truth buffer", name);
    return VOTENET_OK;
}

} // namespace votenet
