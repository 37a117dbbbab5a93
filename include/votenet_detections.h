/*
 * votenet_detections.h -- C ABI of libvotenet_detect.so: per-class detections of a VoteNet on the MI355X (gfx950) -- the VoteNet
 * paper's evaluation protocol (class-wise 3D NMS ordered by objectness, a confidence threshold, one detection per class and kept
 * box) and its matching against ground truth -- beside libvotenet_hip.so (votenet_hip.h).  A library of its own, as
 * libvotenet_monitors.so, libvotenet_guard.so and libvotenet_features.so are: libvotenet_hip.so is the drop-in for the reference's op
 * libraries and exports exactly its two headers; a run under the reference's protocol never loads this one.  Beyond the reference,
 * whose only protocol is class-agnostic NMS ordered by the largest class logit (model.py:133, evaluator.py:224-231; votenet_nms3d /
 * votenet_eval_match).  Conventions as in votenet_hip.h: extern "C", an explicit stream (hipStream_t as void*; NULL = the null
 * stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error, 3 = workspace; text via votenet_detections_last_error()), the
 * caller owns every buffer, no launcher allocates or synchronises, nothing is read back: both entries can be captured in a graph.
 */
#ifndef VOTENET_DETECTIONS_H
#define VOTENET_DETECTIONS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_detections_last_error(void);

/* Class-wise 3D NMS and the detections it leaves.
 *   bboxes (b, n, 8, 3) f32 as votenet_decode_boxes writes them, objectness (b, n, 2) f32 logits, class_scores (b, n, nc) f32 logits;
 *   1 <= n <= 512, 1 <= nc <= 64, b * n * nc < 2^31; iou_threshold in [0, 1]; class_nms, per_class 0 / 1.
 * Per box, in fp32: d = o1 - o0; cls = the first largest class logit, a NaN never winning over a number (all NaN: class 0).
 *   Candidate      iff d > conf_logit.  conf_logit is T = (float)(log(c) - log1p(-c)) of the confidence threshold c in [0, 1), formed
 *                  by the host in double: c = 0 gives -inf, c = 0.5 gives 0 exactly.  P(object) > c  <=>  d > T in real arithmetic;
 *                  the ABI takes T so that the decision is one fp32 comparison.  A NaN d is never a candidate.  -inf <= T < +inf.
 *   Visit order    inside a scene: d descending, equal d by ascending box index -- the order of P(object), decided on d.
 *   Suppression    walking a scene's candidates in visit order, candidate j is dropped iff an earlier KEPT candidate i has
 *                  (class_nms == 0 or cls_i == cls_j) and iou3d(box_j, box_i) > iou_threshold: strictly, the later box first (the
 *                  value votenet_iou3d_matrix writes at [j][i]: one device text, the same flags), a NaN overlap never suppresses.
 *                  Scenes never interact.
 *   Scores         p_obj = 1 / (1 + expf(-d));  p_c = expf(l_c - m) / sum_k expf(l_k - m), m the largest logit as found for cls,
 *                  the sum in class order; all in fp32.
 *   Rows           16 bytes each, {scene, box, class, score bits}.  per_class == 0: one per kept box, (cls, p_obj).  per_class == 1:
 *                  nc per kept box, (c, p_obj * p_c) for c = 0 .. nc-1.  Ordered by scene ascending, then visit order, then class
 *                  ascending: a fixed layout, no atomic decides a position, two calls write the same bytes.
 *   det_offset     (b + 1) ints: the first row of each scene, the total in det_offset[b].  Rows beyond the total are not written.
 * det_rows: 16-byte aligned, det_capacity >= b * n * (per_class ? nc : 1) rows.
 * Filtering by the confidence threshold BEFORE the NMS keeps the same boxes as the paper's filter after it: a box below the threshold
 * comes later in the visit order than every box above it, so it can only suppress boxes that the filter drops anyway.
 * This entry suppresses by the rotated-box IoU of the rest of the project; the paper's NMS uses the overlap of the boxes' axis-aligned
 * hulls, which is votenet_class_nms_aabb (votenet_aabb_nms.h, libvotenet_aabb.so): this entry rule for rule, that overlap in iou3d's place.
 * Launches on `stream`: one workgroup per scene (order, suppression masks by ballots, one wave's pass over them), then one
 * workgroup per scene for the offsets, scores and rows.  workspace: votenet_class_nms3d_workspace_bytes(b, n, nc) bytes. */
size_t votenet_class_nms3d_workspace_bytes(int b, int n, int nc);
int votenet_class_nms3d(int b, int n, int nc, const float *bboxes, const float *objectness, const float *class_scores,
                        float iou_threshold, float conf_logit, int class_nms, int per_class, void *det_rows, long det_capacity,
                        int *det_offset, void *workspace, size_t workspace_bytes, void *stream);

/* votenet_eval_match (votenet_hip.h) on explicit detection rows: one batch's share of the detection evaluation, every row of
 * det_rows[det_offset[s] .. det_offset[s + 1]) one detection {scene s, box, class, score bits} of scene s.  One workgroup per
 * (scene, class): its detections are the scene's rows of that class -- at most 1024 -- visited by score descending, then row
 * ascending (a NaN score ranks as -inf); npos[class] += the scene's valid ground-truth boxes of the class; the overlaps, the
 * (largest overlap, first ground-truth box that has it) per detection, the threshold mask and the scan for an earlier claimant are
 * votenet_eval_match's.  One 16-byte record {score bits, class | tp_mask << 8, scene0 + s, arrival0 + row} per detection, the same
 * format, flags word (1 = records dropped, the buffer was full; 2 = a bad row; 4 = more than 1024 rows of one scene and class) and
 * capacity rule: rec_count counts every record offered.  A bad row -- its scene is not the s whose range holds it, its box outside
 * [0, n), its class outside [0, nc) -- is skipped, and so is a scene whose offsets are not 0 <= det_offset[s] <= det_offset[s + 1]
 * <= nrows.  1 <= n <= 1024, g <= 4096, 1 <= nc <= 256, 1 <= nthr <= 8 (thresholds: a HOST array), b <= 65535. */
int votenet_eval_match_rows(int b, int n, int g, int nc, const float *bboxes, const void *det_rows, long nrows,
                            const int *det_offset, const float *gt_boxes, const int *gt_labels, const int *gt_count, int nthr,
                            const float *thresholds, long scene0, unsigned arrival0, void *records, int capacity, int *rec_count,
                            int *npos, int *flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_DETECTIONS_H */
