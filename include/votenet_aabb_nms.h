/*
 * votenet_aabb_nms.h -- C ABI of libvotenet_aabb.so: the axis-aligned overlaps of the VoteNet paper's NMS on the MI355X (gfx950) --
 * parse_predictions suppresses by the overlap of each box's axis-aligned hull, in 3D (nms_3d_faster) or on the ground plane
 * (nms_2d_faster), as IoU or as the "old type" measure, intersection over the later box -- and the class-wise NMS of
 * votenet_detections.h with that overlap in the rotated-box IoU's place, beside libvotenet_hip.so (votenet_hip.h) and
 * libvotenet_detect.so (votenet_detections.h).  A library of its own, as libvotenet_monitors.so, libvotenet_guard.so,
 * libvotenet_features.so, libvotenet_detect.so and libvotenet_boxpts.so are: the other libraries export what they did, and a
 * prediction that does not ask for an axis-aligned overlap never loads this one.  Beyond the reference, whose only NMS overlap is the
 * rotated-box IoU (tf_nms3d.cpp; votenet_nms3d).  Conventions as in votenet_detections.h: extern "C", an explicit stream
 * (hipStream_t as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error, 3 = workspace; text via
 * votenet_aabb_last_error()), the caller owns every buffer, no launcher allocates or synchronises, nothing is read back: every
 * entry can be captured in a graph.  No atomic decides an output position: two calls write the same bytes.
 *
 * The box rule, in fp32, un-fused, in this order.  Of a box (8, 3) as votenet_decode_boxes writes it, with c_t the coordinate k
 * (k = x, y, z) of corner t:
 *   lo_k = c_0;  for t = 1 .. 7:  lo_k = (c_t < lo_k || c_t != c_t) ? c_t : lo_k
 *   hi_k = c_0;  for t = 1 .. 7:  hi_k = (c_t > hi_k || c_t != c_t) ? c_t : hi_k
 *   e_k  = hi_k - lo_k
 *   v    = (e_x e_y) e_z   mode VOTENET_AABB_3D
 *   v    = e_x e_z         mode VOTENET_AABB_BEV: y is the up axis, the bird's-eye rectangle is (x, z); the y coordinates take no part
 * A NaN is sticky: once lo_k or hi_k is a NaN no later corner replaces it, so a box with a NaN among its eight coordinates k has
 * NaN lo_k, hi_k and e_k.
 *
 * The overlap rule, of a later box j against an earlier box i, for each k the mode reads:
 *   t_k   = (hi_k^j < hi_k^i ? hi_k^j : hi_k^i) - (lo_k^j < lo_k^i ? lo_k^i : lo_k^j)
 *   i_k   = t_k > 0 ? t_k : 0
 *   inter = (i_x i_y) i_z   or   i_x i_z: the product form of v
 *   VOTENET_AABB_IOU          overlap = inter / ((v_j + v_i) - inter)
 *   VOTENET_AABB_OVER_LATER   overlap = inter / v_j                      (the paper's use_old_type_nms)
 * Box j is suppressed iff overlap > threshold, strictly.  There is no special case: what the formulas give is the definition.  A NaN
 * t_k gives i_k = 0.  Under IOU a box with a NaN in a coordinate its mode reads has a NaN v, so its whole row and its whole column
 * are NaN; under OVER_LATER its row is NaN and its column is 0 or NaN.  Two boxes without volume give 0 / 0 under IOU, a later box
 * without volume 0 / 0 under OVER_LATER.  A NaN overlap is not > threshold: such a pair never suppresses.
 */
#ifndef VOTENET_AABB_NMS_H
#define VOTENET_AABB_NMS_H

#include <stddef.h>

#define VOTENET_AABB_3D 0
#define VOTENET_AABB_BEV 1
#define VOTENET_AABB_IOU 0
#define VOTENET_AABB_OVER_LATER 1

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_aabb_last_error(void);

/* out[s][j][i] = the overlap of box j of scene s, as the later box, against box i of scene s, as the earlier one: the table the NMS
 * below decides on (one device function, the same flags), for every pair, the diagonal included.
 *   bboxes (b, n, 8, 3) f32, out (b, n, n) f32, written in full; 0 <= b <= 65535, 0 <= n <= 32768; mode, measure as above.
 * One launch: a workgroup per (64 later boxes, scene); b = 0 or n = 0 launches nothing. */
int votenet_aabb_overlap_matrix(int b, int n, const float *bboxes, int mode, int measure, float *out, void *stream);

/* votenet_class_nms3d (votenet_detections.h) with the overlap above in iou3d's place: candidate j is dropped iff an earlier KEPT
 * candidate i has (class_nms == 0 or cls_i == cls_j) and overlap(box_j, box_i) > iou_threshold.  Everything else is that entry's,
 * rule for rule: the candidates (d = o1 - o0 > conf_logit), the visit order (d descending, equal d by ascending box index), the
 * class (the first largest logit, a NaN never winning), the scores, the 16-byte rows {scene, box, class, score bits} in scene, visit
 * and class order, det_offset (b + 1 ints, rows beyond det_offset[b] are not written), the limits 1 <= n <= 512, 1 <= nc <= 64,
 * b * n * nc < 2^31, b <= 65535, iou_threshold in [0, 1], -inf <= conf_logit < +inf, class_nms and per_class 0 / 1, det_rows 16-byte
 * aligned with det_capacity >= b * n * (per_class ? nc : 1) rows.  votenet_eval_match_rows consumes the rows unchanged.
 * Launches on `stream`: one workgroup of 512 threads per scene -- every candidate's lo, hi and v go to LDS once, in visit order;
 * the suppression masks are ballots over them, a wave per row; one wave's pass over the rows -- then the launch of
 * votenet_class_nms3d for the offsets, scores and rows (one text).  workspace: votenet_class_nms_aabb_workspace_bytes(b, n, nc). */
size_t votenet_class_nms_aabb_workspace_bytes(int b, int n, int nc);
int votenet_class_nms_aabb(int b, int n, int nc, const float *bboxes, const float *objectness, const float *class_scores,
                           float iou_threshold, float conf_logit, int class_nms, int per_class, int mode, int measure, void *det_rows,
                           long det_capacity, int *det_offset, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_AABB_NMS_H */
