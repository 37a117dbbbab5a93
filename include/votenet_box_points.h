/*
 * votenet_box_points.h -- C ABI of libvotenet_boxpts.so: the points of the input cloud inside every predicted box of a VoteNet on the
 * MI355X (gfx950), and the gate that takes a box with too few of them out of the NMS -- the `remove_empty_box` step of the VoteNet
 * paper's parse_predictions -- beside libvotenet_hip.so (votenet_hip.h) and libvotenet_detect.so (votenet_detections.h).  A library of
 * its own, as libvotenet_monitors.so, libvotenet_guard.so, libvotenet_features.so and libvotenet_detect.so are: the other libraries
 * export what they did, and a prediction that does not ask for the step never loads this one.  Beyond the reference, which counts the
 * points of labelled ground-truth boxes only (dataset.py:237-283, sunutils.py:199-209; votenet_select_boxes).  Conventions as in
 * votenet_hip.h: extern "C", an explicit stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid
 * argument, 2 = HIP error; text via votenet_box_points_last_error()), the caller owns every buffer, no launcher allocates or
 * synchronises, nothing is read back: both entries can be captured in a graph.
 */
#ifndef VOTENET_BOX_POINTS_H
#define VOTENET_BOX_POINTS_H

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_box_points_last_error(void);

/* counts[s][i] = the number of points of scene s inside box i of scene s.
 *   bboxes (b, n, 8, 3) f32 as votenet_decode_boxes writes them (corner 0 = (+l/2, +h/2, +w/2) rotated about y, corner 1 = corner 0
 *   moved by -w, corner 3 by -l, corner 4 by -h); points (b, npts, 3) f32, contiguous; counts (b, n) int32, written in full.
 *   0 <= b <= 65535, 1 <= n <= 1024, 0 <= npts < 2^24.  npts = 0 writes zeros; b = 0 launches nothing.
 * The rule, in fp32, un-fused, in this order:
 *   c0 = corner 0;  e_0 = corner 1 - c0 (width axis), e_1 = corner 3 - c0 (length axis), e_2 = corner 4 - c0 (height axis);
 *   q = p - c0;  t_k = (q.x e_k.x + q.y e_k.y) + q.z e_k.z;  ee_k = (e_k.x e_k.x + e_k.y e_k.y) + e_k.z e_k.z;
 *   inside  iff  t_k >= 0 && t_k <= ee_k for k = 0, 1, 2.
 * The closed box: a point on a face, an edge or a corner counts, as it does for the hull test of sunutils.py:199-209.  A NaN fails
 * every comparison: a hole point (NaN or infinite coordinates) and a box with a NaN in a corner that is read count nothing, without a
 * special case (an infinite corner has none either: the arithmetic above decides).  Corners 2, 5, 6 and 7 are not read.  The counts
 * are integers: exact, and the same however they are summed -- two calls write the same bytes.
 * Launches on `stream`: a memset of counts, then (npts > 0) one kernel over point tiles x scenes; integer atomic adds only. */
int votenet_box_point_counts(int b, int n, long npts, const float *bboxes, const float *points, int *counts, void *stream);

/* gated[s][i][:] = objectness[s][i][:], bit for bit, where counts[s][i] >= min_points; elsewhere both logits are a quiet NaN
 * (0x7fc00000).  A box with NaN logits is no candidate of votenet_class_nms3d (its margin o1 - o0 is NaN) nor of votenet_nms3d (o1 > o0
 * is false): handing `gated` to either in objectness' place removes the boxes below min_points BEFORE the suppression, the paper's
 * order, and neither NMS changes.  objectness, gated (b, n, 2) f32; counts (b, n) int32; 0 <= b <= 65535, 1 <= n <= 1024;
 * min_points >= 0 (0: an exact copy).  gated may not overlap objectness; both 8-byte aligned.  One elementwise launch. */
int votenet_gate_objectness(int b, int n, const int *counts, int min_points, const float *objectness, float *gated, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_BOX_POINTS_H */
