/*
 * votenet_instance_boxes.h -- C ABI of libvotenet_instbox.so: ground-truth boxes from instance-labelled points for a VoteNet on the
 * MI355X (gfx950) -- the axis-aligned extent of every labelled instance in the cloud the network sees, as the VoteNet paper's second
 * benchmark forms its boxes -- beside libvotenet_hip.so (votenet_hip.h).  A library of its own, as libvotenet_boxpts.so and the other
 * side libraries are: the other libraries export what they did, and a run that does not ask for the step never loads this one.  Beyond
 * the reference, whose boxes are annotated (dataset.py:237-283; votenet_select_boxes).  Conventions as in votenet_hip.h: extern "C", an
 * explicit stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error; text via
 * votenet_instance_boxes_last_error()), the caller owns every buffer, no launcher allocates or synchronises, nothing is read back:
 * both entries can be captured in a graph.
 *
 * VOTENET_INSTANCE_BOXES_TILE: the points of a scene one workgroup of the tile pass folds.
 */
#ifndef VOTENET_INSTANCE_BOXES_H
#define VOTENET_INSTANCE_BOXES_H

#include <stddef.h>

#define VOTENET_INSTANCE_BOXES_TILE 2048

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_instance_boxes_last_error(void);

/* Bytes of workspace votenet_instance_boxes needs for b scenes and an id table of k entries; positive, non-decreasing in b and in k.
 * 0 when b is outside [1, 65535] or k outside [1, 1024]. */
size_t votenet_instance_boxes_workspace_bytes(int b, int k);

/* One box per labelled instance of every scene.
 *   points (b, n, 3) f32, contiguous: the cloud the network sees;  instance (b, n), semantic (b, n) int32;  class_map (n_sem) int32.
 *   1 <= b <= 65535, 1 <= n < 2^24, 1 <= k <= 1024, 1 <= n_sem <= 65536, min_points >= 1: anything else returns 1 before any HIP call
 *   (and before any buffer is looked at).  n_class is the number of object classes of the network: any int.
 * The rule, per scene s:
 *   A point takes part iff  0 <= instance < k  and its three coordinates are finite.  Every other point is ignored and counted once in
 *   ignored[s][0 .. 2], by the first of these tests that holds, in this order:
 *     [0] unlabelled      instance < 0   (whatever its coordinates: a non-finite point with a negative id counts here)
 *     [1] out of table    instance >= k  (whatever its coordinates)
 *     [2] non-finite      a NaN or an infinity among its coordinates
 *   Each coordinate is read as x + 0.0f: -0 takes part as +0.
 *   Over the points of id i that take part:  count[i];  lo[i], hi[i] the component-wise fp32 minimum and maximum;  first[i] the
 *   smallest point index.  All four are exact and independent of the order of combination: every run writes the same bytes.
 *   sem_i = semantic[s][first[i]];  cls_i = class_map[sem_i] if 0 <= sem_i < n_sem, else -1;  a cls_i < 0 or >= n_class is -1.
 *   status[s][i], the first that holds in this order:  3 absent (count = 0);  1 no object class (cls_i = -1);  2 fewer than min_points
 *   points;  else 0 kept.
 *   A kept instance is one row:  center = (double(lo) + double(hi)) * 0.5,  size = double(hi) - double(lo),  heading = 0.0,
 *   cls = cls_i,  instance_id = i,  n_points = count[i].  Rows are compact over the batch: scene order, then ascending id.
 * Outputs:  center, size (b k, 3) f64, heading (b k) f64, cls, instance_id, n_points (b k) int32: rows of capacity, of which the first
 *   sum(kept) are written and no other;  kept (b) int32: the rows of each scene;  slot (b, k) int32: the row of id i within its scene,
 *   or -1;  status, inst_count (b, k) int32 and ignored (b, 3) int32, written in full.
 * workspace: votenet_instance_boxes_workspace_bytes(b, k) bytes, 4-byte aligned; its content at entry does not matter.
 * No label value, INT_MIN and INT_MAX included, indexes anything: an id is compared with k before it is used, first[i] with n before
 * semantic is read, sem_i with n_sem before class_map is read.
 * Launches on `stream`, three in all: a memset of the workspace; the tile pass, one workgroup per (tile of VOTENET_INSTANCE_BOXES_TILE
 * points, scene), which folds its points into a table of k entries in LDS with integer LDS atomics (the floats through the
 * order-preserving map to unsigned) and adds its non-empty entries to the workspace with integer global atomics; the finish, one
 * workgroup per scene, which counts the kept rows of the scenes before its own itself and waits for no other.  No float atomic. */
int votenet_instance_boxes(int b, long n, int k, int n_sem, int n_class, int min_points, const float *points, const int *instance,
                           const int *semantic, const int *class_map, double *center, double *size, double *heading, int *cls,
                           int *instance_id, int *n_points, int *kept, int *slot, int *status, int *inst_count, int *ignored,
                           void *workspace, size_t workspace_bytes, void *stream);

/* point_box[s][p] = slot[s][instance[s][p]] for a point that takes part (above), -1 for every other point; so -1 too for a point of an
 * instance that was not kept.  points, instance as above, slot (b, k) int32 as votenet_instance_boxes wrote it, point_box (b, n) int32,
 * written in full.  The limits on b, n and k as above.  One elementwise launch. */
int votenet_instance_point_box(int b, long n, int k, const float *points, const int *instance, const int *slot, int *point_box,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_INSTANCE_BOXES_H */
