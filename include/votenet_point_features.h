/*
 * votenet_point_features.h -- C ABI of libvotenet_features.so: the input step of a VoteNet that takes point features (height above the
 * floor, colour, intensity) on the MI355X (gfx950), beside libvotenet_hip.so (votenet_hip.h).  A library of its own, as
 * libvotenet_monitors.so and libvotenet_guard.so are: libvotenet_hip.so is the drop-in for the reference's op libraries and exports
 * exactly its two headers; a run without point features never loads this one.  Beyond the reference, which drops the colour
 * (dataset.py:310) and feeds the coordinates as features (model.py:36).  Conventions as in votenet_hip.h: extern "C", an explicit
 * stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error; text via
 * votenet_point_features_last_error()), the caller owns every buffer, no launcher allocates or synchronises, nothing is read back.
 */
#ifndef VOTENET_POINT_FEATURES_H
#define VOTENET_POINT_FEATURES_H

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_point_features_last_error(void);

/* Everything votenet_subsample_augment takes, with the same meaning (votenet_hip.h: raw / raw_offset / choice | seed, scene0 / the
 * augmentation draws as HOST arrays), and `out` (b, n_out, 3) bit for bit what that entry writes for the same arguments: one device
 * text serves both libraries (csrc/augment_points.h).  Beside it, c = want_height + extra_cols features per point:
 *   feats (b, n_out, c) = [height | raw columns 3 .. 3+extra_cols of the raw row the point came from]
 * want_height 0 / 1, extra_cols 0..4, 1 <= c <= 5, 3 + extra_cols <= raw_stride.  The raw columns are rounded once to float; the
 * augmentation does not touch them.
 * Height: up = -y of the OUTPUT point (upright camera, y down; after the augmentation, so the scale draw scales heights with the
 * cloud).  Over the m points of scene s whose up is finite: k = 0.0099 (m - 1), lo = floor(k), t = k - lo, a / b = the order
 * statistics of rank lo / min(lo + 1, m - 1) of up -- exact: a radix select over order-preserving 32-bit keys, LDS histograms, one
 * workgroup per scene, both ranks from the same four passes --, floor[s] = (float)(a + (b - a) t) in double: np.percentile(up, 0.99)
 * with linear interpolation.  height = up - floor[s], one float subtraction; 0 where up is not finite; floor 0 for m = 0.
 * floor: (b) floats.  order_stats: NULL, or (b, 2) floats: a and b (tests).  want_height = 0: neither is written (floor may be NULL).
 * Launches on `stream`: gather + transform + columns (one per 16 scenes), then floor + heights (one); no scratch. */
int votenet_subsample_augment_features(int b, int n_out, const void *raw, int raw_f64, int raw_stride, const long *raw_offset,
                                       const int *choice, unsigned long long seed, long scene0, int depth_to_camera,
                                       const int *flip, const double *rot_cos, const double *rot_sin, const double *scale,
                                       int want_height, int extra_cols, float *out, float *feats, float *floor,
                                       float *order_stats, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_POINT_FEATURES_H */
