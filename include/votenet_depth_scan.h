/*
 * votenet_depth_scan.h -- C ABI of libvotenet_depth.so: the raw scan of a batch of scenes from their depth images (optionally with
 * colour) on the MI355X (gfx950), beside libvotenet_hip.so (votenet_hip.h).  A library of its own, as libvotenet_features.so and the
 * other side libraries are: libvotenet_hip.so is the drop-in for the reference's op libraries and exports exactly its two headers; a
 * run that starts from scan tables never loads this one.  Beyond the reference, which reads the scan from a text file that an offline
 * pass over the dataset wrote (sunutils.py:178-180, dataset.py:184) and whose own geometry (SUNRGBD_Calibration.
 * project_image_to_camera -> flip_axis_to_depth -> Rtilt, sunutils.py:107-121) never runs on a depth map.  Conventions as in
 * votenet_point_features.h: extern "C", an explicit stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok,
 * 1 = invalid argument, 2 = HIP error; text via votenet_depth_scan_last_error()), the caller owns every buffer, no launcher allocates
 * or synchronises, nothing is read back.
 */
#ifndef VOTENET_DEPTH_SCAN_H
#define VOTENET_DEPTH_SCAN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_depth_scan_last_error(void);

/* Bytes of device scratch votenet_depth_scan needs for b scenes of total_pixels pixels together (an upper bound that holds however
 * the pixels are spread over the scenes; monotone in both arguments). */
size_t votenet_depth_scan_workspace_bytes(int b, long total_pixels);

/* b scenes, 1 <= b <= 32 (their calibrations travel as kernel arguments).  Scene s is h_s x w_s pixels, hw[2 s] = h_s, hw[2 s + 1] =
 * w_s, row-major, at depth[pix_offset[s] .. pix_offset[s + 1]) (device, 16-bit unsigned; any 2-byte aligned address) and, with
 * colour, rgb[3 pix_offset[s] ..) (device, 8-bit unsigned, three channels per pixel; NULL = no colour).  pix_offset[0] = 0,
 * pix_offset[s + 1] - pix_offset[s] = h_s w_s, pix_offset[b] < 2^31.  pix_offset (b + 1 longs), hw (2 b ints), rtilt and k (b x 9
 * doubles, row-major Rtilt and K as votenet_select_boxes takes them) are HOST arrays.
 * The rule, per pixel (row, col) of value p:
 *   d16 = (p >> 3) | (p << 13) in 16 bits (encoding 0, the dataset's) or p (encoding 1, millimetres); the pixel is valid iff d16 != 0
 *   z = (double)d16 / 1000.0; z = max_depth where z > max_depth (the point is kept)
 *   u = col + pixel_origin, v = row + pixel_origin
 *   x = ((u - K[0,2]) z) / K[0,0], y = ((v - K[1,2]) z) / K[1,1], q = (x, z, -y)
 *   out_i = (R[i,0] q0 + R[i,1] q1) + R[i,2] q2
 * in double, un-fused, in this order, each coordinate rounded once to float; with colour, columns 3..5 are
 * (float)((double)c / 255.0) in the image's channel order.  raw_stride = 3 without colour, 6 with it.
 * raw (device, floats, 4-byte aligned): the rows of the valid pixels of scene 0 in row-major pixel order, then scene 1's, ... without
 * gaps -- upright-depth coordinates, what votenet_subsample_augment and votenet_select_boxes take as raw.  Rows from
 * raw_capacity_rows on are never written.  raw_offset_dev (device, b + 1 longs): raw_offset_dev[s] = the valid pixels before scene s,
 * raw_offset_dev[b] their total, whatever the capacity (raw may be NULL when it is 0: a count alone).  The bytes are the same from run
 * to run: no atomic decides a position.
 * Three launches on `stream`: the valid count of every tile of 2048 pixels (tiles never straddle scenes), a one-workgroup exclusive
 * scan over the tiles that also writes raw_offset_dev, and the pass that decodes again and writes.
 * Status 1, nothing launched: b outside [1, 32], a non-positive h or w, pix_offset that does not match hw, raw_stride other than 3
 * (no rgb) / 6 (rgb), ws_bytes < votenet_depth_scan_workspace_bytes(b, pix_offset[b]), K[0,0] or K[1,1] equal to 0, an unknown
 * encoding, a negative capacity, a null or misaligned pointer. */
int votenet_depth_scan(int b, const unsigned short *depth, const unsigned char *rgb, const long *pix_offset, const int *hw,
                       const double *rtilt, const double *k, int encoding, double pixel_origin, double max_depth, float *raw,
                       int raw_stride, long raw_capacity_rows, long *raw_offset_dev, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_DEPTH_SCAN_H */
