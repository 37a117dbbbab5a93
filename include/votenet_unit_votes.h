/*
 * votenet_unit_votes.h -- C ABI of libvotenet_unitvote.so: the vote features divided by their L2 norm, as the authors' VoteNet does
 * between its voting module and its proposal module (features.div(torch.norm(features, p=2, dim=1))), on the MI355X (gfx950): the sum
 * votes = x + offset, its split into xyz and features and the normalisation in ONE launch, and their backward in ONE launch -- each in
 * the place of the glue launch (votenet_row_segments) that forms the same buffers without the normalisation.  A library of its own, as
 * libvotenet_monitors.so ... libvotenet_instvote.so are: the other libraries export what they did, and a run that does not ask for the
 * mode never loads this one.  Beside the reference, which hands the un-normalised sum to its proposal module (model.py:60, 85).
 * Conventions as in votenet_hip.h: extern "C", an explicit stream (hipStream_t as void*; NULL = the null stream), an int status (0 = ok,
 * 1 = invalid argument, 2 = HIP error; text via votenet_unitvote_last_error()), the caller owns every buffer, no launcher allocates or
 * synchronises, nothing is read back.
 *
 * Shapes.  `rows` rows of c feature channels behind 3 coordinates: c % 64 == 0, 64 <= c <= 512; 0 <= rows <= 4 * (2^31 - 1) (four rows per
 * workgroup, 2^31 - 1 workgroups per launch); every row offset is formed in 64 bits.  x and off are (rows, 3 + c) float32 views with row pitches x_pitch, off_pitch
 * >= 3 + c in ELEMENTS (the features start at element 3 of a row and a pitch may be odd: no operand need be aligned beyond 4 bytes).
 * votes_xyz (rows, 3), votes_points (rows, c), norm (rows), d_xyz, cot_xyz (rows, 3) and d_points (rows, c) are contiguous.
 *
 * The rule, per row; all arithmetic fp32, un-fused, in the order written.  A wave of 64 lanes owns the row; lane l owns channels
 * l, l + 64, l + 128, ...
 *   forward:   votes_xyz[k] = x[k] + off[k] for k < 3 (the bits votenet_row_segments writes).  u_k = x[3 + k] + off[3 + k].
 *              p_l = ((u_l * u_l + u_{l+64} * u_{l+64}) + u_{l+128} * u_{l+128}) + ... in ascending channel order; the 64 partials are
 *              combined by an xor butterfly, p_l = p_l + p_{l ^ s} for s = 32, 16, 8, 4, 2, 1 in that order (every lane ends with the
 *              same bits).  norm = sqrtf(p), correctly rounded; votes_points[k] = u_k / norm, correctly rounded.
 *              No epsilon, as in the authors' code: a row of zeros gives NaN in its features and norm 0; a row whose squares overflow
 *              gives norm = +inf and features 0; a NaN channel makes its row's features and norm NaN.  No other row is touched.
 *   backward:  with y = votes_points, g = d_points: q_l = ((y_l * g_l + y_{l+64} * g_{l+64}) + ...) and the same butterfly give dot;
 *              d_votes[3 + k] = (g_k - y_k * dot) / norm, a correctly rounded division: the gradient of the un-normalised sum u.
 *              d_votes[k] = d_xyz[k] + cot_xyz[k] for k < 3, or d_xyz[k] itself when cot_xyz is NULL.  Columns 3 + c .. d_width - 1
 *              are written as zeros; elements d_width .. d_pitch - 1 of a row are not written.
 * No atomics, no workgroup waits for another: two calls write the same bytes.
 */
#ifndef VOTENET_UNIT_VOTES_H
#define VOTENET_UNIT_VOTES_H

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_unitvote_last_error(void);

/* votes_xyz (rows, 3), votes_points (rows, c), norm (rows): all written in full.  A shape outside the limits above, or a null buffer
 * with rows > 0, returns 1 with a text that names the limit, and nothing is launched; rows == 0 is ok and launches nothing.  One launch:
 * a wave per row, four rows per workgroup of 256 threads, every load of a row issued before its first use. */
int votenet_unit_votes(long rows, int c, const float *x, long x_pitch, const float *off, long off_pitch, float *votes_xyz,
                       float *votes_points, float *norm, void *stream);

/* d_votes (rows, d_width) float32 at row pitch d_pitch >= d_width >= 3 + c (elements): columns 0 .. d_width - 1 of every row written.
 * votes_points and norm are what votenet_unit_votes left.  Limits, errors and the launch shape as above. */
int votenet_unit_votes_backward(long rows, int c, const float *d_xyz, const float *cot_xyz /* may be NULL */, const float *d_points,
                                const float *votes_points, const float *norm, float *d_votes, long d_pitch, int d_width, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_UNIT_VOTES_H */
