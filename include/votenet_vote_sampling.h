/*
 * votenet_vote_sampling.h -- C ABI of libvotenet_votesamp.so: the proposal module's clusters sampled by farthest-point sampling on the
 * VOTES, as the VoteNet paper does (its `vote_fps`), on the MI355X (gfx950): sampling, centres and ball query of a batch of vote clouds
 * in one launch.  A library of its own, as libvotenet_monitors.so ... libvotenet_propsup.so are: the other libraries export what they
 * did, and a run that does not ask for the mode never loads this one.  Beside the reference, which samples the SEEDS and takes their
 * votes as centres (utils.py:42-43, model.py:89-93).  Conventions as in votenet_hip.h: extern "C", an explicit stream (hipStream_t as
 * void*; NULL = the null stream), an int status (0 = ok, 1 = invalid argument, 2 = HIP error; text via votenet_votesamp_last_error()),
 * the caller owns every buffer, no launcher allocates or synchronises, nothing is read back.
 *
 * The rule.  votes_xyz (b, n, 3) float32 contiguous; 1 <= n <= 2048, 1 <= m <= 1024, 1 <= nsample <= 64, radius > 0, b >= 0.  The
 * four outputs are, bit for bit, what votenet_farthest_point_sample(b, n, m, votes), votenet_gather_point(votes, fps_idx) and
 * votenet_query_ball_point(b, n, m, radius, nsample, votes, new_xyz) of votenet_hip.h leave; stated in full, per scene, all arithmetic
 * fp32, un-fused, in the order written:
 *   sampling:  the cloud as sampling reads it: a component of point 0 that is NaN or infinite reads as 0; a point k > 0 with a NaN or
 *              infinite component reads as a copy of (that) point 0.  fps_idx[0] = 0; running distance t_k = 1e38f for every k.  For
 *              j = 1 .. m-1, with c the point picked last: d_k = ((x_k - c_x) * (x_k - c_x) + (y_k - c_y) * (y_k - c_y)) +
 *              (z_k - c_z) * (z_k - c_z); t_k = d_k < t_k ? d_k : t_k; fps_idx[j] = the k of the largest t_k, among equals the
 *              smallest k mod 512, among those the smallest k.  So a point with a non-finite component is never sampled (it sits at
 *              distance 0 from the first pick, and index 0 wins every all-zero tie); once every t_k is 0 (m > n, duplicates) index 0
 *              repeats; finite coordinates whose squares overflow give d_k = +inf, which t_k = 1e38f caps: no NaN arises.
 *   centres:   new_xyz[j] = the RAW votes_xyz[fps_idx[j]], bit for bit (point 0's non-finite components included).
 *   ball query: for centre q and candidate k, on the raw coordinates: s = ((q_x - x_k) * (q_x - x_k) + (q_y - y_k) * (q_y - y_k)) +
 *              (q_z - z_k) * (q_z - z_k); a hit is s < T, T = votenet_ball_threshold(radius) of votenet_hip.h: the smallest fp32 whose
 *              correctly rounded sqrtf is >= radius (formed on the host inside the entry; radius <= 1e-20f: nothing is a hit).  A NaN
 *              s is no hit.  idx[j, 0 .. c-1] = the first c = min(hits, nsample) hits in ascending k, idx[j, c ..] = idx[j, 0];
 *              pts_cnt[j] = c.  A centre without a hit (a non-finite one) gets a row of zeros and pts_cnt 0.
 * Every index written lies in [0, n), whatever the votes hold.
 */
#ifndef VOTENET_VOTE_SAMPLING_H
#define VOTENET_VOTE_SAMPLING_H

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error this library raised on the calling thread ("" if none). */
const char *votenet_votesamp_last_error(void);

/* fps_idx (b, m) int32, new_xyz (b, m, 3) float32, idx (b, m, nsample) int32, pts_cnt (b, m) int32: all written in full.  A shape
 * outside the limits above, or a null buffer with b > 0, returns 1 with a text that names the limit, and nothing is launched; b == 0
 * is ok and launches nothing.  One launch, one workgroup per scene: the scene's votes stay in the workgroup's registers over the m - 1
 * sampling rounds (one barrier per round, no memory access on a round's critical path), a raw copy in LDS serves the centres and the
 * ball query (a wave per centre, a lane per candidate, hits placed by ballot and popcount).  No workgroup waits for another, no float
 * atomic: two calls write the same bytes. */
int votenet_cluster_votes(int b, int n, int m, float radius, int nsample, const float *votes_xyz, int *fps_idx, float *new_xyz,
                          int *idx, int *pts_cnt, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOTENET_VOTE_SAMPLING_H */
