// vote_sampling.hip -- libvotenet_votesamp.so (include/votenet_vote_sampling.h), a library of its own beside libvotenet_hip.so (whose
// export list and whose sampling / grouping entries stay what they were): the proposal module's clusters sampled by farthest-point
// sampling on the VOTES, as the VoteNet paper does.
//   votenet_cluster_votes   fps_idx, new_xyz, idx, pts_cnt of a batch of vote clouds: what votenet_farthest_point_sample,
//                           votenet_gather_point and votenet_query_ball_point leave, bit for bit, in ONE launch.
//                           cluster_votes_kernel: a workgroup of 16 waves per scene.
// The votes exist only in the middle of a step's static stretch, so their sampling sits on its critical path; composed from the three
// entries it is five dependent launches (the two prefix-check kernels of fps.hip can never confirm on votes).  A scene is 1024 points:
//   sampling   fps.hip's register-resident round (fps_reg_kernel<4, P>) for n <= 2048, stated here for these sizes: waves 0..3 hold the
//              scene (P = 4 or 8 points per lane, slots in ascending tie key), a round is P un-fused distance updates per lane, a wave
//              arg-max, one LDS 64-bit maximum per wave and ONE barrier; the winner's coordinates travel through the exchange.  Waves
//              4..15 have nothing to sample: they take part in the round's barrier and nothing else (a wave asleep at a barrier
//              issues no instruction).  The picks go to LDS, and to memory after the loop.
//   centres    a raw copy of the scene in LDS (n * 12 bytes <= 24 KB): new_xyz is read from it by pick.
//   ball query all 16 waves, a wave per centre and a lane per candidate, 64 at a time from the LDS copy (stride 3 dwords: no bank
//              conflict): the hit mask is a ballot, a hit's slot the count so far plus the popcount of the ballot below the lane;
//              a wave stops when its row is full.
// Distances are non-negative (or +inf), so min / max / compare run on their bit patterns as unsigned integers, as in fps.hip; no NaN
// can arise in the sampling (the header's rule reads non-finite points as point 0).  Every index written is in [0, n): the ball query's
// by construction (candidate numbers), the picks' because only a real point can hold the maximum (point 0 is always real and wins
// every all-zero tie) -- and they are clamped where they are stored, so that not even a defect here could send the proposal MLP's
// gathers out of bounds.
#include "../common.h"
#include "../error_text.h"
#include "../ball_threshold.h" // ball_threshold: T(r) as votenet_query_ball_point forms it

#pragma GCC visibility push(default)
#include "../../../include/votenet_vote_sampling.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_votesamp_last_error()) ----
static thread_local ErrorText g_vs_err;
#define VS_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_vs_err, cond, __VA_ARGS__)

constexpr int VS_MAX_N = 2048;      // votes per scene: 8 per lane of the four sampling waves
constexpr int VS_MAX_M = 1024;      // clusters per scene
constexpr int VS_MAX_NSAMPLE = 64;  // a row is padded by one wave in one step
constexpr int VS_WAVES = 16;        // the workgroup
constexpr int VS_FPS_WAVES = 4;     // ... of which these sample (fps.hip's choice for n <= 2048)
constexpr int VS_FPS_T = VS_FPS_WAVES * 64;

__device__ __forceinline__ bool vs_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// Slot i of sampling lane `tid` -> point index.  256 lanes own two residues mod 512 each (tid and tid + 256); Q slots per residue, in
// ascending k: slots are in ascending tie key (k mod 512, k), so a strict '>' over the slots keeps the lane's smallest key.
template <int P>
__device__ __forceinline__ int vs_slot_to_k(int tid, int i)
{
    constexpr int Q = P / 2;
    return (i % Q) * 512 + (i / Q) * VS_FPS_T + tid;
}
// The tie key of point k < 2048 in 12 bits: (k mod 512, k / 512); 0xFFF: no point
__device__ __forceinline__ unsigned vs_tiekey(unsigned k) { return ((k & 511u) << 2) | (k >> 9); }
__device__ __forceinline__ unsigned vs_key_to_index(unsigned key) { return (key >> 2) | ((key & 3u) << 9); }

// wave64 reductions on unsigned keys, fps.hip's form: six dependent VOP2-DPP steps (the builtin form is a v_mov_dpp and the operation
// per step: twice the instructions on the round's critical path), result uniform
#define VS_DPP_REDUCE(OP)                                                                                    \
    asm volatile("s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t" \
                 OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"              \
                 OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                  \
                 OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"                       \
                 OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"                     \
                 OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"                         \
                 : "+v"(v))
__device__ __forceinline__ unsigned vs_wave_max_u32(unsigned v)
{
    VS_DPP_REDUCE("v_max_u32_dpp");
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned vs_wave_min_u32(unsigned v)
{
    VS_DPP_REDUCE("v_min_u32_dpp");
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Wave arg-max under (value descending, key ascending): the winning lane; vmax / kmin uniform.  The key reduction only runs when
// several lanes hold the maximum.
__device__ __forceinline__ int vs_wave_argmax(unsigned val, unsigned key, unsigned &vmax, unsigned &kmin)
{
    vmax = vs_wave_max_u32(val);
    unsigned long long hit = __ballot(val == vmax);
    if (hit & (hit - 1)) {
        kmin = vs_wave_min_u32(val == vmax ? key : 0xFFFFFFFFu);
        hit = __ballot(val == vmax && key == kmin);
        return __ffsll((long long)hit) - 1;
    }
    const int l = __ffsll((long long)hit) - 1;
    kmin = (unsigned)__builtin_amdgcn_readlane((int)key, l);
    return l;
}

struct VsLds {
    unsigned long long slot[3];              // the round's maximum of [ distance (32) | 0xFFF - key (12) | wave (4) ], by round % 3
    float4 cand[2][VS_FPS_WAVES];            // the waves' candidates' coordinates, by round parity
    int pick[VS_MAX_M];                      // fps_idx of the scene
    float raw[VS_MAX_N * 3];                 // the scene as it lies in memory
};

// The sampling rounds of waves 0..3 (tid < 256).  One LDS-only barrier per round, which waves 4..15 share (cluster_votes_kernel).
// The exchange is fps.hip's: lane 0 of each wave takes the maximum of a packed word in LDS -- its order is "largest distance, then
// smallest tie key" --; wave 0 clears the NEXT round's word before this round's barrier (its last readers passed the previous barrier,
// its next writers come after this one); the candidates' coordinates alternate between two tables.
template <int P>
__device__ __forceinline__ void vs_sample(VsLds &S, int n, int m, int tid)
{
    const int w = wave_id_uniform(), lane = lane_id();
    // point 0 as sampling reads it
    const float a0 = S.raw[0], b0 = S.raw[1], c0 = S.raw[2];
    const float x0 = vs_nonfinite(a0) ? 0.0f : a0, y0 = vs_nonfinite(b0) ? 0.0f : b0, z0 = vs_nonfinite(c0) ? 0.0f : c0;
    float x[P], y[P], z[P];
    unsigned td[P];
#pragma unroll
    for (int i = 0; i < P; i++) {
        const int k = vs_slot_to_k<P>(tid, i);
        const bool valid = k < n;
        x[i] = y[i] = z[i] = 0.0f;
        if (valid) {
            x[i] = S.raw[k * 3 + 0];
            y[i] = S.raw[k * 3 + 1];
            z[i] = S.raw[k * 3 + 2];
            if (k == 0 || vs_nonfinite(x[i]) || vs_nonfinite(y[i]) || vs_nonfinite(z[i])) x[i] = x0, y[i] = y0, z[i] = z0;
        }
        td[i] = valid ? __float_as_uint(1e38f) : 0u; // a slot without a point never wins
    }
    float cx = x0, cy = y0, cz = z0;
    for (int j = 1; j < m; j++) {
        unsigned best = 0u;
        int bi = 0;
        float bx = x[0], by = y[0], bz = z[0];
#pragma unroll
        for (int i = 0; i < P; i++) {
            const float dx = x[i] - cx, dy = y[i] - cy, dz = z[i] - cz;
            const float d = dx * dx + dy * dy + dz * dz; // un-fused, left to right (-ffp-contract=off)
            const unsigned d2 = min(__float_as_uint(d), td[i]);
            td[i] = d2;
            if (d2 > best) { // strict: the lowest slot (the lane's smallest tie key) wins ties
                best = d2;
                bi = i;
                bx = x[i];
                by = y[i];
                bz = z[i];
            }
        }
        const int bk = vs_slot_to_k<P>(tid, bi);
        const unsigned key = bk < n ? vs_tiekey((unsigned)bk) : 0xFFFu;
        unsigned wmax, wkey;
        const int fl = vs_wave_argmax(best, key, wmax, wkey);
        const float wx = readlane_f32(bx, fl), wy = readlane_f32(by, fl), wz = readlane_f32(bz, fl);
        const int cur = j % 3, nxt = cur == 2 ? 0 : cur + 1;
        if (lane == 0) {
            S.cand[j & 1][w] = make_float4(wx, wy, wz, 0.0f);
            atomicMax(&S.slot[cur], ((unsigned long long)wmax << 32) | ((0xFFFu - wkey) << 4) | (unsigned)w);
            if (w == 0) S.slot[nxt] = 0ull;
        }
        lds_barrier();
        const unsigned low = (unsigned)S.slot[cur];
        const float4 c = S.cand[j & 1][low & (VS_FPS_WAVES - 1)];
        cx = c.x;
        cy = c.y;
        cz = c.z;
        if (tid == 0) S.pick[j] = (int)vs_key_to_index(0xFFFu - ((low >> 4) & 0xFFFu)); // (read behind the loop's last barrier)
    }
}

template <int P>
__global__ __launch_bounds__(VS_WAVES * 64) void cluster_votes_kernel(int n, int m, float thr, int nsample,
                                                                        const float *__restrict__ votes, int *__restrict__ fps_idx,
                                                                        float *__restrict__ new_xyz, int *__restrict__ idx,
                                                                        int *__restrict__ pts_cnt)
{
    __shared__ VsLds S;
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id_uniform(), sc = blockIdx.x;
    const float *__restrict__ pts = votes + (size_t)sc * n * 3;
    for (int i = tid; i < n * 3; i += VS_WAVES * 64) S.raw[i] = pts[i];
    if (tid == 0) {
        S.slot[0] = S.slot[1] = S.slot[2] = 0ull;
        S.pick[0] = 0;
    }
    __syncthreads();
    // ---- sampling: m - 1 rounds, one barrier each, the same count on either side of the branch (w is uniform)
    if (w < VS_FPS_WAVES) {
        vs_sample<P>(S, n, m, tid);
    } else {
        for (int j = 1; j < m; j++) lds_barrier();
    }
    __syncthreads();
    // ---- the picks and their centres, from LDS
    int *__restrict__ ofps = fps_idx + (size_t)sc * m;
    float *__restrict__ oxyz = new_xyz + (size_t)sc * m * 3;
    for (int j = tid; j < m; j += VS_WAVES * 64) ofps[j] = min(max(S.pick[j], 0), n - 1);
    for (int e = tid; e < m * 3; e += VS_WAVES * 64) {
        const int j = e / 3;
        oxyz[e] = S.raw[min(max(S.pick[j], 0), n - 1) * 3 + (e - j * 3)];
    }
    // ---- ball query: wave w takes centres w, w + 16, ...; lane = candidate
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int q = w; q < m; q += VS_WAVES) {
        const int pk = __builtin_amdgcn_readfirstlane(min(max(S.pick[q], 0), n - 1));
        const float qx = S.raw[pk * 3 + 0], qy = S.raw[pk * 3 + 1], qz = S.raw[pk * 3 + 2];
        int *__restrict__ row = idx + ((size_t)sc * m + q) * nsample;
        int cnt = 0, first = 0; // uniform
        for (int base = 0; base < n && cnt < nsample; base += 64) {
            const int k = base + lane;
            const bool valid = k < n;
            const int kk = valid ? k : 0;
            const float dx = qx - S.raw[kk * 3 + 0], dy = qy - S.raw[kk * 3 + 1], dz = qz - S.raw[kk * 3 + 2];
            const float s = dx * dx + dy * dy + dz * dz; // un-fused; a NaN is no hit
            const bool hit = valid && s < thr;
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                const int pos = cnt + __popcll(mask & below);
                if (hit && pos < nsample) row[pos] = k;
                if (cnt == 0) first = base + __ffsll((long long)mask) - 1;
                cnt += __popcll(mask);
            }
        }
        const int c = cnt < nsample ? cnt : nsample;
        if (lane >= c && lane < nsample) row[lane] = first; // the first hit again; no hit: zeros
        if (lane == 0) pts_cnt[(size_t)sc * m + q] = c;
    }
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_votesamp_last_error(void) { return g_vs_err.text; }

extern "C" int votenet_cluster_votes(int b, int n, int m, float radius, int nsample, const float *votes_xyz, int *fps_idx,
                                     float *new_xyz, int *idx, int *pts_cnt, void *stream)
{
    VS_REQUIRE(b >= 0, "cluster_votes: a batch of b >= 0 scenes expected, got b = %d", b);
    VS_REQUIRE(n >= 1 && n <= VS_MAX_N, "cluster_votes: 1 to %d votes per scene, got n = %d", VS_MAX_N, n);
    VS_REQUIRE(m >= 1 && m <= VS_MAX_M, "cluster_votes: 1 to %d clusters per scene, got m = %d", VS_MAX_M, m);
    VS_REQUIRE(nsample >= 1 && nsample <= VS_MAX_NSAMPLE, "cluster_votes: 1 to %d votes per cluster, got nsample = %d", VS_MAX_NSAMPLE,
               nsample);
    VS_REQUIRE(radius > 0, "cluster_votes: a positive radius expected, got %g", (double)radius); // (a NaN is refused too)
    if (b == 0) return VOTENET_OK;
    VS_REQUIRE(votes_xyz && fps_idx && new_xyz && idx && pts_cnt, "cluster_votes: null buffer");
    // d = max(sqrtf(s), 1e-20f) >= 1e-20: nothing can be closer than a radius <= 1e-20 (votenet_query_ball_point's rule)
    const float thr = (radius <= 1e-20f) ? -1.0f : ball_threshold(radius);
    hipStream_t st = as_stream(stream);
    if (n <= 1024)
        hipLaunchKernelGGL((cluster_votes_kernel<4>), dim3(b), dim3(VS_WAVES * 64), 0, st, n, m, thr, nsample, votes_xyz, fps_idx, new_xyz,
                           idx, pts_cnt);
    else
        hipLaunchKernelGGL((cluster_votes_kernel<8>), dim3(b), dim3(VS_WAVES * 64), 0, st, n, m, thr, nsample, votes_xyz, fps_idx, new_xyz,
                           idx, pts_cnt);
    return g_vs_err.check_launch("cluster_votes");
}
