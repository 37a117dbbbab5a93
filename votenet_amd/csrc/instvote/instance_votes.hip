// instance_votes.hip -- libvotenet_instvote.so (include/votenet_instance_votes.h), a library of its own beside libvotenet_hip.so and
// libvotenet_votesup.so (whose export lists stay what they were): vote supervision from instance labels.
//   votenet_seed_points          the cloud point every seed is.  seed_points_kernel: elementwise, a workgroup per (seed tile, scene).
//   votenet_instance_vote_loss   the loss, its cotangent and the re-formed total, one launch behind votenet_loss.
//                                instance_vote_loss_kernel: a workgroup per scene, shaped like paper_vote_loss_kernel (votesup/).
// A seed's box row is three dependent gathers away (idx2 -> idx1 -> point_box).  A lane keeps IV_SPT seeds and issues each level of
// its IV_SPT chains together before it consumes any of them, so a tile pays three memory latencies, not 3 * IV_SPT.  An index that
// fails its bound is replaced by 0 and its result discarded by a select: no load sits under a divergent branch (which costs a full
// vmcnt(0) drain), and no unchecked value ever forms an address.  The arithmetic of the header is plain fp32 in a fixed order
// (-ffp-contract=off, as everywhere in this project): tests/instance_votes_ref.py restates it in numpy float32 and picks, counts and
// cotangents are compared exactly.
#include "../common.h"
#include "../error_text.h"
#include "../nearest_box.h" // LOSS_MAXBOX: the boxes per scene votenet_loss takes
#include "../scene_fold.h"

#pragma GCC visibility push(default)
#include "../../../include/votenet_instance_votes.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_instvote_last_error()) ----
static thread_local ErrorText g_iv_err;
#define IV_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_iv_err, cond, __VA_ARGS__)

constexpr int IV_MAX_B = 65535;              // scenes: a grid extent
constexpr int IV_THREADS = 256;              // four waves
constexpr int IV_SPT = 4;                    // seeds a lane keeps in registers: paper_vote_loss_kernel's layout, so its sums' order
constexpr int IV_TILE = IV_THREADS * IV_SPT; // 1024 seeds: the training shape is one tile per scene
constexpr int IV_WAVES = IV_THREADS / 64;

__device__ __forceinline__ bool in_range(int v, int bound) { return (unsigned)v < (unsigned)bound; } // 0 <= v < bound, bound >= 1

// The chains of this lane's seeds of the tile at `base` of a scene: seed base + k * IV_THREADS + tid in slot k (coalesced rows).
//   point[k]  the cloud point the seed is, -1 where an index of the chain is out of range (or the seed is beyond n)
//   row[k]    point_box of that point where the chain is valid (any value: the caller compares it with bb), -1 otherwise
// Each level's IV_SPT loads are issued before the level below consumes one.  WITH_ROW = false: the first two levels only.
template <bool WITH_ROW>
__device__ __forceinline__ void resolve(const int *__restrict__ idx1, const int *__restrict__ idx2, const int *__restrict__ point_box,
                                        int n0, int n1, int n, int base, int tid, int (&point)[IV_SPT], int (&row)[IV_SPT])
{
    int i[IV_SPT], p[IV_SPT], r[IV_SPT];
    bool ok[IV_SPT];
#pragma unroll
    for (int k = 0; k < IV_SPT; k++) {
        const int j = base + k * IV_THREADS + tid;
        ok[k] = j < n;
        i[k] = idx2[ok[k] ? j : 0];
    }
#pragma unroll
    for (int k = 0; k < IV_SPT; k++) {
        ok[k] = ok[k] & in_range(i[k], n1); // (&, not &&: a select, no branch round the load below)
        p[k] = idx1[ok[k] ? i[k] : 0];
    }
#pragma unroll
    for (int k = 0; k < IV_SPT; k++) {
        ok[k] = ok[k] & in_range(p[k], n0);
        if constexpr (WITH_ROW) r[k] = point_box[ok[k] ? p[k] : 0];
        else r[k] = -1;
    }
#pragma unroll
    for (int k = 0; k < IV_SPT; k++) {
        point[k] = ok[k] ? p[k] : -1;
        row[k] = ok[k] ? r[k] : -1;
    }
}

__global__ __launch_bounds__(IV_THREADS) void seed_points_kernel(int n0, int n1, int n, const int *__restrict__ idx1,
                                                                 const int *__restrict__ idx2, int *__restrict__ seed_point)
{
    const int sc = blockIdx.y, tid = threadIdx.x, base = blockIdx.x * IV_TILE;
    int point[IV_SPT], row[IV_SPT];
    resolve<false>(idx1 + (size_t)sc * n1, idx2 + (size_t)sc * n, nullptr, n0, n1, n, base, tid, point, row);
#pragma unroll
    for (int k = 0; k < IV_SPT; k++) {
        const int j = base + k * IV_THREADS + tid;
        if (j < n) seed_point[(size_t)sc * n + j] = point[k];
    }
}

struct InstVoteArgs {
    int b, n0, n1, n, bb;
    const int *idx1, *idx2, *point_box;
    const float *votes, *xyz;
    float *losses, *d_votes;
    int *counts;
    int *ticket; // the workspace of scene_fold (one sum per scene): zero on entry, left zero
};

// One workgroup per scene.  Pass 1: the supervised seeds P (and the diagnostic count Q) of the WHOLE batch, counted by every workgroup
// for itself (integers, so every workgroup arrives at the same P whatever its order): no workgroup waits for another before it scales
// its cotangents.  The walk over the scenes ends with the workgroup's own, so at the training shape (one tile per scene) the own
// scene's rows are still in registers.  Pass 2: the own scene's distances and cotangents, the targets read from the scene's centres
// in LDS.  The sum of the distances: ascending seeds inside a lane, lanes by wave shuffles, waves in order; the scenes' sums are folded
// in scene order by the last workgroup to finish.
__global__ __launch_bounds__(IV_THREADS) void instance_vote_loss_kernel(InstVoteArgs A)
{
    __shared__ float4 s_xyz[LOSS_MAXBOX];
    __shared__ int s_cnt[IV_WAVES][2];
    __shared__ float s_sum[IV_WAVES];
    const int tid = threadIdx.x, own = blockIdx.x, B = A.b, N = A.n, N0 = A.n0, N1 = A.n1, BB = A.bb;
    // the own scene's centres: loaded first, under the gathers of pass 1; visible behind the barrier of the count
    for (int j = tid; j < BB; j += IV_THREADS) {
        const float *c = A.xyz + ((size_t)own * BB + j) * 3;
        s_xyz[j] = make_float4(c[0], c[1], c[2], 0.0f);
    }
    int point[IV_SPT], row[IV_SPT];
    int cnt = 0, bad = 0;
    for (int t = 1; t <= B; t++) {
        const int sc = (own + t) % B;
        for (int base = 0; base < N; base += IV_TILE) {
            resolve<true>(A.idx1 + (size_t)sc * N1, A.idx2 + (size_t)sc * N, A.point_box + (size_t)sc * N0, N0, N1, N, base, tid, point, row);
#pragma unroll
            for (int k = 0; k < IV_SPT; k++) {
                const bool live = base + k * IV_THREADS + tid < N;
                cnt += in_range(row[k], BB);
                bad += live & ((point[k] < 0) | (row[k] >= BB));
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off), bad += __shfl_down(bad, off);
    if ((tid & 63) == 0) s_cnt[tid >> 6][0] = cnt, s_cnt[tid >> 6][1] = bad;
    __syncthreads();
    int P = 0, Q = 0;
#pragma unroll
    for (int w = 0; w < IV_WAVES; w++) P += s_cnt[w][0], Q += s_cnt[w][1];
    const float inv = 1.0f / ((float)P + 1e-6f);
    // ---- pass 2: the own scene
    const float *votes = A.votes + (size_t)own * N * 3;
    float *d_votes = A.d_votes + (size_t)own * N * 3;
    float sum = 0.0f;
    for (int base = 0; base < N; base += IV_TILE) {
        if (N > IV_TILE) // (uniform: at one tile per scene the registers hold this tile's rows from pass 1)
            resolve<true>(A.idx1 + (size_t)own * N1, A.idx2 + (size_t)own * N, A.point_box + (size_t)own * N0, N0, N1, N, base, tid, point, row);
        float vx[IV_SPT], vy[IV_SPT], vz[IV_SPT];
#pragma unroll
        for (int k = 0; k < IV_SPT; k++) { // every lane loads: a seed beyond n reads seed 0 and stores nothing
            const int j = base + k * IV_THREADS + tid;
            const size_t e = (size_t)(j < N ? j : 0) * 3;
            vx[k] = votes[e + 0], vy[k] = votes[e + 1], vz[k] = votes[e + 2];
        }
#pragma unroll
        for (int k = 0; k < IV_SPT; k++) {
            const int j = base + k * IV_THREADS + tid;
            const bool sup = in_range(row[k], BB);
            const float4 t = s_xyz[sup ? row[k] : 0];
            const float ex = vx[k] - t.x, ey = vy[k] - t.y, ez = vz[k] - t.z;
            const float d = (fabsf(ex) + fabsf(ey)) + fabsf(ez);
            sum += sup ? d : 0.0f;
            const float g0 = sup ? (float)((ex > 0.0f) - (ex < 0.0f)) * inv : 0.0f;
            const float g1 = sup ? (float)((ey > 0.0f) - (ey < 0.0f)) * inv : 0.0f;
            const float g2 = sup ? (float)((ez > 0.0f) - (ez < 0.0f)) * inv : 0.0f;
            if (j < N) {
                const size_t e = (size_t)j * 3;
                d_votes[e + 0] = g0, d_votes[e + 1] = g1, d_votes[e + 2] = g2;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid != 0) return;
    float v[1] = {0.0f}, total[1];
#pragma unroll
    for (int w = 0; w < IV_WAVES; w++) v[0] += s_sum[w];
    if (!scene_fold(A.ticket, own, B, v, total)) return;
    const float vote = total[0] * inv;
    float *L = A.losses;
    L[0] = vote + 0.5f * L[2] + L[9] + 0.1f * L[8]; // votenet_loss's total (loss.hip), from the components it stored
    L[1] = vote;
    if (A.counts) A.counts[0] = P, A.counts[1] = Q;
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_instvote_last_error(void) { return g_iv_err.text; }

extern "C" size_t votenet_instvote_workspace_bytes(int b) { return scene_fold_bytes(b, 1); }

static int check_levels(const char *who, int b, int n0, int n1, int n)
{
    IV_REQUIRE(b >= 1 && b <= IV_MAX_B, "%s: 1 to %d scenes, got b = %d", who, IV_MAX_B, b);
    IV_REQUIRE(n >= 1 && (long)b * n * 3 < (1L << 31), "%s: n >= 1 and b * n * 3 < 2^31 expected, got b = %d, n = %d", who, b, n);
    IV_REQUIRE(n1 >= 1, "%s: n1 >= 1 expected, got n1 = %d", who, n1);
    IV_REQUIRE(n0 >= 1 && (long)b * n0 < (1L << 31), "%s: n0 >= 1 and b * n0 < 2^31 expected, got b = %d, n0 = %d", who, b, n0);
    return VOTENET_OK;
}

extern "C" int votenet_seed_points(int b, int n0, int n1, int n, const int *idx1, const int *idx2, int *seed_point, void *stream)
{
    if (int rc = check_levels("seed_points", b, n0, n1, n)) return rc;
    IV_REQUIRE(idx1 && idx2 && seed_point, "seed_points: null buffer");
    hipLaunchKernelGGL(seed_points_kernel, dim3((n + IV_TILE - 1) / IV_TILE, b), dim3(IV_THREADS), 0, as_stream(stream), n0, n1, n, idx1,
                       idx2, seed_point);
    return g_iv_err.check_launch("seed_points");
}

extern "C" int votenet_instance_vote_loss(int b, int n0, int n1, int n, int bb, const int *idx1, const int *idx2, const int *point_box,
                                          const float *votes, const float *xyz, float *losses, float *d_votes, int *counts,
                                          void *workspace, void *stream)
{
    if (int rc = check_levels("instance_vote_loss", b, n0, n1, n)) return rc;
    IV_REQUIRE(bb >= 1 && bb <= LOSS_MAXBOX, "instance_vote_loss: 1 to %d boxes per scene, got bb = %d", LOSS_MAXBOX, bb);
    IV_REQUIRE(idx1 && idx2 && point_box && votes && xyz && losses && d_votes && workspace, "instance_vote_loss: null buffer");
    const size_t bytes = (size_t)b * n * 3 * sizeof(float);
    const uintptr_t src = reinterpret_cast<uintptr_t>(votes), dst = reinterpret_cast<uintptr_t>(d_votes);
    IV_REQUIRE(dst + bytes <= src || src + bytes <= dst, "instance_vote_loss: d_votes may not overlap votes");
    IV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "instance_vote_loss: the workspace must be 4-byte aligned");
    InstVoteArgs a = {b, n0, n1, n, bb, idx1, idx2, point_box, votes, xyz, losses, d_votes, counts, static_cast<int *>(workspace)};
    hipLaunchKernelGGL(instance_vote_loss_kernel, dim3(b), dim3(IV_THREADS), 0, as_stream(stream), a);
    return g_iv_err.check_launch("instance_vote_loss");
}
