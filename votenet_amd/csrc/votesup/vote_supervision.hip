// vote_supervision.hip -- libvotenet_votesup.so (include/votenet_vote_supervision.h), a library of its own beside libvotenet_hip.so
// (whose export list and whose votenet_loss stay what they were): the vote supervision of the VoteNet paper.
//   votenet_vote_targets      the three target slots and the box count of every seed.  vote_targets_kernel: a workgroup per (seed tile,
//                             scene).
//   votenet_paper_vote_loss   the loss, its cotangent and the re-formed total, one launch behind votenet_loss.  paper_vote_loss_kernel: a
//                             workgroup per scene.
// Both keep VS_SPT seeds per lane in registers over the whole box loop; the eight constants of a box are formed once per workgroup
// into LDS and read wave-uniformly (two 16-byte broadcasts).  The rule of the header is plain fp32 arithmetic in a fixed order
// (-ffp-contract=off, as everywhere in this project): tests/vote_supervision_ref.py restates it in numpy float32 and slots, counts and
// cotangents are compared exactly.
#include "../common.h"
#include "../error_text.h"
#include "../nearest_box.h" // LOSS_MAXBOX: the boxes per scene votenet_loss takes
#include "../scene_fold.h"

#pragma GCC visibility push(default)
#include "../../../include/votenet_vote_supervision.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_votesup_last_error()) ----
static thread_local ErrorText g_vs_err;
#define VS_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_vs_err, cond, __VA_ARGS__)

constexpr int VS_MAX_B = 65535;              // scenes: a grid extent
constexpr int VS_THREADS = 256;              // four waves
constexpr int VS_SPT = 4;                    // seeds a lane keeps in registers
constexpr int VS_TILE = VS_THREADS * VS_SPT; // 1024 seeds: the training shape is one tile per scene
constexpr int VS_WAVES = VS_THREADS / 64;

// The constants of scene `sc`'s boxes into LDS: {cx, cy, cz, c}, {s, hl, hh, hw}.  The trigonometry in double, rounded once.
__device__ __forceinline__ void stage_boxes(float4 (*s_box)[2], int bb, const float *__restrict__ xyz, const float *__restrict__ lwh,
                                            const float *__restrict__ roty, int tid)
{
    for (int j = tid; j < bb; j += VS_THREADS) {
        const double a = (double)roty[j];
        const float c = (float)cos(a), s = (float)sin(a);
        s_box[j][0] = make_float4(xyz[j * 3 + 0], xyz[j * 3 + 1], xyz[j * 3 + 2], c);
        s_box[j][1] = make_float4(s, 0.5f * lwh[j * 3 + 0], 0.5f * lwh[j * 3 + 2], 0.5f * lwh[j * 3 + 1]);
    }
}

__device__ __forceinline__ bool inside_box(const float4 a0, const float4 a1, float px, float py, float pz)
{
    const float qx = px - a0.x, qy = py - a0.y, qz = pz - a0.z;
    const float x0 = a0.w * qx - a1.x * qz;
    const float z0 = a1.x * qx + a0.w * qz;
    return fabsf(x0) <= a1.y && fabsf(qy) <= a1.z && fabsf(z0) <= a1.w;
}

// This lane's seeds of the tile at `base` of a scene: seed base + k * VS_THREADS + tid in slot k (coalesced rows); beyond n: NaN, in no box.
__device__ __forceinline__ void load_seeds(const float *__restrict__ scene, int n, int base, int tid, float (&px)[VS_SPT],
                                           float (&py)[VS_SPT], float (&pz)[VS_SPT])
{
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < VS_SPT; k++) {
        const int i = base + k * VS_THREADS + tid;
        const bool live = i < n;
        px[k] = live ? scene[(size_t)i * 3 + 0] : nan;
        py[k] = live ? scene[(size_t)i * 3 + 1] : nan;
        pz[k] = live ? scene[(size_t)i * 3 + 2] : nan;
    }
}

// The boxes that contain each of the lane's seeds, in index order: their number, the first, the second and the last.
struct Hits {
    int k[VS_SPT], first[VS_SPT], second[VS_SPT], last[VS_SPT];
};
__device__ __forceinline__ void scan_boxes(const float4 (*s_box)[2], int bb, const float (&px)[VS_SPT], const float (&py)[VS_SPT],
                                           const float (&pz)[VS_SPT], Hits &h)
{
#pragma unroll
    for (int k = 0; k < VS_SPT; k++) h.k[k] = 0, h.first[k] = h.second[k] = h.last[k] = -1;
    for (int j = 0; j < bb; j++) {
        const float4 a0 = s_box[j][0], a1 = s_box[j][1];
#pragma unroll
        for (int k = 0; k < VS_SPT; k++) {
            const bool in = inside_box(a0, a1, px[k], py[k], pz[k]);
            h.first[k] = in && h.k[k] == 0 ? j : h.first[k];
            h.second[k] = in && h.k[k] == 1 ? j : h.second[k];
            h.last[k] = in ? j : h.last[k];
            h.k[k] += in;
        }
    }
}
// slots 0, 1, 2 of a seed with k >= 1 boxes
__device__ __forceinline__ void slots_of(const Hits &h, int k, int (&slot)[3])
{
    slot[0] = h.first[k];
    slot[1] = h.k[k] >= 2 ? h.second[k] : h.first[k];
    slot[2] = h.k[k] >= 3 ? h.last[k] : h.first[k];
}

__global__ __launch_bounds__(VS_THREADS) void vote_targets_kernel(int n, int bb, const float *__restrict__ seeds,
                                                                  const float *__restrict__ xyz, const float *__restrict__ lwh,
                                                                  const float *__restrict__ roty, int *__restrict__ slots,
                                                                  int *__restrict__ inside_count)
{
    __shared__ float4 s_box[LOSS_MAXBOX][2];
    const int sc = blockIdx.y, tid = threadIdx.x, base = blockIdx.x * VS_TILE;
    stage_boxes(s_box, bb, xyz + (size_t)sc * bb * 3, lwh + (size_t)sc * bb * 3, roty + (size_t)sc * bb, tid);
    __syncthreads();
    float px[VS_SPT], py[VS_SPT], pz[VS_SPT];
    load_seeds(seeds + (size_t)sc * n * 3, n, base, tid, px, py, pz);
    Hits h;
    scan_boxes(s_box, bb, px, py, pz, h);
#pragma unroll
    for (int k = 0; k < VS_SPT; k++) {
        const int i = base + k * VS_THREADS + tid;
        if (i >= n) continue;
        int slot[3];
        slots_of(h, k, slot); // (k = 0: first = -1, all three -1)
        const size_t e = (size_t)sc * n + i;
        slots[e * 3 + 0] = slot[0];
        slots[e * 3 + 1] = slot[1];
        slots[e * 3 + 2] = slot[2];
        inside_count[e] = h.k[k];
    }
}

struct VoteLossArgs {
    int b, n, bb;
    const float *seeds, *votes, *xyz, *lwh, *roty;
    float *losses, *d_votes;
    int *supervised;
    int *ticket; // the workspace of scene_fold (one sum per scene): zero on entry, left zero
};

// One workgroup per scene.  Pass 1: the supervised seeds of the WHOLE batch, counted by every workgroup for itself (b * n * bb closed-box
// tests over 256 lanes; an integer, so every workgroup arrives at the same P whatever its order): no workgroup waits for another before
// it scales its cotangents.  The walk over the scenes ends with the workgroup's own, whose box constants then stay in LDS.  Pass 2: the
// own scene's slots, minima and cotangents.  The sum of the minima: ascending seeds inside a lane, lanes by wave shuffles, waves in
// order; the scenes' sums are folded in scene order by the last workgroup to finish.
__global__ __launch_bounds__(VS_THREADS) void paper_vote_loss_kernel(VoteLossArgs A)
{
    __shared__ float4 s_box[LOSS_MAXBOX][2];
    __shared__ int s_cnt[VS_WAVES];
    __shared__ float s_sum[VS_WAVES];
    const int tid = threadIdx.x, own = blockIdx.x, B = A.b, N = A.n, BB = A.bb;
    float px[VS_SPT], py[VS_SPT], pz[VS_SPT];
    int cnt = 0;
    for (int t = 1; t <= B; t++) {
        const int sc = (own + t) % B;
        __syncthreads(); // the scene before this one has been read
        stage_boxes(s_box, BB, A.xyz + (size_t)sc * BB * 3, A.lwh + (size_t)sc * BB * 3, A.roty + (size_t)sc * BB, tid);
        __syncthreads();
        for (int base = 0; base < N; base += VS_TILE) {
            load_seeds(A.seeds + (size_t)sc * N * 3, N, base, tid, px, py, pz);
            bool any[VS_SPT];
#pragma unroll
            for (int k = 0; k < VS_SPT; k++) any[k] = false;
            for (int j = 0; j < BB; j++) {
                const float4 a0 = s_box[j][0], a1 = s_box[j][1];
#pragma unroll
                for (int k = 0; k < VS_SPT; k++) any[k] = any[k] || inside_box(a0, a1, px[k], py[k], pz[k]);
            }
#pragma unroll
            for (int k = 0; k < VS_SPT; k++) cnt += any[k];
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    int P = 0;
#pragma unroll
    for (int w = 0; w < VS_WAVES; w++) P += s_cnt[w];
    const float inv = 1.0f / ((float)P + 1e-6f);
    // ---- pass 2: the own scene (its constants are the ones in LDS)
    float sum = 0.0f;
    for (int base = 0; base < N; base += VS_TILE) {
        load_seeds(A.seeds + (size_t)own * N * 3, N, base, tid, px, py, pz);
        Hits h;
        scan_boxes(s_box, BB, px, py, pz, h);
#pragma unroll
        for (int k = 0; k < VS_SPT; k++) {
            const int i = base + k * VS_THREADS + tid;
            if (i >= N) continue;
            const size_t e = ((size_t)own * N + i) * 3;
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
            if (h.k[k] >= 1) {
                int slot[3];
                slots_of(h, k, slot);
                const float vx = A.votes[e + 0], vy = A.votes[e + 1], vz = A.votes[e + 2];
                float best = 0.0f;
                int g = slot[0];
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    const float4 t = s_box[slot[m]][0];
                    const float d = (fabsf(vx - t.x) + fabsf(vy - t.y)) + fabsf(vz - t.z);
                    if (m == 0 || d < best) { // the first strict minimum
                        best = d;
                        g = slot[m];
                    }
                }
                sum += best;
                const float4 t = s_box[g][0];
                const float ex = vx - t.x, ey = vy - t.y, ez = vz - t.z;
                g0 = (float)((ex > 0.0f) - (ex < 0.0f)) * inv;
                g1 = (float)((ey > 0.0f) - (ey < 0.0f)) * inv;
                g2 = (float)((ez > 0.0f) - (ez < 0.0f)) * inv;
            }
            A.d_votes[e + 0] = g0;
            A.d_votes[e + 1] = g1;
            A.d_votes[e + 2] = g2;
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid != 0) return;
    float v[1] = {0.0f}, total[1];
#pragma unroll
    for (int w = 0; w < VS_WAVES; w++) v[0] += s_sum[w];
    if (!scene_fold(A.ticket, own, B, v, total)) return;
    const float vote = total[0] * inv;
    float *L = A.losses;
    L[0] = vote + 0.5f * L[2] + L[9] + 0.1f * L[8]; // votenet_loss's total (loss.hip), from the components it stored
    L[1] = vote;
    if (A.supervised) *A.supervised = P;
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_votesup_last_error(void) { return g_vs_err.text; }

extern "C" size_t votenet_votesup_workspace_bytes(int b) { return scene_fold_bytes(b, 1); }

static int check_shape(const char *who, int b, int n, int bb)
{
    VS_REQUIRE(b >= 1 && b <= VS_MAX_B, "%s: 1 to %d scenes, got b = %d", who, VS_MAX_B, b);
    VS_REQUIRE(n >= 1 && (long)b * n * 3 < (1L << 31), "%s: n >= 1 and b * n * 3 < 2^31 expected, got b = %d, n = %d", who, b, n);
    VS_REQUIRE(bb >= 1 && bb <= LOSS_MAXBOX, "%s: 1 to %d boxes per scene, got bb = %d", who, LOSS_MAXBOX, bb);
    return VOTENET_OK;
}

extern "C" int votenet_vote_targets(int b, int n, int bb, const float *seeds, const float *xyz, const float *lwh, const float *roty,
                                    int *slots, int *inside_count, void *stream)
{
    if (int rc = check_shape("vote_targets", b, n, bb)) return rc;
    VS_REQUIRE(seeds && xyz && lwh && roty && slots && inside_count, "vote_targets: null buffer");
    hipLaunchKernelGGL(vote_targets_kernel, dim3((n + VS_TILE - 1) / VS_TILE, b), dim3(VS_THREADS), 0, as_stream(stream), n, bb, seeds,
                       xyz, lwh, roty, slots, inside_count);
    return g_vs_err.check_launch("vote_targets");
}

extern "C" int votenet_paper_vote_loss(int b, int n, int bb, const float *seeds, const float *votes, const float *xyz, const float *lwh,
                                       const float *roty, float *losses, float *d_votes, int *supervised, void *workspace, void *stream)
{
    if (int rc = check_shape("paper_vote_loss", b, n, bb)) return rc;
    VS_REQUIRE(seeds && votes && xyz && lwh && roty && losses && d_votes && workspace, "paper_vote_loss: null buffer");
    const size_t bytes = (size_t)b * n * 3 * sizeof(float);
    const uintptr_t src = reinterpret_cast<uintptr_t>(votes), dst = reinterpret_cast<uintptr_t>(d_votes);
    VS_REQUIRE(dst + bytes <= src || src + bytes <= dst, "paper_vote_loss: d_votes may not overlap votes");
    VS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "paper_vote_loss: the workspace must be 4-byte aligned");
    VoteLossArgs a = {b, n, bb, seeds, votes, xyz, lwh, roty, losses, d_votes, supervised, static_cast<int *>(workspace)};
    hipLaunchKernelGGL(paper_vote_loss_kernel, dim3(b), dim3(VS_THREADS), 0, as_stream(stream), a);
    return g_vs_err.check_launch("paper_vote_loss");
}
