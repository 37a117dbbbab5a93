// proposal_supervision.hip -- libvotenet_propsup.so (include/votenet_proposal_supervision.h), a library of its own beside
// libvotenet_hip.so (whose export list and whose votenet_loss stay what they were): the objectness and centre supervision of the VoteNet
// paper.
//   votenet_proposal_targets      label, nearest real box, every real box's nearest predicted centre, the real-box count of every scene.
//                                 proposal_targets_kernel: a workgroup per scene.
//   votenet_paper_proposal_loss   the two terms, their cotangents and the re-formed box loss and total, one launch behind votenet_loss.
//                                 paper_proposal_loss_kernel: a workgroup per scene.
// Both keep one proposal per lane in registers over the box loop (64 * ceil(p / 64) lanes, p <= 1024); the scene's box centres are staged
// once in LDS and read wave-uniformly.  The dual minimum over the proposals is a wave64 butterfly on (q, i) that prefers the smaller i on
// equal q, then a fold over the waves in order; a lane then gathers the dual terms it won in ascending box order -- no scatter, no float
// atomic.  The rule of the header is plain fp32 arithmetic in a fixed order (-ffp-contract=off, as everywhere in this project):
// tests/proposal_supervision_ref.py restates it in numpy float32 and decisions and centre cotangents are compared exactly.
#include "../common.h"
#include "../error_text.h"
#include "../nearest_box.h" // nearest_box, LOSS_MAXBOX: the labels are votenet_loss's, decided with the same instructions
#include "../scene_fold.h"

#pragma GCC visibility push(default)
#include "../../../include/votenet_proposal_supervision.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_propsup_last_error()) ----
static thread_local ErrorText g_ps_err;
#define PS_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_ps_err, cond, __VA_ARGS__)

constexpr int PS_MAX_B = 65535;          // scenes: a grid extent
constexpr int PS_MAX_P = 1024;           // proposals per scene: one per lane of one workgroup
constexpr int PS_WAVES = PS_MAX_P / 64;
constexpr int PS_MAXC = 32;              // nh, ns, nc <= 32, as votenet_loss
constexpr int PS_SUMS = 3;               // per scene (scene_fold.h): sum of w * ce, sum of e_i over the positives, sum of f_j over the real boxes
constexpr float PS_W0 = 0.2f, PS_W1 = 0.8f;

struct SceneLds {
    float box[LOSS_MAXBOX][8];       // [j][0..2]: the centre of box row j (the row layout nearest_box reads)
    float wq[PS_WAVES][LOSS_MAXBOX]; // a wave's minimum of q_ij over its lanes ...
    int wi[PS_WAVES][LOSS_MAXBOX];   // ... and the smallest i that attains it
    float q0[LOSS_MAXBOX];           // q_0j as proposal 0 formed it: a NaN there sticks
    float fq[LOSS_MAXBOX];           // f_j
    int fi[LOSS_MAXBOX];             // i2(j)
    int last;                        // the last row whose centre differs from the row before it: g_s = last + 1
};

// Scene `sc`'s box centres into LDS.  The caller's barrier follows.
__device__ __forceinline__ void stage_scene(SceneLds &S, int bb, const float *__restrict__ gxyz, int tid, int nt)
{
    for (int j = tid; j < bb; j += nt) {
        S.box[j][0] = gxyz[j * 3 + 0];
        S.box[j][1] = gxyz[j * 3 + 1];
        S.box[j][2] = gxyz[j * 3 + 2];
    }
    if (tid == 0) S.last = 0;
}
// The real boxes of the staged scene: trailing rows equal to their predecessor (three ==) are padding.  An integer maximum in LDS; the
// caller's barrier follows.
__device__ __forceinline__ void mark_real(SceneLds &S, int bb, int tid, int nt)
{
    for (int j = tid + 1; j < bb; j += nt)
        if (!(S.box[j][0] == S.box[j - 1][0] && S.box[j][1] == S.box[j - 1][1] && S.box[j][2] == S.box[j - 1][2])) atomicMax(&S.last, j);
}

// Over the real boxes of the staged scene, for the predicted centre (cx, cy, cz) of proposal i = tid (live: i < p): the lane's own first
// minimum e at j1 (nearest_box.h's idiom: a NaN in the first candidate sticks), and per box the wave's minimum over its lanes into
// wq / wi.  In the butterfly a NaN never wins (it takes part as +inf with its index, so the smaller index still wins among equals) --
// the sequential rule `first || q < best` over ascending i, where only proposal 0's NaN can stick: fold_dual puts that case back.
__device__ __forceinline__ void scan_real_boxes(SceneLds &S, int g, int tid, bool live, float cx, float cy, float cz, float &e, int &j1)
{
    const int wave = tid >> 6;
    e = 0.0f;
    j1 = 0;
    for (int j = 0; j < g; j++) {
        const float dx = cx - S.box[j][0], dy = cy - S.box[j][1], dz = cz - S.box[j][2];
        const float q = (dx * dx + dy * dy) + dz * dz;
        if (j == 0 || q < e) {
            e = q;
            j1 = j;
        }
        if (tid == 0) S.q0[j] = q;
        float bq = live && q == q ? q : INFINITY;
        int bi = live ? tid : 0x7FFFFFFF;
        for (int off = 32; off > 0; off >>= 1) {
            const float oq = __shfl_xor(bq, off);
            const int oi = __shfl_xor(bi, off);
            if (oq < bq || (oq == bq && oi < bi)) {
                bq = oq;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            S.wq[wave][j] = bq;
            S.wi[wave][j] = bi;
        }
    }
}
// Behind a barrier: the waves' minima in wave order (ascending i: a later wave wins only with a smaller q) -> f_j, i2(j).
__device__ __forceinline__ void fold_dual(SceneLds &S, int g, int tid, int nt)
{
    const int nwaves = nt >> 6;
    for (int j = tid; j < g; j += nt) {
        float bq = S.wq[0][j];
        int bi = S.wi[0][j];
        for (int w = 1; w < nwaves; w++)
            if (S.wq[w][j] < bq) {
                bq = S.wq[w][j];
                bi = S.wi[w][j];
            }
        const float q0 = S.q0[j];
        if (q0 != q0) { // the first candidate is a NaN: it sticks
            bq = q0;
            bi = 0;
        }
        S.fq[j] = bq;
        S.fi[j] = bi;
    }
}

__global__ __launch_bounds__(PS_MAX_P) void proposal_targets_kernel(int p, int bb, const float *__restrict__ pxyz,
                                                                    const float *__restrict__ pout, long pitch,
                                                                    const float *__restrict__ gxyz, float pos_thr, float neg_thr,
                                                                    int *__restrict__ label, int *__restrict__ near_box,
                                                                    int *__restrict__ dual_prop, int *__restrict__ real_boxes)
{
    __shared__ SceneLds S;
    const int tid = threadIdx.x, nt = blockDim.x, sc = blockIdx.x;
    const bool live = tid < p;
    stage_scene(S, bb, gxyz + (size_t)sc * bb * 3, tid, nt);
    __syncthreads();
    mark_real(S, bb, tid, nt);
    const float nan = __builtin_nanf("");
    float cx = nan, cy = nan, cz = nan;
    bool pos = false, neg = false;
    if (live) {
        const size_t q = (size_t)sc * p + tid;
        const float px = pxyz[q * 3 + 0], py = pxyz[q * 3 + 1], pz = pxyz[q * 3 + 2];
        int gi;
        const float dmin = nearest_box(S.box, bb, px, py, pz, gi);
        pos = dmin < pos_thr;
        neg = dmin > neg_thr;
        const float *o = pout + q * (size_t)pitch;
        cx = px + o[2];
        cy = py + o[3];
        cz = pz + o[4];
    }
    __syncthreads();
    const int g = S.last + 1;
    float e;
    int j1;
    scan_real_boxes(S, g, tid, live, cx, cy, cz, e, j1);
    __syncthreads();
    fold_dual(S, g, tid, nt);
    __syncthreads();
    if (live) {
        label[(size_t)sc * p + tid] = pos ? 1 : (neg ? 0 : -1);
        near_box[(size_t)sc * p + tid] = pos ? j1 : -1;
    }
    for (int j = tid; j < bb; j += nt) dual_prop[(size_t)sc * bb + j] = j < g ? S.fi[j] : -1;
    if (tid == 0) real_boxes[sc] = g;
}

struct PropLossArgs {
    int b, p, bb, width;
    const float *pxyz, *pout;
    long pitch;
    const float *gxyz;
    float pos_thr, neg_thr;
    float *losses, *d_pxyz, *d_pout;
    int *counts;
    int *ticket; // the workspace of scene_fold (PS_SUMS sums per scene): zero on entry, left zero
};

// One workgroup per scene.  Pass 1: Np, Nn and G of the WHOLE batch, counted by every workgroup for itself (b * p nearest_box calls over
// the lanes; integers, so every workgroup arrives at the same values whatever its order): no workgroup waits for another before it scales
// its cotangents.  The walk over the scenes ends with the workgroup's own, whose centres then stay in LDS and whose labels stay in the
// lanes.  Pass 2: the own scene's objectness, minima and cotangents.  The sums: lanes by wave shuffles, waves in order; the scenes' sums
// are folded in scene order by the last workgroup to finish.
__global__ __launch_bounds__(PS_MAX_P) void paper_proposal_loss_kernel(PropLossArgs A)
{
    __shared__ SceneLds S;
    __shared__ int s_cnt[PS_WAVES][2];
    __shared__ float s_sum[PS_WAVES][2];
    const int tid = threadIdx.x, nt = blockDim.x, nwaves = nt >> 6, own = blockIdx.x, B = A.b, P = A.p, BB = A.bb;
    const bool live = tid < P;
    const float nan = __builtin_nanf("");
    float px = nan, py = nan, pz = nan;
    bool pos = false, neg = false;
    int np = 0, nn = 0, G = 0;
    for (int t = 1; t <= B; t++) {
        const int sc = (own + t) % B;
        __syncthreads(); // the scene before this one has been read
        stage_scene(S, BB, A.gxyz + (size_t)sc * BB * 3, tid, nt);
        __syncthreads();
        mark_real(S, BB, tid, nt);
        if (live) {
            const size_t q = (size_t)sc * P + tid;
            px = A.pxyz[q * 3 + 0], py = A.pxyz[q * 3 + 1], pz = A.pxyz[q * 3 + 2];
            int gi;
            const float dmin = nearest_box(S.box, BB, px, py, pz, gi);
            pos = dmin < A.pos_thr;
            neg = dmin > A.neg_thr;
            np += pos;
            nn += neg;
        }
        __syncthreads();
        G += S.last + 1;
    }
    const int g = S.last + 1; // the own scene's
    for (int off = 32; off > 0; off >>= 1) {
        np += __shfl_down(np, off);
        nn += __shfl_down(nn, off);
    }
    if ((tid & 63) == 0) s_cnt[tid >> 6][0] = np, s_cnt[tid >> 6][1] = nn;
    __syncthreads();
    int Np = 0, Nn = 0;
    for (int w = 0; w < nwaves; w++) Np += s_cnt[w][0], Nn += s_cnt[w][1];
    const float inv_m = 1.0f / ((float)(Np + Nn) + 1e-6f), inv_p = 1.0f / ((float)Np + 1e-6f), inv_g = 1.0f / ((float)G + 1e-6f);
    // ---- pass 2: the own scene (its centres are the ones in LDS; px, py, pz, pos, neg are the own scene's)
    float cx = nan, cy = nan, cz = nan, go0 = 0.0f, go1 = 0.0f, obj = 0.0f;
    if (live) {
        const float *o = A.pout + ((size_t)own * P + tid) * (size_t)A.pitch;
        cx = px + o[2];
        cy = py + o[3];
        cz = pz + o[4];
        if (pos || neg) {
            const float o0 = o[0], o1 = o[1];
            const float mx = fmaxf(o0, o1);
            const float e0 = expf(o0 - mx), e1 = expf(o1 - mx);
            const float s = e0 + e1;
            const float lse = mx + logf(s);
            const float w = pos ? PS_W1 : PS_W0;
            obj = w * (lse - (pos ? o1 : o0));
            const float r = 1.0f / s;
            go0 = ((0.5f * w) * (e0 * r - (pos ? 0.0f : 1.0f))) * inv_m;
            go1 = ((0.5f * w) * (e1 * r - (pos ? 1.0f : 0.0f))) * inv_m;
        }
    }
    float e;
    int j1;
    scan_real_boxes(S, g, tid, live, cx, cy, cz, e, j1);
    __syncthreads();
    fold_dual(S, g, tid, nt);
    __syncthreads();
    if (live) {
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        if (pos) {
            d0 = (2.0f * (cx - S.box[j1][0])) * inv_p;
            d1 = (2.0f * (cy - S.box[j1][1])) * inv_p;
            d2 = (2.0f * (cz - S.box[j1][2])) * inv_p;
        }
        for (int j = 0; j < g; j++) // the dual terms this proposal won, in ascending box order
            if (S.fi[j] == tid) {
                d0 += (2.0f * (cx - S.box[j][0])) * inv_g;
                d1 += (2.0f * (cy - S.box[j][1])) * inv_g;
                d2 += (2.0f * (cz - S.box[j][2])) * inv_g;
            }
        const size_t q = (size_t)own * P + tid;
        float *go = A.d_pout + q * (size_t)A.width;
        go[0] = go0;
        go[1] = go1;
        go[2] = d0;
        go[3] = d1;
        go[4] = d2;
        A.d_pxyz[q * 3 + 0] = d0;
        A.d_pxyz[q * 3 + 1] = d1;
        A.d_pxyz[q * 3 + 2] = d2;
    }
    // ---- the scene's three sums: lanes -> waves -> (thread 0) waves in order; the f_j by wave 0, ascending j inside a lane
    float esum = pos ? e : 0.0f, fsum = 0.0f;
    if (tid < 64)
        for (int j = tid; j < g; j += 64) fsum += S.fq[j];
    for (int off = 32; off > 0; off >>= 1) {
        obj += __shfl_down(obj, off);
        esum += __shfl_down(esum, off);
        fsum += __shfl_down(fsum, off); // (wave 0's is the one read)
    }
    if ((tid & 63) == 0) s_sum[tid >> 6][0] = obj, s_sum[tid >> 6][1] = esum;
    __syncthreads();
    if (tid != 0) return;
    float v[PS_SUMS] = {0.0f, 0.0f, fsum}, t[PS_SUMS];
    for (int w = 0; w < nwaves; w++) v[0] += s_sum[w][0], v[1] += s_sum[w][1];
    if (!scene_fold(A.ticket, own, B, v, t)) return;
    float *L = A.losses;
    const float objl = t[0] * inv_m;
    const float center = t[1] * inv_p + t[2] * inv_g;
    const float box = center + 0.1f * L[4] + L[5] + 0.1f * L[6] + L[7]; // votenet_loss's box loss and total (loss.hip), from the
    L[0] = L[1] + 0.5f * objl + box + 0.1f * L[8];                      // components it stored
    L[2] = objl;
    L[3] = center;
    L[9] = box;
    if (A.counts) A.counts[0] = Np, A.counts[1] = Nn, A.counts[2] = G;
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_propsup_last_error(void) { return g_ps_err.text; }

extern "C" size_t votenet_propsup_workspace_bytes(int b) { return scene_fold_bytes(b, PS_SUMS); }

static int check_shape(const char *who, int b, int p, int bb)
{
    PS_REQUIRE(b >= 1 && b <= PS_MAX_B, "%s: 1 to %d scenes, got b = %d", who, PS_MAX_B, b);
    PS_REQUIRE(p >= 1 && p <= PS_MAX_P, "%s: 1 to %d proposals per scene, got p = %d", who, PS_MAX_P, p);
    PS_REQUIRE(bb >= 1 && bb <= LOSS_MAXBOX, "%s: 1 to %d boxes per scene, got bb = %d", who, LOSS_MAXBOX, bb);
    return VOTENET_OK;
}

static bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return !(x + abytes <= y || y + bbytes <= x);
}

extern "C" int votenet_proposal_targets(int b, int p, int bb, const float *proposals_xyz, const float *proposals_output,
                                        long output_pitch, const float *bboxes_xyz, float pos_thr, float neg_thr, int *label,
                                        int *near_box, int *dual_prop, int *real_boxes, void *stream)
{
    if (int rc = check_shape("proposal_targets", b, p, bb)) return rc;
    PS_REQUIRE(output_pitch >= 5, "proposal_targets: the pitch of proposals_output (%ld) is smaller than the five columns read", output_pitch);
    PS_REQUIRE(pos_thr < neg_thr, "proposal_targets: pos_thr < neg_thr expected, as votenet_loss");
    PS_REQUIRE(proposals_xyz && proposals_output && bboxes_xyz && label && near_box && dual_prop && real_boxes,
               "proposal_targets: null buffer");
    hipLaunchKernelGGL(proposal_targets_kernel, dim3(b), dim3((p + 63) / 64 * 64), 0, as_stream(stream), p, bb, proposals_xyz,
                       proposals_output, output_pitch, bboxes_xyz, pos_thr, neg_thr, label, near_box, dual_prop, real_boxes);
    return g_ps_err.check_launch("proposal_targets");
}

extern "C" int votenet_paper_proposal_loss(int b, int p, int bb, int nh, int ns, int nc, const float *proposals_xyz,
                                           const float *proposals_output, long output_pitch, const float *bboxes_xyz, float pos_thr,
                                           float neg_thr, float *losses, float *d_proposals_xyz, float *d_proposals_output, int *counts,
                                           void *workspace, void *stream)
{
    if (int rc = check_shape("paper_proposal_loss", b, p, bb)) return rc;
    PS_REQUIRE(nh > 0 && ns > 0 && nc > 0 && nh <= PS_MAXC && ns <= PS_MAXC && nc <= PS_MAXC,
               "paper_proposal_loss: 0 < nh, ns, nc <= %d expected, got %d, %d, %d", PS_MAXC, nh, ns, nc);
    const int width = 5 + 2 * nh + 4 * ns + nc;
    PS_REQUIRE(output_pitch >= width, "paper_proposal_loss: the pitch of proposals_output (%ld) is smaller than its width (%d)",
               output_pitch, width);
    PS_REQUIRE(pos_thr < neg_thr, "paper_proposal_loss: pos_thr < neg_thr expected, as votenet_loss");
    PS_REQUIRE(proposals_xyz && proposals_output && bboxes_xyz && losses && d_proposals_xyz && d_proposals_output && workspace,
               "paper_proposal_loss: null buffer");
    const size_t rows = (size_t)b * p;
    PS_REQUIRE(!overlap(d_proposals_xyz, rows * 3 * sizeof(float), proposals_xyz, rows * 3 * sizeof(float)),
               "paper_proposal_loss: d_proposals_xyz may not overlap proposals_xyz");
    PS_REQUIRE(!overlap(d_proposals_output, rows * width * sizeof(float), proposals_output,
                        ((rows - 1) * (size_t)output_pitch + width) * sizeof(float)),
               "paper_proposal_loss: d_proposals_output may not overlap proposals_output");
    PS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "paper_proposal_loss: the workspace must be 4-byte aligned");
    PropLossArgs a = {b, p, bb, width, proposals_xyz, proposals_output, output_pitch, bboxes_xyz, pos_thr, neg_thr, losses,
                      d_proposals_xyz, d_proposals_output, counts, static_cast<int *>(workspace)};
    hipLaunchKernelGGL(paper_proposal_loss_kernel, dim3(b), dim3((p + 63) / 64 * 64), 0, as_stream(stream), a);
    return g_ps_err.check_launch("paper_proposal_loss");
}
