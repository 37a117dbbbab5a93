// box_points.hip -- libvotenet_boxpts.so (include/votenet_box_points.h), a library of its own beside libvotenet_hip.so and
// libvotenet_detect.so (whose export lists stay what they were): the `remove_empty_box` step of the VoteNet paper's protocol.
//   votenet_box_point_counts   the points of each scene inside each of its predicted boxes.  box_point_counts_kernel: a workgroup per
//                              (point tile, scene), every lane keeps its points in registers over the whole box loop.
//   votenet_gate_objectness    a copy of the objectness logits with the boxes below min_points set to NaN: no candidate of either NMS.
// The rule of the header is plain fp32 arithmetic in a fixed order (-ffp-contract=off, as everywhere in this project):
// tests/box_points_ref.py restates it in numpy float32 and the counts are compared exactly.
#include "../common.h"
#include "../error_text.h"

#include <cstdint>
#pragma GCC visibility push(default)
#include "../../../include/votenet_box_points.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_box_points_last_error()) ----
static thread_local ErrorText g_bp_err;
#define BP_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_bp_err, cond, __VA_ARGS__)

constexpr int BP_MAX_B = 65535;       // scenes: the grid's y extent
constexpr int BP_MAX_N = 1024;
constexpr long BP_MAX_NPTS = 1L << 24; // exclusive
constexpr int BP_THREADS = 128;       // two waves
constexpr int BP_PPT = 4;             // points a lane keeps in registers
constexpr int BP_TILE = BP_THREADS * BP_PPT; // 512 points per workgroup: 8 x 20 480 points are 320 workgroups
constexpr int BP_CHUNK = BP_THREADS;  // boxes whose constants sit in LDS at a time: one thread forms one box's

// A workgroup per (tile of BP_TILE points, scene).  Lane l of wave w holds points tile * BP_TILE + k * BP_THREADS + tid, k < BP_PPT
// (coalesced rows); a point beyond npts is NaN and counts nothing, as a hole point does.
// Per chunk of BP_CHUNK boxes: thread t forms the 15 constants of box t (c0, e_0..e_2, ee_0..ee_2) into LDS, once per box and
// workgroup.  Then every wave walks the chunk: the constants are read wave-uniformly (four 16-byte broadcasts), the wave's count of
// box j is the sum over its BP_PPT point slots of popcount(ballot(inside)), kept in lane j mod 64; after 64 boxes the wave adds its 64
// counts to counts[scene][j0 .. j0 + 64) with one contiguous integer atomic instruction (lanes with nothing to add stay out).
// No workgroup waits for another; counts was zeroed on the stream before the launch.
__global__ __launch_bounds__(BP_THREADS) void box_point_counts_kernel(int n, long npts, const float *__restrict__ bboxes,
                                                                      const float *__restrict__ points, int *__restrict__ counts)
{
    __shared__ float4 s_box[BP_CHUNK][4]; // {c0, ee_0}, {e_0, ee_1}, {e_1, ee_2}, {e_2, -}
    const int scene = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const float nan = __builtin_nanf("");
    float px[BP_PPT], py[BP_PPT], pz[BP_PPT];
    const float *__restrict__ pts = points + (size_t)scene * (size_t)npts * 3;
#pragma unroll
    for (int k = 0; k < BP_PPT; k++) {
        const long p = (long)blockIdx.x * BP_TILE + k * BP_THREADS + tid;
        const bool live = p < npts;
        px[k] = live ? pts[(size_t)p * 3 + 0] : nan;
        py[k] = live ? pts[(size_t)p * 3 + 1] : nan;
        pz[k] = live ? pts[(size_t)p * 3 + 2] : nan;
    }
    const float *__restrict__ boxes = bboxes + (size_t)scene * n * 24;
    int *__restrict__ out = counts + (size_t)scene * n;
    for (int base = 0; base < n; base += BP_CHUNK) {
        const int cnt = n - base < BP_CHUNK ? n - base : BP_CHUNK;
        __syncthreads(); // the chunk before this one has been read
        if (tid < cnt) {
            const float *__restrict__ c = boxes + (size_t)(base + tid) * 24;
            const float c0x = c[0], c0y = c[1], c0z = c[2];
            const float e0x = c[3] - c0x, e0y = c[4] - c0y, e0z = c[5] - c0z;    // corner 1: the width axis
            const float e1x = c[9] - c0x, e1y = c[10] - c0y, e1z = c[11] - c0z;  // corner 3: the length axis
            const float e2x = c[12] - c0x, e2y = c[13] - c0y, e2z = c[14] - c0z; // corner 4: the height axis
            const float ee0 = (e0x * e0x + e0y * e0y) + e0z * e0z;
            const float ee1 = (e1x * e1x + e1y * e1y) + e1z * e1z;
            const float ee2 = (e2x * e2x + e2y * e2y) + e2z * e2z;
            s_box[tid][0] = make_float4(c0x, c0y, c0z, ee0);
            s_box[tid][1] = make_float4(e0x, e0y, e0z, ee1);
            s_box[tid][2] = make_float4(e1x, e1y, e1z, ee2);
            s_box[tid][3] = make_float4(e2x, e2y, e2z, 0.0f);
        }
        __syncthreads();
        for (int g = 0; g < cnt; g += 64) {
            const int m = cnt - g < 64 ? cnt - g : 64;
            int acc = 0;
            for (int jj = 0; jj < m; jj++) {
                const float4 a0 = s_box[g + jj][0], a1 = s_box[g + jj][1], a2 = s_box[g + jj][2], a3 = s_box[g + jj][3];
                int c = 0; // wave-uniform
#pragma unroll
                for (int k = 0; k < BP_PPT; k++) {
                    const float qx = px[k] - a0.x, qy = py[k] - a0.y, qz = pz[k] - a0.z;
                    const float t0 = (qx * a1.x + qy * a1.y) + qz * a1.z;
                    const float t1 = (qx * a2.x + qy * a2.y) + qz * a2.z;
                    const float t2 = (qx * a3.x + qy * a3.y) + qz * a3.z;
                    const bool inside = t0 >= 0.0f && t0 <= a0.w && t1 >= 0.0f && t1 <= a1.w && t2 >= 0.0f && t2 <= a2.w;
                    c += __popcll(__ballot(inside));
                }
                acc = lane == jj ? c : acc;
            }
            if (lane < m && acc != 0) atomicAdd(out + base + g + lane, acc);
        }
    }
}

__global__ __launch_bounds__(256) void gate_objectness_kernel(int total, const int *__restrict__ counts, int min_points,
                                                              const uint2 *__restrict__ objectness, uint2 *__restrict__ gated)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint2 o = objectness[i]; // the bits: a copy, whatever they hold
    gated[i] = counts[i] >= min_points ? o : make_uint2(0x7fc00000u, 0x7fc00000u);
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_box_points_last_error(void) { return g_bp_err.text; }

extern "C" int votenet_box_point_counts(int b, int n, long npts, const float *bboxes, const float *points, int *counts, void *stream)
{
    BP_REQUIRE(b >= 0 && b <= BP_MAX_B, "box_point_counts: batch must be in [0, %d], got %d", BP_MAX_B, b);
    BP_REQUIRE(n >= 1 && n <= BP_MAX_N, "box_point_counts: 1 to %d boxes per scene, got n = %d", BP_MAX_N, n);
    BP_REQUIRE(npts >= 0 && npts < BP_MAX_NPTS, "box_point_counts: points per scene must be in [0, 2^24), got npts = %ld", npts);
    if (b == 0) return VOTENET_OK;
    BP_REQUIRE(bboxes && counts, "box_point_counts: null boxes or counts");
    BP_REQUIRE(points || npts == 0, "box_point_counts: null points");
    hipStream_t st = as_stream(stream);
    int rc = g_bp_err.check(hipMemsetAsync(counts, 0, (size_t)b * n * sizeof(int), st), "box_point_counts (memset)");
    if (rc != VOTENET_OK || npts == 0) return rc;
    const unsigned tiles = (unsigned)((npts + BP_TILE - 1) / BP_TILE); // < 2^15
    hipLaunchKernelGGL(box_point_counts_kernel, dim3(tiles, b), dim3(BP_THREADS), 0, st, n, npts, bboxes, points, counts);
    return g_bp_err.check_launch("box_point_counts");
}

extern "C" int votenet_gate_objectness(int b, int n, const int *counts, int min_points, const float *objectness, float *gated,
                                       void *stream)
{
    BP_REQUIRE(b >= 0 && b <= BP_MAX_B, "gate_objectness: batch must be in [0, %d], got %d", BP_MAX_B, b);
    BP_REQUIRE(n >= 1 && n <= BP_MAX_N, "gate_objectness: 1 to %d boxes per scene, got n = %d", BP_MAX_N, n);
    BP_REQUIRE(min_points >= 0, "gate_objectness: min_points must be >= 0, got %d", min_points);
    if (b == 0) return VOTENET_OK;
    BP_REQUIRE(counts && objectness && gated, "gate_objectness: null counts, objectness or gated");
    const size_t bytes = (size_t)b * n * 2 * sizeof(float);
    const uintptr_t src = reinterpret_cast<uintptr_t>(objectness), dst = reinterpret_cast<uintptr_t>(gated);
    BP_REQUIRE(dst + bytes <= src || src + bytes <= dst, "gate_objectness: gated may not alias objectness");
    BP_REQUIRE(src % 8 == 0 && dst % 8 == 0, "gate_objectness: objectness and gated must be 8-byte aligned");
    const int total = b * n; // <= 65535 * 1024 < 2^31
    hipLaunchKernelGGL(gate_objectness_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), total, counts, min_points,
                       (const uint2 *)objectness, (uint2 *)gated);
    return g_bp_err.check_launch("gate_objectness");
}
