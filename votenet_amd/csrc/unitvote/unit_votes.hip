// unit_votes.hip -- libvotenet_unitvote.so (include/votenet_unit_votes.h), a library of its own beside libvotenet_hip.so (whose export
// list and whose glue entries stay what they were): the vote features divided by their L2 norm, as the authors' VoteNet does.
//   votenet_unit_votes            votes_xyz = x + off, votes_points = u / |u| with u = x[3:] + off[3:], norm = |u|, in ONE launch, in
//                                 the place of the votenet_row_segments launch that forms votes_xyz and u.   unit_votes_kernel
//   votenet_unit_votes_backward   d_votes = [d_xyz (+ cot_xyz) | (g - y (y . g)) / norm | 0] in ONE launch, in the place of the
//                                 votenet_row_segments launch that forms [d_xyz (+ cot_xyz) | g | 0].       unit_votes_backward_kernel
// The votes exist only in the middle of a step's static stretch, a chain of small launches: both kernels are launch- and latency-bound
// (25 MB / 34 MB at 8192 rows x 256 channels), so each is shaped for the shortest dependent chain, not for bandwidth: a wave per row,
// four rows per workgroup, lane l owns channels l, l + 64, ...: every load and store instruction of a wave covers 64 contiguous dwords
// (the operands start at element 3 of a row and a pitch may be odd, so nothing wider than a dword is aligned).  NCH = c / 64 is a
// template parameter: the row's loads are all issued before the first use, none under a branch; the only branch is the row bound (and,
// in the backward, the store loop of a zero tail wider than 64 columns).  The sum over the row: NCH products per lane in ascending
// channel order, then an xor butterfly 32, 16, 8, 4, 2, 1 (__shfl_xor: no LDS allocation, every lane ends with the same bits).  No
// contraction (-ffp-contract=off) and no SLP packing (-fno-slp-vectorize): tests/unit_votes_ref.py restates the rule operation for
// operation.  sqrtf and / are the compiler's correctly rounded fp32 forms (its default for HIP; __fsqrt_rn is the NATIVE square root
// unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so it is not used); denormals are honoured.
#include "../common.h"
#include "../error_text.h"

#pragma GCC visibility push(default)
#include "../../../include/votenet_unit_votes.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_unitvote_last_error()) ----
static thread_local ErrorText g_uv_err;
#define UV_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_uv_err, cond, __VA_ARGS__)

constexpr int UV_MIN_C = 64, UV_MAX_C = 512;  // channels: 1 to 8 per lane
constexpr int UV_ROWS_PER_WG = 4;             // a wave per row
constexpr long UV_MAX_ROWS = (long)UV_ROWS_PER_WG * 2147483647L;

// The coordinate loads feed a store that only lanes 0..2 make: without this the compiler sinks them into that branch, behind every other
// load's use -- a second memory latency in a kernel that is nothing but latency.  An empty statement that "uses" both values keeps the
// loads where they are written, first in the row's batch (loads return in order: waiting for the oldest two costs nothing).
#define UV_KEEP_LOADED(a, b) asm volatile("" : "+v"(a), "+v"(b))

// p + p_partner over the xor butterfly 32, 16, 8, 4, 2, 1: all 64 lanes take part (the row bound is uniform in a wave)
__device__ __forceinline__ float uv_butterfly(float p)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s, 64);
    return p;
}

template <int NCH>
__global__ __launch_bounds__(UV_ROWS_PER_WG * 64) void unit_votes_kernel(long rows, const float *__restrict__ x, long x_pitch,
                                                                          const float *__restrict__ off, long off_pitch,
                                                                          float *__restrict__ votes_xyz, float *__restrict__ votes_points,
                                                                          float *__restrict__ norm)
{
    const int lane = lane_id();
    const long row = (long)blockIdx.x * UV_ROWS_PER_WG + wave_id_uniform();
    if (row >= rows) return;
    const float *__restrict__ xr = x + row * x_pitch;
    const float *__restrict__ fr = off + row * off_pitch;
    const int k3 = lane < 3 ? lane : 0; // every lane loads a coordinate (in bounds), lanes 0..2 store theirs
    float xa = xr[k3], xb = fr[k3];
    float a[NCH], b[NCH];
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        a[i] = xr[3 + i * 64 + lane];
        b[i] = fr[3 + i * 64 + lane];
    }
    UV_KEEP_LOADED(xa, xb);
    if (lane < 3) votes_xyz[row * 3 + lane] = xa + xb;
    float u[NCH];
#pragma unroll
    for (int i = 0; i < NCH; i++) u[i] = a[i] + b[i];
    float p = u[0] * u[0];
#pragma unroll
    for (int i = 1; i < NCH; i++) p = p + u[i] * u[i];
    p = uv_butterfly(p);
    const float nrm = sqrtf(p);
    float *__restrict__ yr = votes_points + row * (long)(NCH * 64);
#pragma unroll
    for (int i = 0; i < NCH; i++) yr[i * 64 + lane] = u[i] / nrm;
    if (lane == 0) norm[row] = nrm;
}

template <int NCH, bool COT>
__global__ __launch_bounds__(UV_ROWS_PER_WG * 64) void unit_votes_backward_kernel(long rows, const float *__restrict__ d_xyz,
                                                                                   const float *__restrict__ cot_xyz,
                                                                                   const float *__restrict__ d_points,
                                                                                   const float *__restrict__ votes_points,
                                                                                   const float *__restrict__ norm, float *__restrict__ d_votes,
                                                                                   long d_pitch, int d_width)
{
    constexpr int C = NCH * 64;
    const int lane = lane_id();
    const long row = (long)blockIdx.x * UV_ROWS_PER_WG + wave_id_uniform();
    if (row >= rows) return;
    const int k3 = lane < 3 ? lane : 0;
    float da = d_xyz[row * 3 + k3], db = 0.0f;
    if constexpr (COT) db = cot_xyz[row * 3 + k3];
    const float nrm = norm[row];
    const float *__restrict__ yr = votes_points + row * (long)C;
    const float *__restrict__ gr = d_points + row * (long)C;
    float y[NCH], g[NCH];
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        y[i] = yr[i * 64 + lane];
        g[i] = gr[i * 64 + lane];
    }
    UV_KEEP_LOADED(da, db);
    float *__restrict__ dr = d_votes + row * d_pitch;
    if (lane < 3) dr[lane] = COT ? da + db : da;
    float q = y[0] * g[0];
#pragma unroll
    for (int i = 1; i < NCH; i++) q = q + y[i] * g[i];
    const float dot = uv_butterfly(q);
#pragma unroll
    for (int i = 0; i < NCH; i++) dr[3 + i * 64 + lane] = (g[i] - y[i] * dot) / nrm;
    for (long j = 3 + C + lane; j < d_width; j += 64) dr[j] = 0.0f; // the zero tail of a padded layer (29 columns in the model: one store)
}

template <int NCH>
static void uv_launch_forward(dim3 grid, hipStream_t st, long rows, const float *x, long x_pitch, const float *off, long off_pitch,
                              float *votes_xyz, float *votes_points, float *norm)
{
    hipLaunchKernelGGL((unit_votes_kernel<NCH>), grid, dim3(UV_ROWS_PER_WG * 64), 0, st, rows, x, x_pitch, off, off_pitch, votes_xyz,
                       votes_points, norm);
}

template <int NCH>
static void uv_launch_backward(dim3 grid, hipStream_t st, long rows, const float *d_xyz, const float *cot_xyz, const float *d_points,
                               const float *votes_points, const float *norm, float *d_votes, long d_pitch, int d_width)
{
    if (cot_xyz)
        hipLaunchKernelGGL((unit_votes_backward_kernel<NCH, true>), grid, dim3(UV_ROWS_PER_WG * 64), 0, st, rows, d_xyz, cot_xyz, d_points,
                           votes_points, norm, d_votes, d_pitch, d_width);
    else
        hipLaunchKernelGGL((unit_votes_backward_kernel<NCH, false>), grid, dim3(UV_ROWS_PER_WG * 64), 0, st, rows, d_xyz, cot_xyz, d_points,
                           votes_points, norm, d_votes, d_pitch, d_width);
}

// `CALL(NCH)` for the NCH = c / 64 of a checked c
#define UV_DISPATCH(c, CALL) \
    switch ((c) / 64) {      \
    case 1: CALL(1); break;  \
    case 2: CALL(2); break;  \
    case 3: CALL(3); break;  \
    case 4: CALL(4); break;  \
    case 5: CALL(5); break;  \
    case 6: CALL(6); break;  \
    case 7: CALL(7); break;  \
    default: CALL(8); break; \
    }

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_unitvote_last_error(void) { return g_uv_err.text; }

extern "C" int votenet_unit_votes(long rows, int c, const float *x, long x_pitch, const float *off, long off_pitch, float *votes_xyz,
                                  float *votes_points, float *norm, void *stream)
{
    UV_REQUIRE(rows >= 0 && rows <= UV_MAX_ROWS, "unit_votes: 0 to %ld rows expected, got rows = %ld", UV_MAX_ROWS, rows);
    UV_REQUIRE(c >= UV_MIN_C && c <= UV_MAX_C && c % 64 == 0, "unit_votes: %d to %d channels in multiples of 64 expected, got c = %d",
               UV_MIN_C, UV_MAX_C, c);
    UV_REQUIRE(x_pitch >= 3 + c && off_pitch >= 3 + c, "unit_votes: row pitches of at least 3 + c = %d elements expected, got x_pitch = %ld, "
               "off_pitch = %ld", 3 + c, x_pitch, off_pitch);
    if (rows == 0) return VOTENET_OK;
    UV_REQUIRE(x && off && votes_xyz && votes_points && norm, "unit_votes: null buffer");
    const dim3 grid((unsigned)((rows + UV_ROWS_PER_WG - 1) / UV_ROWS_PER_WG));
    hipStream_t st = as_stream(stream);
#define UV_FWD(N) uv_launch_forward<N>(grid, st, rows, x, x_pitch, off, off_pitch, votes_xyz, votes_points, norm)
    UV_DISPATCH(c, UV_FWD);
#undef UV_FWD
    return g_uv_err.check_launch("unit_votes");
}

extern "C" int votenet_unit_votes_backward(long rows, int c, const float *d_xyz, const float *cot_xyz, const float *d_points,
                                           const float *votes_points, const float *norm, float *d_votes, long d_pitch, int d_width,
                                           void *stream)
{
    UV_REQUIRE(rows >= 0 && rows <= UV_MAX_ROWS, "unit_votes_backward: 0 to %ld rows expected, got rows = %ld", UV_MAX_ROWS, rows);
    UV_REQUIRE(c >= UV_MIN_C && c <= UV_MAX_C && c % 64 == 0,
               "unit_votes_backward: %d to %d channels in multiples of 64 expected, got c = %d", UV_MIN_C, UV_MAX_C, c);
    UV_REQUIRE(d_width >= 3 + c, "unit_votes_backward: d_width of at least 3 + c = %d columns expected, got d_width = %d", 3 + c, d_width);
    UV_REQUIRE(d_pitch >= d_width, "unit_votes_backward: a row pitch d_pitch >= d_width = %d elements expected, got d_pitch = %ld", d_width,
               d_pitch);
    if (rows == 0) return VOTENET_OK;
    UV_REQUIRE(d_xyz && d_points && votes_points && norm && d_votes, "unit_votes_backward: null buffer (only cot_xyz may be null)");
    const dim3 grid((unsigned)((rows + UV_ROWS_PER_WG - 1) / UV_ROWS_PER_WG));
    hipStream_t st = as_stream(stream);
#define UV_BWD(N) uv_launch_backward<N>(grid, st, rows, d_xyz, cot_xyz, d_points, votes_points, norm, d_votes, d_pitch, d_width)
    UV_DISPATCH(c, UV_BWD);
#undef UV_BWD
    return g_uv_err.check_launch("unit_votes_backward");
}
