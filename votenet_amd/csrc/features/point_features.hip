// point_features.hip -- libvotenet_features.so (include/votenet_point_features.h), a library of its own beside libvotenet_hip.so (whose
// export list is the drop-in ABI of the reference's ops and stays what it was): the input step of a network that takes point features.
//   votenet_subsample_augment_features   votenet_subsample_augment's points -- the same device text, ../augment_points.h -- plus, per
//                                        point, the height above the scene's floor and up to four raw columns (colour, intensity).
// Two launches: subsample_augment_kernel<T, true> (gather + transform + columns), floor_height_kernel (floor + heights).
#include "../augment_points.h"
#include "../error_text.h"
#include <cmath>
#pragma GCC visibility push(default)
#include "../../../include/votenet_point_features.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_point_features_last_error()) ----
static thread_local ErrorText g_feat_err;
#define FEAT_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_feat_err, cond, __VA_ARGS__)

// ---- height above the floor (votenet_subsample_augment_features) ----
// up = -y of the output point (upright camera, y down); the floor of a scene is np.percentile(up, 0.99) over its finite values:
// k = 0.0099 (m - 1), the order statistics of rank floor(k) and the next one, interpolated.  Both ranks by ONE radix select over
// order-preserving 32-bit keys: four passes of 8 bits, a histogram per wave in LDS (a flat floor puts a third of the scene into one
// bin: the same-address adds of one wave serialise, but never those of sixteen), the bin that holds a rank found by a wave64 scan.
// While the two ranks share their prefix -- every pass but the last, as a rule -- one histogram serves both.  One workgroup per
// scene: it then walks its rows again and writes height = up - floor (0 for a row whose up is not finite).
constexpr int FLOOR_THREADS = 1024, FLOOR_WAVES = FLOOR_THREADS / 64;

__device__ __forceinline__ unsigned up_key(float up) // unsigned order == float order (-0.0 sorts just below +0.0: equal values)
{
    const unsigned u = __float_as_uint(up);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_up(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(FLOOR_THREADS) void floor_height_kernel(int n_out, const float *__restrict__ points, int c,
                                                                     float *__restrict__ feats, float *__restrict__ floor_out,
                                                                     float *__restrict__ order_stats)
{
    __shared__ unsigned hist[2][FLOOR_WAVES][256];
    __shared__ unsigned s_m, s_prefix[2], s_rank[2];
    const int sc = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float *py = points + (long)sc * n_out * 3 + 1;
    if (tid == 0) s_m = 0u;
    __syncthreads();
    unsigned cnt = 0;
    for (int j = tid; j < n_out; j += FLOOR_THREADS) cnt += finite_bits(-py[(long)j * 3]) ? 1u : 0u;
    cnt = wave_sum_u32(cnt);
    if (lane == 0 && cnt) atomicAdd(&s_m, cnt);
    __syncthreads();
    const unsigned m = s_m;
    float fl = 0.0f;
    if (m > 0) { // (uniform)
        const double k = 0.0099 * (double)(m - 1);
        const unsigned lo = (unsigned)floor(k);
        const double t = k - (double)lo;
        if (tid == 0) {
            s_prefix[0] = s_prefix[1] = 0u;
            s_rank[0] = lo;
            s_rank[1] = lo + 1 < m ? lo + 1 : m - 1;
        }
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            const unsigned above = pass ? 0xffffffffu << (shift + 8) : 0u; // the digits already decided
            __syncthreads();
            const unsigned p0 = s_prefix[0], p1 = s_prefix[1];
            const bool same = p0 == p1;
            for (int i = lane; i < 256; i += 64) hist[0][wave][i] = hist[1][wave][i] = 0u;
            __syncthreads();
            for (int j = tid; j < n_out; j += FLOOR_THREADS) {
                const float up = -py[(long)j * 3];
                if (!finite_bits(up)) continue;
                const unsigned key = up_key(up), d = (key >> shift) & 255u;
                if ((key & above) == p0) atomicAdd(&hist[0][wave][d], 1u);
                if (!same && (key & above) == p1) atomicAdd(&hist[1][wave][d], 1u);
            }
            __syncthreads();
            if (tid < (same ? 256 : 512)) { // the waves' histograms summed into wave 0's row (a thread owns its bin's column)
                const int w = tid >> 8, bin = tid & 255;
                unsigned s = 0;
                for (int v = 0; v < FLOOR_WAVES; v++) s += hist[w][v][bin];
                hist[w][0][bin] = s;
            }
            __syncthreads();
            if (wave < 2) { // wave w finds the bin of rank w: lane l owns bins 4l .. 4l+3
                const unsigned *h = hist[same ? 0 : wave][0];
                const unsigned rank = s_rank[wave];
                const unsigned b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];
                const unsigned own = b0 + b1 + b2 + b3;
                unsigned incl = own;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                unsigned before = incl - own;
                if (before <= rank && rank < incl) { // exactly one lane
                    unsigned bin = 4 * lane;
                    if (rank >= before + b0) {
                        before += b0;
                        bin++;
                        if (rank >= before + b1) {
                            before += b1;
                            bin++;
                            if (rank >= before + b2) {
                                before += b2;
                                bin++;
                            }
                        }
                    }
                    s_prefix[wave] = (wave ? p1 : p0) | (bin << shift);
                    s_rank[wave] = rank - before;
                }
            }
        }
        __syncthreads();
        const float a = key_up(s_prefix[0]), b = key_up(s_prefix[1]);
        fl = (float)((double)a + ((double)b - (double)a) * t);
        if (tid == 0 && order_stats) {
            order_stats[2 * sc] = a;
            order_stats[2 * sc + 1] = b;
        }
    } else if (tid == 0 && order_stats) {
        order_stats[2 * sc] = order_stats[2 * sc + 1] = 0.0f;
    }
    if (tid == 0) floor_out[sc] = fl;
    float *f = feats + (long)sc * n_out * c;
    for (int j = tid; j < n_out; j += FLOOR_THREADS) {
        const float up = -py[(long)j * 3];
        f[(long)j * c] = finite_bits(up) ? up - fl : 0.0f;
    }
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_point_features_last_error(void) { return g_feat_err.text; }

extern "C" int votenet_subsample_augment_features(int b, int n_out, const void *raw, int raw_f64, int raw_stride,
                                                  const long *raw_offset, const int *choice, unsigned long long seed, long scene0,
                                                  int depth_to_camera, const int *flip, const double *rot_cos, const double *rot_sin,
                                                  const double *scale, int want_height, int extra_cols, float *out, float *feats,
                                                  float *floor, float *order_stats, void *stream)
{
    const char *what = "subsample_augment_features";
    char msg[256];
    FEAT_REQUIRE(points_args_ok(what, b, n_out, raw, raw_stride, raw_offset, flip, rot_cos, rot_sin, scale, out, msg, sizeof msg), "%s", msg);
    FEAT_REQUIRE(want_height == 0 || want_height == 1, "%s: want_height must be 0 or 1, got %d", what, want_height);
    FEAT_REQUIRE(extra_cols >= 0 && extra_cols <= 4, "%s: extra_cols must be in [0, 4], got %d", what, extra_cols);
    const int c = want_height + extra_cols;
    FEAT_REQUIRE(c >= 1, "%s: no feature asked for (want_height = 0 and extra_cols = 0)", what);
    FEAT_REQUIRE(3 + extra_cols <= raw_stride, "%s: extra_cols = %d needs raw rows of %d elements, raw_stride is %d", what, extra_cols,
               3 + extra_cols, raw_stride);
    FEAT_REQUIRE(feats, "%s: null feats pointer", what);
    FEAT_REQUIRE(!want_height || floor, "%s: null floor pointer (want_height = 1)", what);
    // extra_cols = 0: the plain gather (the second launch writes the only column)
    launch_points(b, n_out, raw, raw_f64, raw_stride, raw_offset, choice, seed, scene0, depth_to_camera, flip, rot_cos, rot_sin, scale,
                  out, extra_cols ? feats : nullptr, c, want_height, extra_cols, as_stream(stream));
    if (want_height)
        hipLaunchKernelGGL(floor_height_kernel, dim3(b), dim3(FLOOR_THREADS), 0, as_stream(stream), n_out, out, c, feats, floor,
                           order_stats);
    return g_feat_err.check_launch(what);
}
