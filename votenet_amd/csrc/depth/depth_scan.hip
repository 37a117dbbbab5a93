// depth_scan.hip -- libvotenet_depth.so (include/votenet_depth_scan.h), a library of its own beside libvotenet_hip.so: the raw scan of
// a batch of scenes from their 16-bit depth images, optionally with colour -- what votenet_subsample_augment, votenet_select_boxes
// and votenet_subsample_augment_features take as `raw`.  The rule of the header is double arithmetic in a fixed order
// (-ffp-contract=off, as everywhere in this project), rounded once to float: tests/depth_scan_ref.py restates it in numpy and the
// bytes are compared exactly.
//   depth_count_kernel   the valid pixels of every tile.  A tile is DS_TILE pixels of ONE scene; a lane takes 8 consecutive pixels.
//   depth_scan_kernel    one workgroup: the exclusive scan over all tiles of all scenes, and raw_offset_dev.
//   depth_emit_kernel    decodes again, forms the rows in LDS in pixel order and writes the tile's rows, which are contiguous in raw,
//                        with 16-byte stores.
// Tiles are cut on 16-byte boundaries of the depth ADDRESS, not on the scene's first pixel (scene starts are not aligned): with
// a = the scene's first pixel's address / 2 mod 8, tile t of the scene holds its pixels p with t DS_TILE <= p + a < (t + 1) DS_TILE, and
// lane l the eight from p + a = t DS_TILE + 8 l -- one 16-byte load where all eight belong to the scene, element loads for the at most
// two groups per scene that straddle its first or last pixel.  Pixel order is lane order, so a row's position is the tile's base + the
// counts of the lanes before it (a wave64 prefix and four wave totals) + the valid pixels before it in its own lane: no atomic.
#include "../common.h"
#include "../error_text.h"

#include <cstdint>
#pragma GCC visibility push(default)
#include "../../../include/votenet_depth_scan.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_depth_scan_last_error()) ----
static thread_local ErrorText g_ds_err;
#define DS_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_ds_err, cond, __VA_ARGS__)

constexpr int DS_MAX_B = 32;          // scenes per call: their offsets and calibrations are kernel arguments (3.7 KB of them)
constexpr int DS_THREADS = 256;       // four waves
constexpr int DS_PPT = 8;             // pixels per lane: 16 bytes of depth
constexpr int DS_TILE = DS_THREADS * DS_PPT; // 2048 pixels per workgroup: a 530 x 730 scene is 189 tiles
constexpr int DS_SCAN_THREADS = 1024;
constexpr long DS_MAX_PIXELS = 1L << 31; // exclusive, all scenes together: positions are ints

struct DsPixels {
    long off[DS_MAX_B + 1];
};

struct DsScenes {
    long off[DS_MAX_B + 1];
    double R[DS_MAX_B][9]; // row-major Rtilt
    double K[DS_MAX_B][4]; // K[0,0], K[1,1], K[0,2], K[1,2]
    int w[DS_MAX_B];
};

__host__ __device__ inline int ds_head(const unsigned short *depth, long off) // a: where the scene starts inside its 16-byte group
{
    return (int)(((reinterpret_cast<uintptr_t>(depth) >> 1) + (uintptr_t)off) & 7);
}
__host__ __device__ inline long ds_tiles(int head, long n) { return (head + n + DS_TILE - 1) / DS_TILE; }

// The lane's eight pixel values, zero (= not valid) where the position lies outside the scene.  p0 = the first position's pixel index
// in the scene (-7 .. n - 1), px = the scene's pixels, n their count.
__device__ __forceinline__ void ds_load8(const unsigned short *__restrict__ px, long p0, long n, unsigned short v[DS_PPT])
{
    if (p0 >= 0 && p0 + DS_PPT <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(px + p0); // 16-byte aligned: the tiles are cut so
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = (unsigned short)(w[k] & 0xffffu);
            v[2 * k + 1] = (unsigned short)(w[k] >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < DS_PPT; k++) v[k] = (p0 + k >= 0 && p0 + k < n) ? px[p0 + k] : (unsigned short)0;
    }
}

__device__ __forceinline__ int wave_inclusive_sum(int v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane_id() >= d) v += o;
    }
    return v;
}

// Grid (the most tiles a scene of the call has, b): a workgroup beyond its scene's tiles counts nothing.  count[scene][tile].
__global__ __launch_bounds__(DS_THREADS) void depth_count_kernel(DsPixels P, const unsigned short *__restrict__ depth, int max_tiles,
                                                                 int *__restrict__ count)
{
    __shared__ int s_wave[DS_THREADS / 64];
    const int sc = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const long off = P.off[sc], n = P.off[sc + 1] - off;
    const int head = ds_head(depth, off);
    int c = 0;
    if (t < ds_tiles(head, n)) {
        unsigned short v[DS_PPT];
        ds_load8(depth + off, (long)t * DS_TILE + tid * DS_PPT - head, n, v);
#pragma unroll
        for (int k = 0; k < DS_PPT; k++) c += v[k] != 0; // the rotation of encoding 0 keeps zero and nothing else at zero
    }
    c = wave_inclusive_sum(c);
    if (lane_id() == 63) s_wave[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) count[(size_t)sc * max_tiles + t] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// One workgroup.  tile[i]: the count on entry, the valid pixels of all tiles before i on exit; raw_offset_dev[s] = that of scene s's
// first tile, raw_offset_dev[b] the total.
__global__ __launch_bounds__(DS_SCAN_THREADS) void depth_scan_kernel(int b, int max_tiles, int *__restrict__ tile,
                                                                     long *__restrict__ raw_offset_dev)
{
    __shared__ int s_wave[DS_SCAN_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6;
    const long total = (long)b * max_tiles;
    long carry = 0; // the same in every thread
    for (long base = 0; base < total; base += DS_SCAN_THREADS) {
        const long i = base + tid;
        const int v = i < total ? tile[i] : 0;
        const int incl = wave_inclusive_sum(v);
        if (lane_id() == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < DS_SCAN_THREADS / 64; k++) {
            before += k < wave ? s_wave[k] : 0;
            all += s_wave[k];
        }
        const long excl = carry + before + (incl - v);
        if (i < total) {
            tile[i] = (int)excl; // < 2^31: at most one per pixel
            if (i % max_tiles == 0) raw_offset_dev[i / max_tiles] = excl;
        }
        carry += all;
        __syncthreads(); // s_wave is rewritten by the next round
    }
    if (tid == 0) raw_offset_dev[b] = carry;
}

// STRIDE 3: coordinates; 6: coordinates and colour.  The workgroup's rows sit in LDS at the float position they have in raw modulo 4
// (`shift`), so that a 16-byte LDS read is a 16-byte aligned store; what lies before the first and after the last 16-byte boundary goes
// out as single floats.  Nothing at or beyond float cap_rows * STRIDE is written.
template <int STRIDE>
__global__ __launch_bounds__(DS_THREADS) void depth_emit_kernel(DsScenes P, const unsigned short *__restrict__ depth,
                                                                const unsigned char *__restrict__ rgb, int encoding, double origin,
                                                                double max_depth, int max_tiles, const int *__restrict__ tile_base,
                                                                float *__restrict__ raw, long cap_rows)
{
    __shared__ __attribute__((aligned(16))) float s_rows[DS_TILE * STRIDE + 4];
    __shared__ float s_colour[256];
    __shared__ int s_wave[DS_THREADS / 64];
    const int sc = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const long off = P.off[sc], n = P.off[sc + 1] - off;
    const int head = ds_head(depth, off);
    if (t >= ds_tiles(head, n)) return; // the whole workgroup
    const long p0 = (long)t * DS_TILE + tid * DS_PPT - head;
    unsigned short v[DS_PPT];
    ds_load8(depth + off, p0, n, v);
    int c = 0;
#pragma unroll
    for (int k = 0; k < DS_PPT; k++) c += v[k] != 0;
    const int incl = wave_inclusive_sum(c);
    if (lane_id() == 63) s_wave[tid >> 6] = incl;
    if (STRIDE == 6) s_colour[tid] = (float)((double)tid / 255.0);
    __syncthreads();
    int before = 0, rows = 0;
#pragma unroll
    for (int k = 0; k < DS_THREADS / 64; k++) {
        before += k < (tid >> 6) ? s_wave[k] : 0;
        rows += s_wave[k];
    }
    const long row0 = tile_base[(size_t)sc * max_tiles + t];
    const size_t f0 = (size_t)row0 * STRIDE; // the tile's first float in raw
    const int shift = (int)(((reinterpret_cast<uintptr_t>(raw) >> 2) + f0) & 3);
    if (c) {
        unsigned char col8[DS_PPT * 3];
        if (STRIDE == 6) {
            if (p0 >= 0 && p0 + DS_PPT <= n && ((reinterpret_cast<uintptr_t>(rgb) + (uintptr_t)(off + p0) * 3) & 7) == 0) {
                const uint2 *q = reinterpret_cast<const uint2 *>(rgb + (off + p0) * 3);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint2 w = q[k];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        col8[8 * k + j] = (unsigned char)(w.x >> (8 * j));
                        col8[8 * k + 4 + j] = (unsigned char)(w.y >> (8 * j));
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < DS_PPT; k++) {
                    const bool in = p0 + k >= 0 && p0 + k < n;
#pragma unroll
                    for (int j = 0; j < 3; j++) col8[3 * k + j] = in ? rgb[(off + p0 + k) * 3 + j] : (unsigned char)0;
                }
            }
        }
        const double *__restrict__ R = P.R[sc];
        const double fu = P.K[sc][0], fv = P.K[sc][1], cu = P.K[sc][2], cv = P.K[sc][3];
        const int w = P.w[sc];
        const long first = p0 < 0 ? 0 : p0; // a valid pixel lies at or after it
        int prow = (int)(first / w), pcol = (int)(first - (long)prow * w);
        float *__restrict__ dst = s_rows + shift + (size_t)(before + incl - c) * STRIDE;
#pragma unroll
        for (int k = 0; k < DS_PPT; k++) {
            if (p0 + k < first) continue;
            if (v[k] != 0) {
                const unsigned p = v[k];
                const unsigned d16 = encoding == 0 ? ((p >> 3) | (p << 13)) & 0xffffu : p;
                double z = (double)d16 / 1000.0;
                if (z > max_depth) z = max_depth;
                const double uu = (double)pcol + origin, vv = (double)prow + origin;
                const double x = ((uu - cu) * z) / fu;
                const double y = ((vv - cv) * z) / fv;
                const double q0 = x, q1 = z, q2 = -y;
                dst[0] = (float)((R[0] * q0 + R[1] * q1) + R[2] * q2);
                dst[1] = (float)((R[3] * q0 + R[4] * q1) + R[5] * q2);
                dst[2] = (float)((R[6] * q0 + R[7] * q1) + R[8] * q2);
                if (STRIDE == 6) {
                    dst[3] = s_colour[col8[3 * k + 0]];
                    dst[4] = s_colour[col8[3 * k + 1]];
                    dst[5] = s_colour[col8[3 * k + 2]];
                }
                dst += STRIDE;
            }
            if (++pcol == w) pcol = 0, prow++;
        }
    }
    __syncthreads();
    const size_t cap = (size_t)cap_rows * STRIDE;
    if (f0 >= cap) return;
    const size_t room = cap - f0;
    const int len = (size_t)rows * STRIDE < room ? rows * STRIDE : (int)room; // floats to write, <= DS_TILE * STRIDE
    // LDS float j in [shift, shift + len) is raw float f0 - shift + j; f0 - shift is a multiple of four floats from a 16-byte boundary
    float *__restrict__ out = raw + f0 - shift;
    const int jb = shift, je = shift + len;
    const int qb = (jb + 3) >> 2, qe = je >> 2;
    const int he = 4 * qb < je ? 4 * qb : je;   // [jb, he): before the first boundary
    const int ts = 4 * qe > he ? 4 * qe : he;   // [ts, je): after the last
    for (int q = qb + tid; q < qe; q += DS_THREADS)
        reinterpret_cast<float4 *>(out)[q] = reinterpret_cast<const float4 *>(s_rows)[q];
    if (tid < 4 && jb + tid < he) out[jb + tid] = s_rows[jb + tid];
    if (tid >= 4 && tid < 8 && ts + (tid - 4) < je) out[ts + (tid - 4)] = s_rows[ts + (tid - 4)];
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_depth_scan_last_error(void) { return g_ds_err.text; }

extern "C" size_t votenet_depth_scan_workspace_bytes(int b, long total_pixels)
{
    // a scene of n pixels that starts a pixels into its 16-byte group has ceil((a + n) / DS_TILE) <= n / DS_TILE + 2 tiles, and n <= total
    const size_t scenes = b > 0 ? (size_t)b : 1, pixels = total_pixels > 0 ? (size_t)total_pixels : 0;
    return scenes * (pixels / DS_TILE + 2) * sizeof(int);
}

extern "C" int votenet_depth_scan(int b, const unsigned short *depth, const unsigned char *rgb, const long *pix_offset, const int *hw,
                                  const double *rtilt, const double *k, int encoding, double pixel_origin, double max_depth, float *raw,
                                  int raw_stride, long raw_capacity_rows, long *raw_offset_dev, void *ws, size_t ws_bytes, void *stream)
{
    DS_REQUIRE(b >= 1 && b <= DS_MAX_B, "depth_scan: 1 to %d scenes per call, got b = %d", DS_MAX_B, b);
    DS_REQUIRE(depth && pix_offset && hw && rtilt && k && raw_offset_dev && ws, "depth_scan: null pointer");
    DS_REQUIRE(raw || raw_capacity_rows == 0, "depth_scan: null raw with room for %ld rows", raw_capacity_rows);
    DS_REQUIRE(encoding == 0 || encoding == 1, "depth_scan: encoding must be 0 (the dataset's) or 1 (millimetres), got %d", encoding);
    DS_REQUIRE(raw_stride == (rgb ? 6 : 3), "depth_scan: raw_stride must be %d %s colour, got %d", rgb ? 6 : 3, rgb ? "with" : "without",
               raw_stride);
    DS_REQUIRE(raw_capacity_rows >= 0, "depth_scan: raw_capacity_rows must be >= 0, got %ld", raw_capacity_rows);
    DS_REQUIRE(pix_offset[0] == 0, "depth_scan: pix_offset must start at 0, got %ld", pix_offset[0]);
    for (int s = 0; s < b; s++) {
        const int h = hw[2 * s], w = hw[2 * s + 1];
        DS_REQUIRE(h > 0 && w > 0, "depth_scan: scene %d is %d x %d pixels", s, h, w);
        DS_REQUIRE(pix_offset[s + 1] - pix_offset[s] == (long)h * w, "depth_scan: scene %d is %d x %d pixels, pix_offset gives it %ld", s, h,
                   w, pix_offset[s + 1] - pix_offset[s]);
        DS_REQUIRE(pix_offset[s + 1] < DS_MAX_PIXELS, "depth_scan: more than 2^31 - 1 pixels up to scene %d", s);
        DS_REQUIRE(k[9 * s + 0] != 0.0 && k[9 * s + 4] != 0.0, "depth_scan: scene %d has K[0,0] = %g, K[1,1] = %g", s, k[9 * s + 0],
                   k[9 * s + 4]);
    }
    const size_t need = votenet_depth_scan_workspace_bytes(b, pix_offset[b]);
    DS_REQUIRE(ws_bytes >= need, "depth_scan: workspace of %zu bytes, need %zu", ws_bytes, need);
    DS_REQUIRE(reinterpret_cast<uintptr_t>(depth) % 2 == 0 && reinterpret_cast<uintptr_t>(raw) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(raw_offset_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(ws) % 4 == 0,
               "depth_scan: depth must be 2-byte, raw and ws 4-byte and raw_offset_dev 8-byte aligned");
    DsScenes P = {};
    DsPixels Q = {};
    long max_tiles = 1;
    for (int s = 0; s < b; s++) {
        P.off[s] = Q.off[s] = pix_offset[s];
        P.off[s + 1] = Q.off[s + 1] = pix_offset[s + 1];
        for (int a = 0; a < 9; a++) P.R[s][a] = rtilt[9 * s + a];
        P.K[s][0] = k[9 * s + 0], P.K[s][1] = k[9 * s + 4], P.K[s][2] = k[9 * s + 2], P.K[s][3] = k[9 * s + 5];
        P.w[s] = hw[2 * s + 1];
        const long tiles = ds_tiles(ds_head(depth, pix_offset[s]), pix_offset[s + 1] - pix_offset[s]);
        if (tiles > max_tiles) max_tiles = tiles;
    }
    // b * max_tiles ints fit: max_tiles <= pix_offset[b] / DS_TILE + 2, which is what `need` holds per scene
    int *tile = (int *)ws;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)max_tiles, b); // max_tiles <= 2^20 + 2
    hipLaunchKernelGGL(depth_count_kernel, grid, dim3(DS_THREADS), 0, st, Q, depth, (int)max_tiles, tile);
    hipLaunchKernelGGL(depth_scan_kernel, dim3(1), dim3(DS_SCAN_THREADS), 0, st, b, (int)max_tiles, tile, raw_offset_dev);
    if (rgb)
        hipLaunchKernelGGL(depth_emit_kernel<6>, grid, dim3(DS_THREADS), 0, st, P, depth, rgb, encoding, pixel_origin, max_depth,
                           (int)max_tiles, tile, raw, raw_capacity_rows);
    else
        hipLaunchKernelGGL(depth_emit_kernel<3>, grid, dim3(DS_THREADS), 0, st, P, depth, rgb, encoding, pixel_origin, max_depth,
                           (int)max_tiles, tile, raw, raw_capacity_rows);
    return g_ds_err.check_launch("depth_scan");
}
