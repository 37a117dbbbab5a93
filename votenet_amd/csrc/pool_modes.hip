// pool_modes.hip -- the pooling modes of pointnet_sa_module other than the fused max-pool path (utils.py:131-146), and group_all
// (utils.py:64-90): one group of all n points per scene.
//
//   votenet_bn_relu_pool        y = act(z*scale+shift) reduced over each group of k consecutive rows: mean, weighted sum,
//                               max (+ arg-max) or [mean | max].  A group's rows are split over workgroups when there are
//                               too few (group, channel tile) pairs to fill the GPU; the partials are combined in a fixed
//                               order by a second launch, so results do not depend on scheduling.  No atomics.
//   votenet_sa_pool_weights     w = softmax_k(-5 |v|), v = xyz[idx] - new_xyz or xyz (group_all)   (utils.py:135-140)
//   votenet_sa_pool_grad        the gradient reaching y: gout/k, w*gout, gout at the arg-max row, or both parts of [mean | max]
//   votenet_sa_pool_weights_grad  dv (rows x 3) through the softmax weights; |v| = 0 rows get 0 (tf.norm's 0 * inf is NaN there)
#include "common.h"

#include <cstdint>

namespace votenet {
namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_CTILE = 64;           // channels per workgroup
constexpr int POOL_MIN_ROWS = 256;       // a split keeps at least this many rows per workgroup
constexpr long POOL_TARGET_WG = 1024;    // ~4 workgroups per CU (256 CUs)

struct PoolPlan {
    int tiles, splits, chunk;
};

PoolPlan pool_plan(long groups, int k, int c)
{
    PoolPlan p;
    p.tiles = (c + POOL_CTILE - 1) / POOL_CTILE;
    const long base = groups * p.tiles;
    long s = 1;
    if (base > 0 && base < POOL_TARGET_WG) {
        s = (POOL_TARGET_WG + base - 1) / base;
        const long most = (k + POOL_MIN_ROWS - 1) / POOL_MIN_ROWS;
        if (s > most) s = most;
        if (s < 1) s = 1;
    }
    p.chunk = (int)((k + s - 1) / s);
    p.splits = (k + p.chunk - 1) / p.chunk;
    return p;
}

inline int grid_for(long total, int block)
{
    long g = (total + block - 1) / block;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ float act(float v, int relu) { return relu ? (v > 0.0f ? v : 0.0f) : v; }

// One workgroup per (group, split, channel tile).  V = 4: 16 channel quads x 16 row lanes, 16-byte loads; V = 1: 64 channels x
// 4 row lanes.  Each thread walks its rows in order; the row lanes are combined in lane order (sum) and by (value, row) for the
// maximum, so the first maximum in row order wins, as in votenet_bn_relu_max.  splits == 1: the final values are written;
// otherwise partial (sum, max, arg-max) per (group, split, channel) go to `work` for pool_combine_kernel.
template <int V>
__global__ __launch_bounds__(POOL_THREADS) void pool_partial_kernel(int k, int c, int splits, int chunk, const float *__restrict__ z,
                                                                     const float *__restrict__ scale, const float *__restrict__ shift,
                                                                     int relu, int mode, const float *__restrict__ w,
                                                                     float *__restrict__ out, int *__restrict__ argmax,
                                                                     float *__restrict__ work)
{
    constexpr int CL = POOL_CTILE / V;      // channel lanes
    constexpr int RL = POOL_THREADS / CL;   // row lanes
    __shared__ float s_sum[RL][POOL_CTILE];
    __shared__ float s_max[RL][POOL_CTILE];
    __shared__ int s_arg[RL][POOL_CTILE];

    const long gs = blockIdx.x;
    const long g = gs / splits;
    const int s = (int)(gs - g * splits);
    const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
    const int c0 = blockIdx.y * POOL_CTILE + cl * V;
    const int r0 = s * chunk, r1 = min(k, r0 + chunk);
    const bool want_sum = mode != VOTENET_POOL_MAX, want_max = mode == VOTENET_POOL_MAX || mode == VOTENET_POOL_MAX_AND_AVG;

    float sum[V], best[V], sc[V], sh[V];
    int bi[V];
#pragma unroll
    for (int u = 0; u < V; u++) {
        sum[u] = 0.0f;
        best[u] = 0.0f;
        bi[u] = -1;
        sc[u] = c0 + u < c ? scale[c0 + u] : 0.0f;
        sh[u] = c0 + u < c ? shift[c0 + u] : 0.0f;
    }
    if (c0 < c) {
        const float *__restrict__ zg = z + (size_t)g * k * c;
#pragma unroll 4
        for (int j = r0 + rl; j < r1; j += RL) {
            float x[V];
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(zg + (size_t)j * c + c0);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
                x[0] = zg[(size_t)j * c + c0];
            }
            const float wj = mode == VOTENET_POOL_WEIGHTED_AVG ? w[(size_t)g * k + j] : 1.0f;
#pragma unroll
            for (int u = 0; u < V; u++) {
                const float y = act(x[u] * sc[u] + sh[u], relu);
                if (want_sum) sum[u] += mode == VOTENET_POOL_WEIGHTED_AVG ? wj * y : y;
                if (want_max && (bi[u] < 0 || y > best[u])) {
                    best[u] = y;
                    bi[u] = j;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < V; u++) {
        s_sum[rl][cl * V + u] = sum[u];
        s_max[rl][cl * V + u] = best[u];
        s_arg[rl][cl * V + u] = bi[u];
    }
    __syncthreads();
    if (threadIdx.x >= POOL_CTILE) return;
    const int ch = blockIdx.y * POOL_CTILE + threadIdx.x;
    if (ch >= c) return;
    float tsum = 0.0f, tmax = 0.0f;
    int targ = -1;
    for (int r = 0; r < RL; r++) {
        tsum += s_sum[r][threadIdx.x];
        const int a = s_arg[r][threadIdx.x];
        const float v = s_max[r][threadIdx.x];
        if (a >= 0 && (targ < 0 || v > tmax || (v == tmax && a < targ))) {
            tmax = v;
            targ = a;
        }
    }
    if (splits == 1) {
        const int cw = mode == VOTENET_POOL_MAX_AND_AVG ? 2 * c : c;
        float *o = out + (size_t)g * cw;
        if (mode == VOTENET_POOL_AVG || mode == VOTENET_POOL_MAX_AND_AVG) o[ch] = tsum / (float)k;
        if (mode == VOTENET_POOL_WEIGHTED_AVG) o[ch] = tsum;
        if (mode == VOTENET_POOL_MAX) o[ch] = tmax;
        if (mode == VOTENET_POOL_MAX_AND_AVG) o[c + ch] = tmax;
        if (want_max && argmax) argmax[(size_t)g * c + ch] = targ;
        return;
    }
    const size_t e = ((size_t)g * splits + s) * c + ch, plane = (size_t)gridDim.x * c;  // gridDim.x = groups * splits
    work[e] = tsum;
    work[plane + e] = tmax;
    reinterpret_cast<int *>(work)[2 * plane + e] = targ;
}

// Second stage: per (group, channel) the splits in increasing order (their rows are in increasing order too, so a strict
// comparison keeps the first maximum).
__global__ void pool_combine_kernel(long groups, int k, int c, int splits, int mode, const float *__restrict__ work,
                                    float *__restrict__ out, int *__restrict__ argmax)
{
    const long total = groups * c;
    const size_t plane = (size_t)groups * splits * c;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long g = e / c;
        const int ch = (int)(e - g * c);
        float tsum = 0.0f, tmax = 0.0f;
        int targ = -1;
        for (int s = 0; s < splits; s++) {
            const size_t p = ((size_t)g * splits + s) * c + ch;
            tsum += work[p];
            const float v = work[plane + p];
            const int a = reinterpret_cast<const int *>(work)[2 * plane + p];
            if (a >= 0 && (targ < 0 || v > tmax)) {
                tmax = v;
                targ = a;
            }
        }
        const int cw = mode == VOTENET_POOL_MAX_AND_AVG ? 2 * c : c;
        float *o = out + (size_t)g * cw;
        if (mode == VOTENET_POOL_AVG || mode == VOTENET_POOL_MAX_AND_AVG) o[ch] = tsum / (float)k;
        if (mode == VOTENET_POOL_WEIGHTED_AVG) o[ch] = tsum;
        if (mode == VOTENET_POOL_MAX) o[ch] = tmax;
        if (mode == VOTENET_POOL_MAX_AND_AVG) o[c + ch] = tmax;
        if ((mode == VOTENET_POOL_MAX || mode == VOTENET_POOL_MAX_AND_AVG) && argmax) argmax[e] = targ;
    }
}

// Block-wide reductions in a fixed order: each wave by a butterfly, then the waves in index order through LDS.
template <int NT>
__device__ float block_reduce(float v, bool is_max, float *lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, t) : v + t;
    }
    constexpr int NW = NT / 64;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = lds[0];
    for (int i = 1; i < NW; i++) r = is_max ? fmaxf(r, lds[i]) : r + lds[i];
    return r;
}

__device__ __forceinline__ void group_vec(int n, int m, int k, const float *xyz, const float *new_xyz, const int *idx, long g, int j,
                                          float &vx, float &vy, float &vz)
{
    const long bb = g / m;
    if (idx) {
        const int p = idx[(size_t)g * k + j];
        const float *q = xyz + ((size_t)bb * n + p) * 3, *cn = new_xyz + (size_t)g * 3;
        vx = q[0] - cn[0];
        vy = q[1] - cn[1];
        vz = q[2] - cn[2];
    } else {  // group_all: the raw coordinates, group g = scene g
        const float *q = xyz + ((size_t)bb * n + j) * 3;
        vx = q[0];
        vy = q[1];
        vz = q[2];
    }
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// One workgroup per group: the maximum of s = -5|v|, the sum of exp(s - max), then w = exp(s - max) / sum.
template <int NT>
__global__ __launch_bounds__(NT) void pool_weights_kernel(int n, int m, int k, const float *__restrict__ xyz,
                                                          const float *__restrict__ new_xyz, const int *__restrict__ idx,
                                                          float *__restrict__ w)
{
    __shared__ float lds[NT / 64];
    const long g = blockIdx.x;
    float *wg = w + (size_t)g * k;
    float smax = -__builtin_inff();
    for (int j = threadIdx.x; j < k; j += NT) {
        float vx, vy, vz;
        group_vec(n, m, k, xyz, new_xyz, idx, g, j, vx, vy, vz);
        const float s = -norm3(vx, vy, vz) * 5.0f;
        wg[j] = s;
        smax = fmaxf(smax, s);
    }
    smax = block_reduce<NT>(smax, true, lds);
    float ssum = 0.0f;
    for (int j = threadIdx.x; j < k; j += NT) {
        const float e = expf(wg[j] - smax);
        wg[j] = e;
        ssum += e;
    }
    ssum = block_reduce<NT>(ssum, false, lds);
    for (int j = threadIdx.x; j < k; j += NT) wg[j] = wg[j] / ssum;
}

// da[row, ch] = d out / d y[row, ch]   (gout: groups x cw, cw = 2c for [mean | max], else c)
__global__ void pool_grad_kernel(long rows, int k, int c, int mode, const float *__restrict__ gout, const float *__restrict__ w,
                                 const int *__restrict__ argmax, float *__restrict__ da)
{
    const long total = rows * c;
    const int cw = mode == VOTENET_POOL_MAX_AND_AVG ? 2 * c : c;
    const float inv_k = 1.0f / (float)k;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long row = e / c;
        const int ch = (int)(e - row * c);
        const long g = row / k;
        const int j = (int)(row - g * k);
        const float *go = gout + (size_t)g * cw;
        float v = 0.0f;
        if (mode == VOTENET_POOL_AVG || mode == VOTENET_POOL_MAX_AND_AVG) v = go[ch] * inv_k;
        if (mode == VOTENET_POOL_WEIGHTED_AVG) v = w[row] * go[ch];
        if (mode == VOTENET_POOL_MAX && argmax[(size_t)g * c + ch] == j) v = go[ch];
        if (mode == VOTENET_POOL_MAX_AND_AVG && argmax[(size_t)g * c + ch] == j) v += go[c + ch];
        da[e] = v;
    }
}

// c % 4 == 0 and 16-byte aligned gout / da: a channel quad per thread
__global__ void pool_grad_vec_kernel(long rows, int k, int c, int mode, const float *__restrict__ gout, const float *__restrict__ w,
                                     const int *__restrict__ argmax, float *__restrict__ da)
{
    const int qc = c >> 2;
    const long total = rows * qc;
    const int cw = mode == VOTENET_POOL_MAX_AND_AVG ? 2 * c : c;
    const float inv_k = 1.0f / (float)k;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long row = e / qc;
        const int q = (int)(e - row * qc);
        const long g = row / k;
        const int j = (int)(row - g * k);
        const float *go = gout + (size_t)g * cw + 4 * q;
        float v[4];
        for (int u = 0; u < 4; u++) {
            float t = 0.0f;
            if (mode == VOTENET_POOL_AVG || mode == VOTENET_POOL_MAX_AND_AVG) t = go[u] * inv_k;
            if (mode == VOTENET_POOL_WEIGHTED_AVG) t = w[row] * go[u];
            if (mode == VOTENET_POOL_MAX && argmax[(size_t)g * c + 4 * q + u] == j) t = go[u];
            if (mode == VOTENET_POOL_MAX_AND_AVG && argmax[(size_t)g * c + 4 * q + u] == j) t += go[c + u];
            v[u] = t;
        }
        *reinterpret_cast<float4 *>(da + (size_t)row * c + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// gw[row] = sum_c gout[g, c] * act(z[row, c]*scale[c]+shift[c]): one wave per row, lanes over the channels, a butterfly sum.
__global__ __launch_bounds__(256) void pool_wdot_kernel(long rows, int k, int c, const float *__restrict__ z,
                                                        const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                                                        const float *__restrict__ gout, float *__restrict__ gw)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float *zr = z + (size_t)row * c, *go = gout + (size_t)(row / k) * c;
    float acc = 0.0f;
    for (int ch = lane; ch < c; ch += 64) acc += go[ch] * act(zr[ch] * scale[ch] + shift[ch], relu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) gw[row] = acc;
}

// Per group: t = sum_j w_j gw_j, ds_j = w_j (gw_j - t), d|v|_j = -5 ds_j, dv_j = d|v|_j v_j / |v_j| (0 where |v_j| = 0).
template <int NT>
__global__ __launch_bounds__(NT) void pool_weights_grad_kernel(int n, int m, int k, const float *__restrict__ xyz,
                                                               const float *__restrict__ new_xyz, const int *__restrict__ idx,
                                                               const float *__restrict__ w, const float *__restrict__ gw,
                                                               float *__restrict__ dv)
{
    __shared__ float lds[NT / 64];
    const long g = blockIdx.x;
    const float *wg = w + (size_t)g * k, *gg = gw + (size_t)g * k;
    float t = 0.0f;
    for (int j = threadIdx.x; j < k; j += NT) t += wg[j] * gg[j];
    t = block_reduce<NT>(t, false, lds);
    for (int j = threadIdx.x; j < k; j += NT) {
        float vx, vy, vz;
        group_vec(n, m, k, xyz, new_xyz, idx, g, j, vx, vy, vz);
        const float d = norm3(vx, vy, vz);
        const float dd = -5.0f * (wg[j] * (gg[j] - t));
        const float f = d > 0.0f ? dd / d : 0.0f;
        float *o = dv + ((size_t)g * k + j) * 3;
        o[0] = f * vx;
        o[1] = f * vy;
        o[2] = f * vz;
    }
}

bool valid_mode(int mode) { return mode >= VOTENET_POOL_MAX && mode <= VOTENET_POOL_MAX_AND_AVG; }

}  // namespace
}  // namespace votenet

using namespace votenet;

extern "C" size_t votenet_bn_relu_pool_workspace_floats(long groups, int k, int c)
{
    if (groups <= 0 || k <= 0 || c <= 0) return 0;
    const PoolPlan p = pool_plan(groups, k, c);
    return p.splits > 1 ? 3 * (size_t)groups * p.splits * c : 0;
}

extern "C" int votenet_bn_relu_pool(long groups, int k, int c, const float *z, const float *scale, const float *shift, int relu, int mode,
                                    const float *w, float *out, int *argmax, float *work, void *stream)
{
    VN_REQUIRE(groups >= 0 && k > 0 && c > 0, "bn_relu_pool expects groups >= 0, k > 0, c > 0");
    VN_REQUIRE(valid_mode(mode), "bn_relu_pool: unknown pooling mode %d", mode);
    if (groups == 0) return VOTENET_OK;
    VN_REQUIRE(z && scale && shift && out, "bn_relu_pool: null buffer");
    VN_REQUIRE(mode != VOTENET_POOL_WEIGHTED_AVG || w, "bn_relu_pool: weighted_avg needs the weights");
    const PoolPlan p = pool_plan(groups, k, c);
    VN_REQUIRE(p.splits == 1 || work, "bn_relu_pool: %d splits need the workspace (votenet_bn_relu_pool_workspace_floats)", p.splits);
    VN_REQUIRE(groups * p.splits < (1L << 31) && p.tiles < 65536, "bn_relu_pool: too many groups");
    const bool vec = c % 4 == 0 && (uintptr_t)z % 16 == 0;
    const dim3 grid((unsigned)(groups * p.splits), (unsigned)p.tiles);
    if (vec)
        hipLaunchKernelGGL(pool_partial_kernel<4>, grid, dim3(POOL_THREADS), 0, as_stream(stream), k, c, p.splits, p.chunk, z, scale,
                           shift, relu, mode, w, out, argmax, work);
    else
        hipLaunchKernelGGL(pool_partial_kernel<1>, grid, dim3(POOL_THREADS), 0, as_stream(stream), k, c, p.splits, p.chunk, z, scale,
                           shift, relu, mode, w, out, argmax, work);
    int rc = check_launch("bn_relu_pool");
    if (rc != VOTENET_OK || p.splits == 1) return rc;
    hipLaunchKernelGGL(pool_combine_kernel, dim3(grid_for(groups * c, 256)), dim3(256), 0, as_stream(stream), groups, k, c, p.splits,
                       mode, work, out, argmax);
    return check_launch("bn_relu_pool combine");
}

extern "C" int votenet_sa_pool_weights(int b, int n, int m, int k, const float *xyz, const float *new_xyz, const int *idx, float *w,
                                       void *stream)
{
    VN_REQUIRE(b >= 0 && n > 0 && m > 0 && k > 0, "sa_pool_weights expects b >= 0, n > 0, m > 0, k > 0");
    VN_REQUIRE((idx == nullptr) == (new_xyz == nullptr), "sa_pool_weights: idx and new_xyz are given together (or neither: group_all)");
    VN_REQUIRE(idx || (m == 1 && k == n), "sa_pool_weights: group_all takes m = 1, k = n");
    if (b == 0) return VOTENET_OK;
    VN_REQUIRE(xyz && w, "sa_pool_weights: null buffer");
    if (k >= 4096)
        hipLaunchKernelGGL(pool_weights_kernel<1024>, dim3((unsigned)((long)b * m)), dim3(1024), 0, as_stream(stream), n, m, k, xyz,
                           new_xyz, idx, w);
    else
        hipLaunchKernelGGL(pool_weights_kernel<64>, dim3((unsigned)((long)b * m)), dim3(64), 0, as_stream(stream), n, m, k, xyz, new_xyz,
                           idx, w);
    return check_launch("sa_pool_weights");
}

extern "C" int votenet_sa_pool_grad(long groups, int k, int c, int mode, const float *gout, const float *w, const int *argmax, float *da,
                                    void *stream)
{
    VN_REQUIRE(groups >= 0 && k > 0 && c > 0, "sa_pool_grad expects groups >= 0, k > 0, c > 0");
    VN_REQUIRE(valid_mode(mode), "sa_pool_grad: unknown pooling mode %d", mode);
    if (groups == 0) return VOTENET_OK;
    VN_REQUIRE(gout && da, "sa_pool_grad: null buffer");
    VN_REQUIRE(mode != VOTENET_POOL_WEIGHTED_AVG || w, "sa_pool_grad: weighted_avg needs the weights");
    VN_REQUIRE((mode != VOTENET_POOL_MAX && mode != VOTENET_POOL_MAX_AND_AVG) || argmax, "sa_pool_grad: max needs the arg-max");
    const long rows = groups * k;
    if (c % 4 == 0 && (uintptr_t)gout % 16 == 0 && (uintptr_t)da % 16 == 0)
        hipLaunchKernelGGL(pool_grad_vec_kernel, dim3(grid_for(rows * (c / 4), 256)), dim3(256), 0, as_stream(stream), rows, k, c, mode,
                           gout, w, argmax, da);
    else
        hipLaunchKernelGGL(pool_grad_kernel, dim3(grid_for(rows * c, 256)), dim3(256), 0, as_stream(stream), rows, k, c, mode, gout, w,
                           argmax, da);
    return check_launch("sa_pool_grad");
}

extern "C" int votenet_sa_pool_weights_grad(int b, int n, int m, int k, int c, const float *xyz, const float *new_xyz, const int *idx,
                                            const float *z, const float *scale, const float *shift, int relu, const float *gout,
                                            const float *w, float *gw, float *dv, void *stream)
{
    VN_REQUIRE(b >= 0 && n > 0 && m > 0 && k > 0 && c > 0, "sa_pool_weights_grad expects b >= 0, n, m, k, c > 0");
    VN_REQUIRE((idx == nullptr) == (new_xyz == nullptr), "sa_pool_weights_grad: idx and new_xyz are given together (or neither: group_all)");
    VN_REQUIRE(idx || (m == 1 && k == n), "sa_pool_weights_grad: group_all takes m = 1, k = n");
    if (b == 0) return VOTENET_OK;
    VN_REQUIRE(xyz && z && scale && shift && gout && w && gw && dv, "sa_pool_weights_grad: null buffer");
    const long rows = (long)b * m * k;
    hipLaunchKernelGGL(pool_wdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, as_stream(stream), rows, k, c, z, scale, shift,
                       relu, gout, gw);
    int rc = check_launch("sa_pool_weights_grad dot");
    if (rc != VOTENET_OK) return rc;
    if (k >= 4096)
        hipLaunchKernelGGL(pool_weights_grad_kernel<1024>, dim3((unsigned)((long)b * m)), dim3(1024), 0, as_stream(stream), n, m, k, xyz,
                           new_xyz, idx, w, gw, dv);
    else
        hipLaunchKernelGGL(pool_weights_grad_kernel<64>, dim3((unsigned)((long)b * m)), dim3(64), 0, as_stream(stream), n, m, k, xyz,
                           new_xyz, idx, w, gw, dv);
    return check_launch("sa_pool_weights_grad");
}
