// instance_boxes.hip -- libvotenet_instbox.so (include/votenet_instance_boxes.h), a library of its own beside libvotenet_hip.so (whose
// export list stays what it was): ground-truth boxes from instance-labelled points, the axis-aligned extent of every instance in the
// cloud the network sees.
//   votenet_instance_boxes      memset of the workspace; instance_tile_kernel: a workgroup per (tile of points, scene) folds its points
//                               into a table of k entries in LDS and adds its non-empty entries to the workspace;
//                               instance_finish_kernel: a workgroup per scene decides status, class and slots and writes the rows.
//   votenet_instance_point_box  the row of every point's instance, elementwise.
// Every combination is an integer maximum or an integer sum: exact, the same in any order, no float atomic anywhere.  The float
// minimum and maximum go through the order-preserving map to unsigned; the minimum and the first index are kept complemented, so that
// every field combines by max (the count by add) and an all-zero table is the empty one: one memset initialises the workspace.
// tests/instance_boxes_ref.py restates the rule in numpy and every output is compared by bit pattern.
#include "../common.h"
#include "../error_text.h"

#include <cstdint>
#pragma GCC visibility push(default)
#include "../../../include/votenet_instance_boxes.h"
#pragma GCC visibility pop

namespace votenet {

// ---- error plumbing of this library (thread-local text behind votenet_instance_boxes_last_error()) ----
static thread_local ErrorText g_ib_err;
#define IB_REQUIRE(cond, ...) VN_REQUIRE_IN(::votenet::g_ib_err, cond, __VA_ARGS__)

constexpr int IB_MAX_B = 65535;     // scenes: the grid's y extent
constexpr long IB_MAX_N = 1L << 24; // exclusive: ~index of a point stays above every empty (zero) entry
constexpr int IB_MAX_K = 1024;
constexpr int IB_MAX_SEM = 65536;
constexpr int IB_THREADS = 256;
constexpr int IB_PPT = 8; // points a lane folds
constexpr int IB_TILE = IB_THREADS * IB_PPT;
static_assert(IB_TILE == VOTENET_INSTANCE_BOXES_TILE, "the header states the tile");
// the fields of a table, k words each (a scene's table in the workspace and a workgroup's in LDS alike): lanes on consecutive ids touch
// consecutive words
enum { F_NLO = 0, F_HI = 3, F_COUNT = 6, F_NFIRST = 7, F_WORDS = 8 };
constexpr int IB_IGN = 4; // words per scene behind the tables: the three ignored counters, one of padding

inline size_t ib_table_bytes(int b, int k) { return align256((size_t)b * k * F_WORDS * sizeof(unsigned)); }
inline size_t ib_workspace_bytes(int b, int k) { return ib_table_bytes(b, k) + align256((size_t)b * IB_IGN * sizeof(unsigned)); }

// x + 0.0f of a finite x, on the bits: -0 becomes +0, everything else is itself (denormals too, whatever the float mode)
__device__ __forceinline__ unsigned plus_zero(unsigned u) { return u == 0x80000000u ? 0u : u; }
__device__ __forceinline__ bool finite_bits(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }
// order-preserving: a < b as floats  <=>  ordered(a) < ordered(b) as unsigned (no NaN, -0 already +0)
__device__ __forceinline__ unsigned ordered(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float unordered(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// A workgroup per (tile of IB_TILE points, scene).  Lane t folds points tile * IB_TILE + j * IB_THREADS + t, j < IB_PPT (coalesced
// rows).  An id is compared with k before it indexes the table.
__global__ __launch_bounds__(IB_THREADS) void instance_tile_kernel(long n, int k, const float *__restrict__ points,
                                                                   const int *__restrict__ instance, unsigned *__restrict__ tables,
                                                                   unsigned *__restrict__ ign)
{
    __shared__ unsigned s_tab[F_WORDS * IB_MAX_K]; // 32 bytes per id
    __shared__ unsigned s_ign[3];
    const int scene = blockIdx.y, tid = threadIdx.x;
    for (int w = tid; w < F_WORDS * k; w += IB_THREADS) s_tab[w] = 0u;
    if (tid < 3) s_ign[tid] = 0u;
    const float *__restrict__ pts = points + (size_t)scene * (size_t)n * 3;
    const int *__restrict__ ids = instance + (size_t)scene * (size_t)n;
    const long p0 = (long)blockIdx.x * IB_TILE + tid;
    int id[IB_PPT];
    unsigned x[IB_PPT], y[IB_PPT], z[IB_PPT];
#pragma unroll
    for (int j = 0; j < IB_PPT; j++) {
        const long p = p0 + j * IB_THREADS;
        const bool live = p < n;
        id[j] = live ? ids[p] : 0;
        x[j] = live ? __float_as_uint(pts[(size_t)p * 3 + 0]) : 0u;
        y[j] = live ? __float_as_uint(pts[(size_t)p * 3 + 1]) : 0u;
        z[j] = live ? __float_as_uint(pts[(size_t)p * 3 + 2]) : 0u;
    }
    __syncthreads();
    unsigned unlabelled = 0, outside = 0, nonfinite = 0;
#pragma unroll
    for (int j = 0; j < IB_PPT; j++) {
        const long p = p0 + j * IB_THREADS;
        if (p >= n) continue;
        if (id[j] < 0) {
            unlabelled++;
        } else if (id[j] >= k) {
            outside++;
        } else if (!(finite_bits(x[j]) && finite_bits(y[j]) && finite_bits(z[j]))) {
            nonfinite++;
        } else {
            unsigned *e = s_tab + id[j]; // 0 <= id < k
            const unsigned ox = ordered(plus_zero(x[j])), oy = ordered(plus_zero(y[j])), oz = ordered(plus_zero(z[j]));
            atomicMax(e + (F_NLO + 0) * k, ~ox);
            atomicMax(e + (F_NLO + 1) * k, ~oy);
            atomicMax(e + (F_NLO + 2) * k, ~oz);
            atomicMax(e + (F_HI + 0) * k, ox);
            atomicMax(e + (F_HI + 1) * k, oy);
            atomicMax(e + (F_HI + 2) * k, oz);
            atomicAdd(e + F_COUNT * k, 1u);
            atomicMax(e + F_NFIRST * k, ~(unsigned)p);
        }
    }
    if (unlabelled) atomicAdd(&s_ign[0], unlabelled);
    if (outside) atomicAdd(&s_ign[1], outside);
    if (nonfinite) atomicAdd(&s_ign[2], nonfinite);
    __syncthreads();
    // the flush: only the entries this tile has met
    unsigned *__restrict__ g = tables + (size_t)scene * F_WORDS * k;
    for (int i = tid; i < k; i += IB_THREADS) {
        const unsigned c = s_tab[F_COUNT * k + i];
        if (c == 0u) continue;
#pragma unroll
        for (int f = 0; f < F_COUNT; f++) atomicMax(g + f * k + i, s_tab[f * k + i]);
        atomicAdd(g + F_COUNT * k + i, c);
        atomicMax(g + F_NFIRST * k + i, s_tab[F_NFIRST * k + i]);
    }
    if (tid < 3 && s_ign[tid] != 0u) atomicAdd(ign + (size_t)scene * IB_IGN + tid, s_ign[tid]);
}

struct FinishArgs {
    long n;
    int k, n_sem, n_class, min_points;
    const int *semantic, *class_map;
    const unsigned *tables, *ign;
};

// status, count and class of id i of scene sc.  first is compared with n before semantic is read, the label with n_sem before class_map.
__device__ __forceinline__ int instance_status(const FinishArgs &a, int sc, int i, int &count, int &cls)
{
    const unsigned *__restrict__ g = a.tables + (size_t)sc * F_WORDS * a.k;
    count = (int)g[F_COUNT * a.k + i];
    cls = -1;
    if (count == 0) return 3;
    const unsigned first = ~g[F_NFIRST * a.k + i];
    const int sem = (long)first < a.n ? a.semantic[(size_t)sc * (size_t)a.n + first] : -1;
    if (sem >= 0 && sem < a.n_sem) cls = a.class_map[sem];
    if (cls < 0 || cls >= a.n_class) cls = -1;
    if (cls < 0) return 1;
    return count < a.min_points ? 2 : 0;
}

// A workgroup per scene, thread i for id i (the block is k rounded up to whole waves).  The rows of the scenes before this one are
// counted here, from the same tables: no workgroup waits for another.  Positions inside the scene: ballot / popcount per wave, the
// waves' totals through LDS.
__global__ __launch_bounds__(IB_MAX_K) void instance_finish_kernel(FinishArgs a, double *__restrict__ center, double *__restrict__ size,
                                                                   double *__restrict__ heading, int *__restrict__ cls_out,
                                                                   int *__restrict__ instance_id, int *__restrict__ n_points,
                                                                   int *__restrict__ kept, int *__restrict__ slot,
                                                                   int *__restrict__ status, int *__restrict__ inst_count,
                                                                   int *__restrict__ ignored)
{
    __shared__ int s_wave[IB_MAX_K / 64];
    __shared__ int s_before;
    const int scene = blockIdx.x, i = threadIdx.x, lane = i & 63, wave = i >> 6, waves = (int)(blockDim.x >> 6);
    const bool live = i < a.k;
    if (i == 0) s_before = 0;
    __syncthreads();
    int count = 0, cls = -1, before = 0;
    if (live)
        for (int sp = 0; sp < scene; sp++) before += instance_status(a, sp, i, count, cls) == 0 ? 1 : 0;
    if (before) atomicAdd(&s_before, before);
    const int st = live ? instance_status(a, scene, i, count, cls) : 3;
    const bool keep = live && st == 0;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int pos = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < waves; w++) {
        const int c = s_wave[w];
        pos += w < wave ? c : 0;
        total += c;
    }
    if (i == 0) kept[scene] = total;
    if (i < 3) ignored[(size_t)scene * 3 + i] = (int)a.ign[(size_t)scene * IB_IGN + i];
    if (!live) return;
    const size_t o = (size_t)scene * a.k + i;
    status[o] = st;
    inst_count[o] = count;
    slot[o] = keep ? pos : -1;
    if (!keep) return;
    const unsigned *__restrict__ g = a.tables + (size_t)scene * F_WORDS * a.k;
    const size_t row = (size_t)s_before + (size_t)pos;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double lo = (double)unordered(~g[(F_NLO + d) * a.k + i]), hi = (double)unordered(g[(F_HI + d) * a.k + i]);
        center[row * 3 + d] = (lo + hi) * 0.5;
        size[row * 3 + d] = hi - lo;
    }
    heading[row] = 0.0;
    cls_out[row] = cls;
    instance_id[row] = i;
    n_points[row] = count;
}

__global__ __launch_bounds__(256) void instance_point_box_kernel(long n, int k, const float *__restrict__ points,
                                                                 const int *__restrict__ instance, const int *__restrict__ slot,
                                                                 int *__restrict__ point_box)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int scene = blockIdx.y;
    const size_t o = (size_t)scene * (size_t)n + (size_t)p;
    const int id = instance[o];
    int row = -1;
    if (id >= 0 && id < k) {
        const float *__restrict__ q = points + o * 3;
        if (finite_bits(__float_as_uint(q[0])) && finite_bits(__float_as_uint(q[1])) && finite_bits(__float_as_uint(q[2])))
            row = slot[(size_t)scene * k + id];
    }
    point_box[o] = row;
}

static int check_limits(const char *who, int b, long n, int k)
{
    IB_REQUIRE(b >= 1 && b <= IB_MAX_B, "%s: batch must be in [1, %d], got %d", who, IB_MAX_B, b);
    IB_REQUIRE(n >= 1 && n < IB_MAX_N, "%s: points per scene must be in [1, 2^24), got n = %ld", who, n);
    IB_REQUIRE(k >= 1 && k <= IB_MAX_K, "%s: the instance id table holds 1 to %d entries, got k = %d", who, IB_MAX_K, k);
    return VOTENET_OK;
}

} // namespace votenet

using namespace votenet;

extern "C" const char *votenet_instance_boxes_last_error(void) { return g_ib_err.text; }

extern "C" size_t votenet_instance_boxes_workspace_bytes(int b, int k)
{
    if (b < 1 || b > IB_MAX_B || k < 1 || k > IB_MAX_K) return 0;
    return ib_workspace_bytes(b, k);
}

extern "C" int votenet_instance_boxes(int b, long n, int k, int n_sem, int n_class, int min_points, const float *points,
                                      const int *instance, const int *semantic, const int *class_map, double *center, double *size,
                                      double *heading, int *cls, int *instance_id, int *n_points, int *kept, int *slot, int *status,
                                      int *inst_count, int *ignored, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_limits("instance_boxes", b, n, k)) return rc;
    IB_REQUIRE(n_sem >= 1 && n_sem <= IB_MAX_SEM, "instance_boxes: class_map holds 1 to %d labels, got n_sem = %d", IB_MAX_SEM, n_sem);
    IB_REQUIRE(min_points >= 1, "instance_boxes: min_points must be >= 1, got %d", min_points);
    IB_REQUIRE(points && instance && semantic && class_map, "instance_boxes: null points, instance, semantic or class_map");
    IB_REQUIRE(center && size && heading && cls && instance_id && n_points, "instance_boxes: null row output");
    IB_REQUIRE(kept && slot && status && inst_count && ignored, "instance_boxes: null kept, slot, status, inst_count or ignored");
    const size_t need = ib_workspace_bytes(b, k);
    IB_REQUIRE(workspace && workspace_bytes >= need, "instance_boxes: workspace of %zu bytes needed, got %zu", need, workspace_bytes);
    IB_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "instance_boxes: workspace must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned *tables = static_cast<unsigned *>(workspace);
    unsigned *ign = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + ib_table_bytes(b, k));
    if (int rc = g_ib_err.check(hipMemsetAsync(workspace, 0, need, st), "instance_boxes (memset)")) return rc;
    const unsigned tiles = (unsigned)((n + IB_TILE - 1) / IB_TILE); // <= 2^13
    hipLaunchKernelGGL(instance_tile_kernel, dim3(tiles, b), dim3(IB_THREADS), 0, st, n, k, points, instance, tables, ign);
    if (int rc = g_ib_err.check_launch("instance_boxes (tile pass)")) return rc;
    const FinishArgs a = {n, k, n_sem, n_class, min_points, semantic, class_map, tables, ign};
    hipLaunchKernelGGL(instance_finish_kernel, dim3(b), dim3((k + 63) / 64 * 64), 0, st, a, center, size, heading, cls, instance_id,
                       n_points, kept, slot, status, inst_count, ignored);
    return g_ib_err.check_launch("instance_boxes (finish)");
}

extern "C" int votenet_instance_point_box(int b, long n, int k, const float *points, const int *instance, const int *slot,
                                          int *point_box, void *stream)
{
    if (int rc = check_limits("instance_point_box", b, n, k)) return rc;
    IB_REQUIRE(points && instance && slot && point_box, "instance_point_box: null points, instance, slot or point_box");
    hipLaunchKernelGGL(instance_point_box_kernel, dim3((unsigned)((n + 255) / 256), b), dim3(256), 0, as_stream(stream), n, k, points,
                       instance, slot, point_box);
    return g_ib_err.check_launch("instance_point_box");
}
