// select_boxes.hip -- which labelled objects of a scene become ground truth (dataset.py:237-283,300).  For every object the
// reference projects the subsampled cloud into the image, keeps the points inside the object's 2D box, builds the eight
// corners of the 3D box (sunutils.py:212-241), and counts the frustum points inside their hull with one scipy Delaunay
// triangulation per object; the object trains iff it is whitelisted, its corners span at least 1e-7 in y and at least 5
// points are inside.  Here: one launch over (scene, 256 points), every lane holds one gathered row and its pixel, the
// scene's boxes sit in LDS, one ballot + popcount per wavefront and object, integer atomics only (the counts, and so every
// output, do not depend on scheduling); a second one-wavefront launch decides and compacts.  Arithmetic is double
// precision, un-fused, in the reference's order.  The hull test is the closed analytic one, |R^T (p - c)| <= (l, w, h).
#include "common.h"

namespace votenet {

constexpr int SEL_CHUNK = 8;  // scenes per launch: their calibrations travel as kernel arguments
constexpr int SEL_PASS = 64;  // objects derived into LDS at a time; a scene with more takes several passes
constexpr int SEL_MIN_POINTS = 5; // dataset.py:283

struct SelScenes {
    long raw_off[SEL_CHUNK + 1], obj_off[SEL_CHUNK + 1];
    double R[SEL_CHUNK][9], K[SEL_CHUNK][9]; // row-major Rtilt and K (sunutils.py:59-64)
    unsigned key[SEL_CHUNK];
};

struct SelObjects {
    const int *cls;
    const double *box2d, *centroid, *half_extent, *heading;
};

// what the label says about one box: rotz(-heading) entries, the y span of the eight corners and the centre the
// reference reports, (corner0 + corner6) / 2, both in the upright-camera frame (x, -z, y)
struct BoxGeom {
    double c, s, span_y, center[3];
};

__device__ __forceinline__ BoxGeom box_geometry(const double *cen, const double *ext, double heading)
{
    BoxGeom g;
    const double t = -1 * heading; // sunutils.py:222
    g.c = cos(t);
    g.s = sin(t);
    const double R[3][3] = {{g.c, -g.s, 0.0}, {g.s, g.c, 0.0}, {0.0, 0.0, 1.0}}; // rotz, sunutils.py:142-148
    const double l = ext[0], w = ext[1], h = ext[2];
    const double xs[8] = {-l, l, l, -l, -l, l, l, -l}; // sunutils.py:232-234
    const double ys[8] = {w, w, -w, -w, w, w, -w, -w};
    const double zs[8] = {h, h, h, h, -h, -h, -h, -h};
    double ymin = 0, ymax = 0, c0[3] = {0, 0, 0}, c6[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; a++) p[a] = (R[a][0] * xs[k] + R[a][1] * ys[k] + R[a][2] * zs[k]) + cen[a];
        const double cam[3] = {p[0], -p[2], p[1]}; // flip_axis_to_camera, sunutils.py:70-77
        if (k == 0 || cam[1] < ymin) ymin = cam[1];
        if (k == 0 || cam[1] > ymax) ymax = cam[1];
        if (k == 0) c0[0] = cam[0], c0[1] = cam[1], c0[2] = cam[2];
        if (k == 6) c6[0] = cam[0], c6[1] = cam[1], c6[2] = cam[2];
    }
    g.span_y = ymax - ymin;
#pragma unroll
    for (int a = 0; a < 3; a++) g.center[a] = (c0[a] + c6[a]) / 2; // dataset.py:259
    return g;
}

template <typename T>
__global__ __launch_bounds__(256) void select_count_kernel(SelScenes P, int n_out, const T *__restrict__ raw, int stride,
                                                           const int *__restrict__ choice, SelObjects O, int scene_base,
                                                           int *__restrict__ n_inside, int *__restrict__ obj_scene,
                                                           unsigned char *__restrict__ inside)
{
    __shared__ double s_box[SEL_PASS][12]; // c, s, centroid, |half extents|, xmin, ymin, xmax, ymax
    __shared__ int s_skip[SEL_PASS], s_cnt[SEL_PASS];
    const int sc = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const bool valid = j < n_out;
    double x = 0, y = 0, z = 0, u = 0, v = 0;
    if (valid) {
        const long n = P.raw_off[sc + 1] - P.raw_off[sc];
        long i;
        if (choice) {
            i = choice[(long)sc * n_out + j];
            i = i < 0 ? 0 : (i >= n ? n - 1 : i); // validated on the host side of the Python mirror; never read out of range
        } else {
            int bits = 2;
            while ((1ll << bits) < n) bits += 2;
            i = feistel_perm(j, n, P.key[sc], bits >> 1);
        }
        const T *p = raw + (P.raw_off[sc] + i) * stride;
        x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const double *R = P.R[sc], *K = P.K[sc];
        // project_upright_depth_to_image, sunutils.py:85-99: R^T p, (x, y, z) -> (x, -z, y), K p_cam, divide by the depth
        const double d0 = R[0] * x + R[3] * y + R[6] * z;
        const double d1 = R[1] * x + R[4] * y + R[7] * z;
        const double d2 = R[2] * x + R[5] * y + R[8] * z;
        const double c0 = d0, c1 = -d2, c2 = d1;
        const double uv0 = K[0] * c0 + K[1] * c1 + K[2] * c2;
        const double uv1 = K[3] * c0 + K[4] * c1 + K[5] * c2;
        const double uv2 = K[6] * c0 + K[7] * c1 + K[8] * c2;
        u = uv0 / uv2;
        v = uv1 / uv2;
    }
    const long o0 = P.obj_off[sc], o1 = P.obj_off[sc + 1];
    for (long base = o0; base < o1; base += SEL_PASS) {
        const int np = o1 - base < SEL_PASS ? (int)(o1 - base) : SEL_PASS;
        if ((int)threadIdx.x < np) {
            const int t = threadIdx.x;
            const long o = base + t;
            const BoxGeom g = box_geometry(O.centroid + o * 3, O.half_extent + o * 3, O.heading[o]);
            s_box[t][0] = g.c;
            s_box[t][1] = g.s;
            for (int a = 0; a < 3; a++) {
                s_box[t][2 + a] = O.centroid[o * 3 + a];
                s_box[t][5 + a] = fabs(O.half_extent[o * 3 + a]);
            }
            for (int a = 0; a < 4; a++) s_box[t][8 + a] = O.box2d[o * 4 + a];
            s_skip[t] = (O.cls[o] < 0 || g.span_y < 1e-7) ? 1 : 0; // dataset.py:243,254
            s_cnt[t] = 0;
            if (blockIdx.x == 0) obj_scene[o] = scene_base + sc;
        }
        __syncthreads();
        for (int t = 0; t < np; t++) {
            bool in = false;
            if (!s_skip[t] && valid) {
                const double *B = s_box[t];
                // dataset.py:243-244 (half-open), then the box in its own axes: rotz(-heading)^T (p - centroid)
                const bool fov = (u < B[10]) & (u >= B[8]) & (v < B[11]) & (v >= B[9]);
                const double dx = x - B[2], dy = y - B[3], dz = z - B[4];
                const double lx = B[0] * dx + B[1] * dy;
                const double ly = -B[1] * dx + B[0] * dy;
                in = fov & (fabs(lx) <= B[5]) & (fabs(ly) <= B[6]) & (fabs(dz) <= B[7]);
            }
            const unsigned long long m = __ballot(in);
            if (m && lane_id() == 0) atomicAdd(&s_cnt[t], __popcll(m));
            if (inside && valid) inside[(base + t) * (long)n_out + j] = in ? 1 : 0;
        }
        __syncthreads();
        if ((int)threadIdx.x < np && s_cnt[threadIdx.x]) atomicAdd(&n_inside[base + threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads(); // the next pass overwrites s_box / s_cnt
    }
}

struct SelOut {
    double *center, *size, *heading;
    int *cls, *kept_count, *status;
};

// one wavefront walks the objects in label order: status, and the kept ones compacted behind a running count
__global__ __launch_bounds__(64) void select_compact_kernel(long n_obj, SelObjects O, const int *__restrict__ n_inside,
                                                            const int *__restrict__ obj_scene, SelOut Q)
{
    long kept = 0;
    for (long base = 0; base < n_obj; base += 64) {
        const long o = base + lane_id();
        int st = -1;
        BoxGeom g = {};
        if (o < n_obj) {
            g = box_geometry(O.centroid + o * 3, O.half_extent + o * 3, O.heading[o]);
            st = O.cls[o] < 0 ? 1 : (g.span_y < 1e-7 ? 2 : (n_inside[o] < SEL_MIN_POINTS ? 3 : 0));
            Q.status[o] = st;
        }
        const unsigned long long m = __ballot(st == 0);
        if (st == 0) {
            const long q = kept + __popcll(m & ((1ull << lane_id()) - 1ull));
            for (int a = 0; a < 3; a++) {
                Q.center[q * 3 + a] = g.center[a];
                Q.size[q * 3 + a] = 2 * O.half_extent[o * 3 + a]; // dataset.py:258
            }
            Q.heading[q] = O.heading[o];
            Q.cls[q] = O.cls[o];
            atomicAdd(&Q.kept_count[obj_scene[o]], 1);
        }
        kept += __popcll(m);
    }
}

} // namespace votenet

using namespace votenet;

extern "C" size_t votenet_select_boxes_workspace_bytes(int b, long n_obj)
{
    (void)b;
    return (size_t)(n_obj > 0 ? n_obj : 1) * sizeof(int); // the scene of every object
}

extern "C" int votenet_select_boxes(int b, int n_out, const void *raw, int raw_f64, int raw_stride, const long *raw_offset,
                                    const int *choice, unsigned long long seed, long scene0, const double *rtilt,
                                    const double *kmat, const long *obj_offset, const int *cls, const double *box2d,
                                    const double *centroid, const double *half_extent, const double *heading, double *center,
                                    double *size, double *heading_out, int *cls_out, int *kept_count, int *n_inside,
                                    int *status, unsigned char *inside, void *workspace, size_t workspace_bytes, void *stream)
{
    VN_REQUIRE(b > 0 && n_out > 0, "select_boxes: b and n_out must be positive, got %d, %d", b, n_out);
    VN_REQUIRE(raw && raw_offset && rtilt && kmat && obj_offset && kept_count, "select_boxes: null pointer");
    VN_REQUIRE(raw_stride >= 3, "select_boxes: raw rows need at least 3 elements, got %d", raw_stride);
    for (int s = 0; s < b; s++) {
        const long n = raw_offset[s + 1] - raw_offset[s];
        VN_REQUIRE(n >= n_out, "select_boxes: scene %d has %ld points, cannot take %d without replacement", s, n, n_out);
        VN_REQUIRE(n < (1l << 31), "select_boxes: scene %d has %ld points (limit 2^31)", s, n);
        VN_REQUIRE(obj_offset[s + 1] >= obj_offset[s], "select_boxes: obj_offset decreases at scene %d", s);
    }
    VN_REQUIRE(obj_offset[0] == 0, "select_boxes: obj_offset must start at 0, got %ld", obj_offset[0]);
    const long n_obj = obj_offset[b];
    if (n_obj > 0) {
        VN_REQUIRE(cls && box2d && centroid && half_extent && heading, "select_boxes: null object pointer");
        VN_REQUIRE(center && size && heading_out && cls_out && n_inside && status, "select_boxes: null output pointer");
        VN_REQUIRE(workspace && workspace_bytes >= votenet_select_boxes_workspace_bytes(b, n_obj),
                   "select_boxes: workspace of %zu bytes, need %zu", workspace_bytes, votenet_select_boxes_workspace_bytes(b, n_obj));
    }
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(kept_count, 0, (size_t)b * sizeof(int), st) != hipSuccess) return check_launch("select_boxes");
    if (n_obj == 0) return check_launch("select_boxes");
    if (hipMemsetAsync(n_inside, 0, (size_t)n_obj * sizeof(int), st) != hipSuccess) return check_launch("select_boxes");
    int *obj_scene = (int *)workspace;
    const SelObjects O = {cls, box2d, centroid, half_extent, heading};
    for (int s0 = 0; s0 < b; s0 += SEL_CHUNK) {
        const int ns = b - s0 < SEL_CHUNK ? b - s0 : SEL_CHUNK;
        if (obj_offset[s0 + ns] == obj_offset[s0]) continue; // nothing labelled in these scenes
        SelScenes P = {};
        for (int s = 0; s < ns; s++) {
            P.raw_off[s] = raw_offset[s0 + s];
            P.raw_off[s + 1] = raw_offset[s0 + s + 1];
            P.obj_off[s] = obj_offset[s0 + s];
            P.obj_off[s + 1] = obj_offset[s0 + s + 1];
            P.key[s] = scene_key(seed, scene0 + s0 + s);
            for (int a = 0; a < 9; a++) {
                P.R[s][a] = rtilt[(long)(s0 + s) * 9 + a];
                P.K[s][a] = kmat[(long)(s0 + s) * 9 + a];
            }
        }
        const dim3 grid((n_out + 255) / 256, ns);
        const int *ch = choice ? choice + (long)s0 * n_out : nullptr;
        if (raw_f64)
            hipLaunchKernelGGL(select_count_kernel<double>, grid, dim3(256), 0, st, P, n_out, (const double *)raw, raw_stride, ch,
                               O, s0, n_inside, obj_scene, inside);
        else
            hipLaunchKernelGGL(select_count_kernel<float>, grid, dim3(256), 0, st, P, n_out, (const float *)raw, raw_stride, ch, O,
                               s0, n_inside, obj_scene, inside);
    }
    const SelOut Q = {center, size, heading_out, cls_out, kept_count, status};
    hipLaunchKernelGGL(select_compact_kernel, dim3(1), dim3(64), 0, st, n_obj, O, n_inside, obj_scene, Q);
    return check_launch("select_boxes");
}
