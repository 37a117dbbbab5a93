// augment_points.h -- the device text of the input pipeline's point step, shared by libvotenet_hip.so (augment.hip:
// votenet_subsample_augment) and libvotenet_features.so (features/point_features.hip: votenet_subsample_augment_features), so that
// both write the same points bit for bit: the row draw, the double-precision transform in the reference's order, one rounding to float.
#pragma once
#include "common.h"
#include <cstdio>

namespace votenet {

constexpr int AUG_CHUNK = 16; // scenes per launch: their parameters travel as kernel arguments

struct AugScenes {
    long off[AUG_CHUNK + 1];
    double c[AUG_CHUNK], s[AUG_CHUNK], scale[AUG_CHUNK], angle[AUG_CHUNK];
    int flip[AUG_CHUNK];
    unsigned key[AUG_CHUNK];
};

// FEATS: the same rows also carry `extra` raw columns behind xyz into feats (b, n_out, c) at column h0 (= want_height: column 0 is
// the height, written by floor_height_kernel below); one rounding to float, no augmentation.  The points are the same text either way.
template <typename T, bool FEATS>
__global__ __launch_bounds__(256) void subsample_augment_kernel(AugScenes P, int n_out, const T *__restrict__ raw, int stride,
                                                                const int *__restrict__ choice, int to_camera, int train,
                                                                float *__restrict__ out, float *__restrict__ feats, int c, int h0,
                                                                int extra)
{
    const int sc = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_out) return;
    const long n = P.off[sc + 1] - P.off[sc];
    long i;
    if (choice) {
        i = choice[(long)sc * n_out + j];
        i = i < 0 ? 0 : (i >= n ? n - 1 : i); // validated on the host side of the Python mirror; never read out of range
    } else {
        int bits = 2;
        while ((1ll << bits) < n) bits += 2;
        i = feistel_perm(j, n, P.key[sc], bits >> 1);
    }
    const T *p = raw + (P.off[sc] + i) * stride;
    double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    if (to_camera) { // sunutils.py:70-77: (x, y, z) -> (x, -z, y)
        const double t = y;
        y = -z;
        z = t;
    }
    if (train) {
        if (P.flip[sc] & 1) x = -x; // dataset.py:303-306
        if (P.flip[sc] & 2) z = -z;
        const double c = P.c[sc], s = P.s[sc];
        const double xr = c * x + s * z; // roty(a) @ p, sunutils.py:133-139
        const double zr = -s * x + c * z;
        x = xr * P.scale[sc]; // dataset.py:308
        y = y * P.scale[sc];
        z = zr * P.scale[sc];
    }
    float *o = out + ((long)sc * n_out + j) * 3;
    o[0] = (float)x;
    o[1] = (float)y;
    o[2] = (float)z;
    if (FEATS) {
        float *f = feats + ((long)sc * n_out + j) * c + h0;
        for (int e = 0; e < extra; e++) f[e] = (float)p[3 + e];
    }
}

// The argument checks of both point entries (`what` names the entry): true, or false with the message in msg.
inline bool points_args_ok(const char *what, int b, int n_out, const void *raw, int raw_stride, const long *raw_offset, const int *flip,
                           const double *rot_cos, const double *rot_sin, const double *scale, const float *out, char *msg, size_t cap)
{
#define VN_POINTS_REQUIRE(cond, ...)        \
    do {                                    \
        if (!(cond)) {                      \
            snprintf(msg, cap, __VA_ARGS__); \
            return false;                   \
        }                                   \
    } while (0)
    VN_POINTS_REQUIRE(b > 0 && n_out > 0, "%s: b and n_out must be positive, got %d, %d", what, b, n_out);
    VN_POINTS_REQUIRE(raw && raw_offset && out, "%s: null pointer", what);
    VN_POINTS_REQUIRE(raw_stride >= 3, "%s: raw rows need at least 3 elements, got %d", what, raw_stride);
    VN_POINTS_REQUIRE(!flip || (rot_cos && rot_sin && scale), "%s: flip given without rot_cos / rot_sin / scale", what);
    for (int s = 0; s < b; s++) {
        const long n = raw_offset[s + 1] - raw_offset[s];
        VN_POINTS_REQUIRE(n >= n_out, "%s: scene %d has %ld points, cannot take %d without replacement", what, s, n, n_out);
        VN_POINTS_REQUIRE(n < (1l << 31), "%s: scene %d has %ld points (limit 2^31)", what, s, n);
    }
#undef VN_POINTS_REQUIRE
    return true;
}

// The gather / transform launches (one per AUG_CHUNK scenes); feats != NULL: they also carry `extra` raw columns into
// feats (b, n_out, c) from column h0 on.
inline void launch_points(int b, int n_out, const void *raw, int raw_f64, int raw_stride, const long *raw_offset, const int *choice,
                          unsigned long long seed, long scene0, int depth_to_camera, const int *flip, const double *rot_cos,
                          const double *rot_sin, const double *scale, float *out, float *feats, int c, int h0, int extra, hipStream_t st)
{
    for (int s0 = 0; s0 < b; s0 += AUG_CHUNK) {
        const int ns = b - s0 < AUG_CHUNK ? b - s0 : AUG_CHUNK;
        AugScenes P = {};
        for (int s = 0; s < ns; s++) {
            P.off[s] = raw_offset[s0 + s];
            P.off[s + 1] = raw_offset[s0 + s + 1];
            P.key[s] = scene_key(seed, scene0 + s0 + s);
            if (flip) {
                P.flip[s] = flip[s0 + s];
                P.c[s] = rot_cos[s0 + s];
                P.s[s] = rot_sin[s0 + s];
                P.scale[s] = scale[s0 + s];
            }
        }
        const dim3 grid((n_out + 255) / 256, ns);
        const int *ch = choice ? choice + (long)s0 * n_out : nullptr;
        float *o = out + (long)s0 * n_out * 3;
        float *f = feats ? feats + (long)s0 * n_out * c : nullptr;
        const int train = flip ? 1 : 0;
        if (raw_f64 && feats)
            hipLaunchKernelGGL((subsample_augment_kernel<double, true>), grid, dim3(256), 0, st, P, n_out, (const double *)raw,
                               raw_stride, ch, depth_to_camera, train, o, f, c, h0, extra);
        else if (raw_f64)
            hipLaunchKernelGGL((subsample_augment_kernel<double, false>), grid, dim3(256), 0, st, P, n_out, (const double *)raw,
                               raw_stride, ch, depth_to_camera, train, o, nullptr, 0, 0, 0);
        else if (feats)
            hipLaunchKernelGGL((subsample_augment_kernel<float, true>), grid, dim3(256), 0, st, P, n_out, (const float *)raw,
                               raw_stride, ch, depth_to_camera, train, o, f, c, h0, extra);
        else
            hipLaunchKernelGGL((subsample_augment_kernel<float, false>), grid, dim3(256), 0, st, P, n_out, (const float *)raw,
                               raw_stride, ch, depth_to_camera, train, o, nullptr, 0, 0, 0);
    }
}

} // namespace votenet
