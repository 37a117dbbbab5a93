// iou3d.h -- rotated-box 3D IoU of one ordered pair of corner boxes (tf_nms3d.cpp:43-192), shared by the NMS / IoU-table kernels
// (nms3d.hip) and the detection matcher (eval_match.hip): one definition, so the overlaps of the two files are bit-equal.
#pragma once
#include "common.h"

namespace votenet {

struct P2 {
    float x, z;
};

// tf_nms3d.cpp:43-46
__device__ __forceinline__ float box_area2d(const float *bb)
{
    return sqrtf((bb[0] - bb[3]) * (bb[0] - bb[3]) + (bb[2] - bb[5]) * (bb[2] - bb[5])) *
           sqrtf((bb[3] - bb[6]) * (bb[3] - bb[6]) + (bb[5] - bb[8]) * (bb[5] - bb[8]));
}
// tf_nms3d.cpp:48-50
__device__ __forceinline__ float box_area3d(const float *bb) { return box_area2d(bb) * (bb[1] - bb[13]); }

// tf_nms3d.cpp:53-67 : even-odd ray test against the first four corners
__device__ __forceinline__ bool point_in_quad(float px, float pz, const float *poly)
{
    bool result = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int j = (i + 3) & 3;
        const float xi = poly[i * 3], zi = poly[i * 3 + 2], xj = poly[j * 3], zj = poly[j * 3 + 2];
        if ((zi > pz) != (zj > pz) && (px < (xj - xi) * (pz - zi) / (zj - zi) + xi)) result = !result;
    }
    return result;
}

// tf_nms3d.cpp:69-100
__device__ __forceinline__ bool seg_intersect(float ax, float az, float bx, float bz, float cx, float cz, float dx,
                                              float dz, P2 *out)
{
    const double A1 = (double)(bz - az);
    const double B1 = (double)(ax - bx);
    const double C1 = A1 * (double)ax + B1 * (double)az;
    const double A2 = (double)(dz - cz);
    const double B2 = (double)(cx - dx);
    const double C2 = A2 * (double)cx + B2 * (double)cz;
    const double det = A1 * B2 - A2 * B1;
    if (fabs(det) < 1e-7) return false;
    const double x = (B2 * C1 - B1 * C2) / det;
    const double z = (A1 * C2 - A2 * C1) / det;
    const bool on1 = ((double)fminf(ax, bx) <= x) && ((double)fmaxf(ax, bx) >= x) && ((double)fminf(az, bz) <= z) &&
                     ((double)fmaxf(az, bz) >= z);
    const bool on2 = ((double)fminf(cx, dx) <= x) && ((double)fmaxf(cx, dx) >= x) && ((double)fminf(cz, dz) <= z) &&
                     ((double)fmaxf(cz, dz) >= z);
    if (on1 && on2) {
        out->x = (float)x;
        out->z = (float)z;
        return true;
    }
    return false;
}

// tf_nms3d.cpp:122-175 : at most 4 + 4 + 16 vertices
__device__ float bev_intersection(const float *b1, const float *b2)
{
    P2 cc[24];
    float ang[24];
    int nc = 0;
    for (int i = 0; i < 4; i++)
        if (point_in_quad(b1[i * 3], b1[i * 3 + 2], b2)) {
            cc[nc].x = b1[i * 3];
            cc[nc].z = b1[i * 3 + 2];
            nc++;
        }
    for (int i = 0; i < 4; i++)
        if (point_in_quad(b2[i * 3], b2[i * 3 + 2], b1)) {
            cc[nc].x = b2[i * 3];
            cc[nc].z = b2[i * 3 + 2];
            nc++;
        }
    for (int i = 0; i < 4; i++) {
        const int nx = (i + 1) & 3;
        for (int e = 0; e < 4; e++) {
            const int en = (e + 1) & 3;
            P2 ip;
            if (seg_intersect(b1[i * 3], b1[i * 3 + 2], b1[nx * 3], b1[nx * 3 + 2], b2[e * 3], b2[e * 3 + 2], b2[en * 3],
                              b2[en * 3 + 2], &ip)) {
                cc[nc] = ip;
                nc++;
            }
        }
    }
    if (nc == 0) return 0.0f; // reference: 0/0 centroid, both loops skipped, area 0
    float mx = 0, mz = 0;
    for (int i = 0; i < nc; i++) {
        mx += cc[i].x;
        mz += cc[i].z;
    }
    mx /= (float)nc;
    mz /= (float)nc;
    for (int i = 0; i < nc; i++) ang[i] = atan2f(cc[i].z - mz, cc[i].x - mx);
    // insertion sort by angle (what std::sort does for <= 16 elements; stable)
    for (int i = 1; i < nc; i++) {
        const P2 p = cc[i];
        const float a = ang[i];
        int j = i - 1;
        while (j >= 0 && a < ang[j]) {
            cc[j + 1] = cc[j];
            ang[j + 1] = ang[j];
            j--;
        }
        cc[j + 1] = p;
        ang[j + 1] = a;
    }
    float area = 0;
    for (int i = 0, j = nc - 1; i < nc; j = i++)
        area += fabsf((mx * (cc[i].z - cc[j].z) + cc[i].x * (cc[j].z - mz) + cc[j].x * (mz - cc[i].z)) / 2);
    return area;
}

// tf_nms3d.cpp:178-192
__device__ float iou3d_pair(const float *bi, const float *bj)
{
    const float inter2d = bev_intersection(bi, bj);
    const float top = fminf(bi[1], bj[1]);
    const float bot = fmaxf(bi[13], bj[13]);
    const float h = (top - bot) > 0.0f ? (top - bot) : 0.0f;
    const float inter3d = h * inter2d;
    return inter3d / (box_area3d(bi) + box_area3d(bj) - inter3d);
}

} // namespace votenet
