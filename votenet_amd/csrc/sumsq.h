// sumsq.h -- the optimizer's per-tensor sum of squares (seg_sumsq_kernel), shared by votenet_clip_adam (mlp_bwd.hip) and the guarded
// optimizer step of libvotenet_guard.so (guard/step_guard.hip): one text, so both form the same partial sums bit for bit.
// Include inside namespace votenet, after include/votenet_hip.h (VOTENET_SUMSQ_SLICES).
#pragma once
// sum of squares of every tensor's gradient segment: grid (kSumsqSlices slices, ntensors) -> out[tensor * kSumsqSlices + slice]; the
// optimizer adds the partials in slice order (no atomics: every data-parallel replica must compute bit-identical clip factors from
// the same all-reduced gradient, or the replicas drift apart).  32 slices and four loads in flight per thread: the largest tensors
// (512 x 256) bound the launch -- 27 -> see profiles (8 slices, one load at a time)
constexpr int kSumsqSlices = VOTENET_SUMSQ_SLICES;
__global__ __launch_bounds__(256) void seg_sumsq_kernel(const float *__restrict__ g, const long *__restrict__ seg,
                                                        float *__restrict__ out)
{
    __shared__ float sh[256];
    const long a = seg[2 * blockIdx.y], b = seg[2 * blockIdx.y + 1];
    const long step = 256L * gridDim.x;
    float s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    long i = a + (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * step < b; i += 4 * step) {
        const float v0 = g[i], v1 = g[i + step], v2 = g[i + 2 * step], v3 = g[i + 3 * step];
        s0 += v0 * v0;
        s1 += v1 * v1;
        s2 += v2 * v2;
        s3 += v3 * v3;
    }
    for (; i < b; i += step) s0 += g[i] * g[i];
    sh[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.y * kSumsqSlices + blockIdx.x] = sh[0];
}
