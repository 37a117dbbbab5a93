// nearest_box.h -- the proposal assignment of model.py:148-155, shared by the loss kernels (loss.hip) and the accuracy kernel
// (monitors/monitors.hip) so that both decide positives, negatives and the assigned box with the same instructions.
#pragma once
#include <hip/hip_runtime.h>

namespace votenet {

constexpr int LOSS_MAXBOX = 256; // boxes per scene

// nearest ground-truth centre of proposal (px,py,pz) among the scene's boxes staged in LDS: -> distance, box index
__device__ __forceinline__ float nearest_box(const float (*s_box)[8], int BB, float px, float py, float pz, int &g)
{
    float best = 0.0f;
    g = 0;
    for (int j = 0; j < BB; j++) {
        const float dx = px - s_box[j][0], dy = py - s_box[j][1], dz = pz - s_box[j][2];
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (j == 0 || d < best) { // tf.argmin: first minimum
            best = d;
            g = j;
        }
    }
    return best;
}

} // namespace votenet
