// scene_fold.h -- the end of a kernel of one workgroup per scene that needs K sums over ALL scenes added in ONE fixed order, whatever
// order the workgroups finish in: the one text of paper_vote_loss_kernel (votesup/, K = 1) and paper_proposal_loss_kernel (propsup/, 3).
// The workspace: SCENE_FOLD_INTS ints, the ticket first, then K floats per scene.  Zero on entry, zero again when the launch is over.
#pragma once
#include "common.h"

namespace votenet {

constexpr int SCENE_FOLD_INTS = 4; // [ticket, pad x 3]
constexpr size_t scene_fold_bytes(int b, int k) { return (SCENE_FOLD_INTS + (size_t)(b > 0 ? b : 0) * k) * sizeof(float); }

// Called by ONE thread of the workgroup of scene `own` (of b) with that scene's sums v.  -> whether this workgroup was the last to
// arrive; only then total holds the sums over scenes 0 .. b-1, added in ascending scene order, and workspace and ticket are zero again.
template <int K>
__device__ __forceinline__ bool scene_fold(int *ticket, int own, int b, const float (&v)[K], float (&total)[K])
{
    float *sums = reinterpret_cast<float *>(ticket + SCENE_FOLD_INTS);
    for (int k = 0; k < K; k++) __hip_atomic_store(&sums[(size_t)own * K + k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence(); // the scene's sums are visible device-wide before the ticket is taken
    if (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != b - 1) return false;
    __threadfence();
    for (int k = 0; k < K; k++) total[k] = 0.0f;
    for (int sc = 0; sc < b; sc++)
        for (int k = 0; k < K; k++) {
            total[k] += __hip_atomic_load(&sums[(size_t)sc * K + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sums[(size_t)sc * K + k], 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // the workspace is left zero
        }
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

} // namespace votenet
