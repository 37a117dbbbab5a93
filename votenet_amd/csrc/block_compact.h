// block_compact.h -- ordered compaction of one round of a workgroup's threads: the threads whose flag is set get consecutive slots of
// a list in LDS, in thread order, behind the slots of the rounds before.  One text for the kernels that build such a list
// (nms3d.hip, eval_match.hip, detect/detections.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace votenet {

// Called by ALL threads of a workgroup of WAVES wave64s.  s_wcnt: WAVES ints of LDS; s_len: the list's running length in LDS, set
// by the caller and visible (a barrier) before the first call.  Returns the slot of a thread with `mine` (what the others get is
// no slot) and advances *s_len by the round's count; a slot at or beyond the caller's array is the caller's to drop.  Three
// barriers: the counts, every thread has read the length, the new length.  On return every thread may read *s_len; what the
// callers write at their slots after the last round needs a barrier of the caller's before another thread reads it.
template <int WAVES>
__device__ __forceinline__ int block_compact(bool mine, int *s_wcnt, int *s_len)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) s_wcnt[w] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int i = 0; i < WAVES; i++) {
        if (i < w) woff += s_wcnt[i];
        tot += s_wcnt[i];
    }
    const int base = *s_len;
    __syncthreads();
    if (threadIdx.x == 0) *s_len = base + tot;
    __syncthreads();
    return base + woff + __popcll(bal & ((1ull << lane) - 1ull));
}

} // namespace votenet
