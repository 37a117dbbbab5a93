// ball_threshold.h -- the ball query's hit threshold (host only).  The reference's test max(sqrtf(s),1e-20f) < r is evaluated on the
// device as s < T(r); every library that decides a ball-query hit (grouping.hip, votesamp/vote_sampling.hip) forms T with this text, so
// they agree on every hit.  tests/test_abi.py::test_ball_threshold_table pins it through votenet_ball_threshold.
#pragma once
#include <cmath>

namespace votenet {

// smallest fp32 T with sqrtf(T) >= r (host, correctly rounded sqrtf)
inline float ball_threshold(float r)
{
    float t = r * r;
    while (t > 0.0f && sqrtf(t) >= r) t = nextafterf(t, 0.0f);
    while (sqrtf(t) < r) t = nextafterf(t, INFINITY);
    return t;
}

} // namespace votenet
