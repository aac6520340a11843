// The "squared distance to the nearest staged point" walk that points_min_dist_kernel (evalmetrics.hip) and pair_eval_warp_near_kernel
// (pair_eval.hip) share: the per-sample and the batched evaluation paths agree bit for bit because both run THIS loop.
//
// Arithmetic, as the reference's dist.float(): the difference of each coordinate in f64, cast to f32, then d0*d0 + d1*d1 in f32 (evaluated as
// written: the library is built with -ffp-contract=off) and fminf.  The caller takes sqrtf of the final minimum (sqrt is monotonic).  Each kernel
// keeps its own staging: S is what it staged, float (the list as given) or double (already widened); (double)s is exact for both.
#pragma once
#include "xp_common.h"

template <typename S, int TILE>
__device__ __forceinline__ float xp_near_walk(double q0, double q1, const S (&tile)[TILE][2], int n, float best) {
    for (int j = 0; j < n; ++j) {
        const float d0 = (float)(q0 - (double)tile[j][0]), d1 = (float)(q1 - (double)tile[j][1]);
        best = fminf(best, d0 * d0 + d1 * d1);
    }
    return best;
}
