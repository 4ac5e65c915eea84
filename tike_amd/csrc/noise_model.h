// The per-pixel formulas of the two noise models on a complete intensity, and
// the fixed-order float64 sum of a frame's cost: ONE home for
// tike_fly_farplane_gradient (fly.hip) and tike_cost_factor /
// tike_cost_curvature (autograd_cost.hip), whose costs carry the same bits.
//   gaussian: cost term (sqrt(I) - sqrt(d))^2, factor 1 - sqrt(d) / (sqrt(I) + 1e-9)
//             (reference operators/cupy/objective.py:11-15, :31-44)
//   poisson:  cost term I - d log(I + 1e-9),   factor 1 - d / (I + 1e-9)
//             (objective.py:72-74, :90-104)
#pragma once

#include "common.h"

// Cost term into `term`, the gradient factor l'(I, d) returned.  Neither is
// selected here: the count of an unmeasured pixel may be NaN, and the caller
// selects both away (never multiplies).
template <int MODEL>
__device__ __forceinline__ float tk_noise_pixel(float I, float d, float& term) {
  if (MODEL == 0) {
    const float sI = sqrtf(I), sd = sqrtf(d);
    const float diff = sI - sd;
    term = diff * diff;
    return 1.0f - sd / (sI + 1e-9f);
  }
  term = I - d * logf(I + 1e-9f);
  return 1.0f - d / (I + 1e-9f);
}

// The sum of a 256-lane workgroup's per-lane float64 partial sums in thread 0:
// wave shuffles, then the four waves through `red` (>= 4 doubles of LDS) as
// (w0 + w1) + (w2 + w3).  Contains a barrier; only thread 0's result counts.
__device__ __forceinline__ double tk_frame_sum_f64(double v, double* red) {
  v = tk_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
