// Device helpers and constants of the column pass that more than one unit of
// the fused operator uses: the detector counts and mask bits of a column-pass
// thread, the far-plane gradient factor, the XCD-aware tile order.
#pragma once
#include "common.h"

constexpr int TK_FG_PIX = 1024;  // pixels per workgroup of the stored-far-plane cost kernels
// fewest modes at which the gradient pass (and the Poisson sweeps) keep F of
// all modes in registers (fwd_grad_ifft2_pass1_resident_kernel; measured where
// ptycho.hip chooses between the two)
#define TK_FG_RESIDENT_MIN_MODES 6

#if defined(__HIPCC__)
// Counts and mask bits of the RB pixels (k1 + 16 k2, t) of position n of an
// N x N pattern, requested TOGETHER and unconditionally (a branch per pixel
// around its load makes RB serial memory round trips of them); unmeasured
// pixels may hold NaN: they are selected away by the mask bit, never multiplied.
template <int N, int RB, class DT>
__device__ __forceinline__ void tk_request_data(const DT* __restrict__ data,
                                                const unsigned char* __restrict__ mask, long n,
                                                int k1, int t, DT (&raw)[RB], unsigned& bits) {
  static_assert(RB <= 32, "one mask bit per pixel");
  const DT* __restrict__ d = data + n * (long)N * N + k1 * N;  // uniform
  const unsigned lo = (unsigned)t * (unsigned)sizeof(DT);
#pragma unroll
  for (int k2 = 0; k2 < RB; ++k2) raw[k2] = *tk_at_pinned(d + (16 * k2) * N, lo);
  bits = 0xffffffffu;
  if (mask) {  // uniform
    unsigned char mb[RB];
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) mb[k2] = mask[(k1 + 16 * k2) * N + t];
    bits = 0;
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) bits |= (mb[k2] ? 1u : 0u) << k2;
  }
}
template <class DT>
__device__ __forceinline__ void tk_request_data16(const DT* __restrict__ data,
                                                  const unsigned char* __restrict__ mask, long n,
                                                  int k1, int t, DT (&raw)[16], unsigned& bits) {
  tk_request_data<256, 16>(data, mask, n, k1, t, raw, bits);
}

// I[k2] (intensity) -> g * fwd_scale, returns this thread's cost terms.
template <int MODEL, int RB, class DT>
__device__ __forceinline__ float tk_gradient_factor(float (&I)[RB], const DT (&raw)[RB],
                                                    unsigned bits, float unmeasured_scaling,
                                                    float fwd_scale) {
  float cost = 0.f;
#pragma unroll
  for (int k2 = 0; k2 < RB; ++k2) {
    const bool meas = (bits >> k2) & 1u;
    const float dv = (float)raw[k2];
    float term, g;
    if (MODEL == 0) {
      const float sI = sqrtf(I[k2]), sd = sqrtf(dv);
      const float diff = sI - sd;
      term = diff * diff;
      g = -(1.0f - sd / (sI + 1e-9f));
    } else {
      term = I[k2] - dv * logf(I[k2] + 1e-9f);
      g = -(1.0f - dv / (I[k2] + 1e-9f));
    }
    cost += meas ? term : 0.f;
    I[k2] = (meas ? g : unmeasured_scaling - 1.0f) * fwd_scale;
  }
  return cost;
}
template <int MODEL, class DT>
__device__ __forceinline__ float tk_gradient_factor16(float (&I)[16], const DT (&raw)[16],
                                                      unsigned bits, float unmeasured_scaling,
                                                      float fwd_scale) {
  return tk_gradient_factor<MODEL, 16>(I, raw, bits, unmeasured_scaling, fwd_scale);
}

// XCD-aware tile order for kernels whose S mode tiles of one position share a
// per-position table (gscale): workgroups are dealt round-robin over the 8
// XCDs, so virtual block v runs on XCD v % 8; giving the S modes of a position
// to consecutive blocks OF ONE XCD lets that XCD's L2 fetch the table once
// instead of every XCD fetching it.  v ranges over ceil(nscan/8)*8*S; returns
// -1 for the padding.  Placement only affects speed, never results.
__device__ __forceinline__ long tk_xcd_tile(long v, int S, long nscan) {
  const long xcd = v & 7, slot = v >> 3;
  const long p = (slot / S) * 8 + xcd;
  return p < nscan ? p * S + slot % S : -1;
}

#endif
