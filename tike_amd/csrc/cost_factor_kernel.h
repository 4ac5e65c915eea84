// The kernel of tike_cost_factor (autograd_cost.hip) and
// tike_background_cost_factor (background.hip): ONE home.
#pragma once

#include "frame_lanes.h"
#include "noise_model.h"

namespace {

constexpr int CT_PX = 4;  // pixels of a lane per sweep: two 16-byte far-plane loads

// The layout of fly_farplane_gradient_kernel without its scaling: one
// workgroup per frame, a lane owns CT_PX consecutive pixels per sweep and walks
// the P planes (any P; nothing is kept), the last npix % CT_PX pixels one per
// lane.  The frame's cost is summed as that kernel sums it -- lane, wave
// shuffles, the four waves through LDS, float64 -- so costs carry its bits.
// The intensity is the float32 running sum of tike_intensity (planes
// ascending, each product and each sum rounded): contraction is off in the
// kernel body so that those bits do not hang on what the compiler fuses (see
// intensity_tangent_kernel); the noise-model formulas are compiled in
// noise_model.h exactly as fly.hip compiles them.  BG: `background` (npix) is
// added to the complete intensity (one float32 add) in front of the noise
// model, as fly_frame.h adds it; it is the LAST kernel argument, so that the
// instantiations without it keep the argument offsets, and with them the
// instructions, they had in autograd_cost.hip.
template <int MODEL, bool U16, bool BG>
__global__ __launch_bounds__(256) void cost_factor_kernel(
    const cf* __restrict__ farplane, const void* __restrict__ data_,
    const unsigned char* __restrict__ mask, const float* __restrict__ upstream,
    float* __restrict__ costs, float* __restrict__ table, int P, long npix,
    double inv_nmeasured, const float* __restrict__ background) {
#pragma clang fp contract(off)
  constexpr int PX = CT_PX;
  __shared__ double red[4];
  const long n = blockIdx.x;
  const cf* __restrict__ F = farplane + n * P * npix;
  const void* __restrict__ data =
      U16 ? (const void*)((const unsigned short*)data_ + n * npix)
          : (const void*)((const float*)data_ + n * npix);
  // upstream / num_measured, rounded once
  const float up = (float)((upstream != nullptr ? (double)upstream[n] : 1.0) * inv_nmeasured);
  float* __restrict__ T = table != nullptr ? table + n * npix : nullptr;
  double cost = 0.;
  const long nvec = npix / PX;
  for (long v = threadIdx.x; v < nvec; v += blockDim.x) {
    const long p = v * PX;
    // the counts and the mask are requested with the planes, not behind them
    float d[PX];
    tk_counts4<U16>(data, p, d);
    bool measured[PX] = {true, true, true, true};
    if (mask != nullptr) tk_mask4(mask, p, measured);
    tk_f4a4 bg;
    if (BG) bg = *reinterpret_cast<const tk_f4a4*>(background + p);
    float I[PX] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < P; ++j) {
      const cf* at = F + j * npix + p;
      const tk_f4a8 a = *reinterpret_cast<const tk_f4a8*>(at);
      const tk_f4a8 b = *reinterpret_cast<const tk_f4a8*>(at + 2);
      I[0] += a.x * a.x + a.y * a.y;
      I[1] += a.z * a.z + a.w * a.w;
      I[2] += b.x * b.x + b.y * b.y;
      I[3] += b.z * b.z + b.w * b.w;
    }
    tk_f4a4 o;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      float term;
      const float lp = tk_noise_pixel<MODEL>(BG ? I[k] + bg[k] : I[k], d[k], term);
      cost += measured[k] ? (double)term : 0.0;
      o[k] = measured[k] ? up * lp : 0.0f;
    }
    if (T != nullptr) *reinterpret_cast<tk_f4a4*>(T + p) = o;
  }
  // scalar tail: fewer than CT_PX pixels, one per lane
  for (long p = nvec * PX + threadIdx.x; p < npix; p += blockDim.x) {
    const float dv = U16 ? (float)((const unsigned short*)data)[p] : ((const float*)data)[p];
    const bool measured = mask != nullptr ? mask[p] != 0 : true;
    float I = 0.f;
    for (int j = 0; j < P; ++j) {
      const cf a = F[j * npix + p];
      I += a.x * a.x + a.y * a.y;
    }
    float term;
    const float lp = tk_noise_pixel<MODEL>(BG ? I + background[p] : I, dv, term);
    cost += measured ? (double)term : 0.0;
    if (T != nullptr) T[p] = measured ? up * lp : 0.0f;
  }
  if (costs != nullptr) {
    cost = tk_frame_sum_f64(cost, red);
    if (threadIdx.x == 0) costs[n] = (float)(cost * inv_nmeasured);
  }
}

}  // namespace
