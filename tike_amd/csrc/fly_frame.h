// The kernel of tike_fly_farplane_gradient (fly.hip) and
// tike_background_farplane_gradient (background.hip): ONE home, so that the
// two entries cannot drift apart.  BG adds the incoherent background b[p] to
// the complete intensity before the noise model is evaluated.  `background`
// is the LAST kernel argument: the instantiations without it keep the
// argument offsets, and with them the instructions, they had in fly.hip.
#pragma once

#include "frame_lanes.h"
#include "noise_model.h"

namespace {

constexpr int FLY_PX = 4;  // pixels of a lane per sweep: two 16-byte far-plane loads

// One pixel whose intensity is complete: its cost term into `cost` (measured
// pixels only) and the factor the far plane is multiplied by, -(gradient
// factor) on measured pixels and unmeasured_scaling - 1 elsewhere.  The count
// of an unmeasured pixel may be NaN: selected away, never multiplied.  The
// formulas live in noise_model.h.
template <int MODEL>
__device__ __forceinline__ float fly_pixel(float I, float d, bool measured, float ums1,
                                           double& cost) {
  float term;
  const float g = -tk_noise_pixel<MODEL>(I, d, term);
  cost += measured ? (double)term : 0.0;
  return measured ? g : ums1;
}

// One workgroup per frame; a lane owns FLY_PX consecutive pixels per sweep.
// R > 0 (with GRAD, P <= R): the P planes of those pixels stay in registers
// between the intensity sum and the scaling -- the far plane is read from
// memory once.  R == 0: the planes are read a second time for the scaling; the
// second read follows the first within one sweep of the workgroup
// (256 lanes * 4 pixels * 8 bytes * P).  The last npix % FLY_PX pixels are
// taken one per lane.  The frame's cost is summed in float64 in a fixed order:
// lane, wave shuffles, the four waves through LDS.  BG: `background` (npix)
// is added to the complete intensity (one float32 add) in front of the noise
// model; `intensity` receives the sum without it.  A background value under
// the mask may be NaN, like a count there.
template <int MODEL, bool GRAD, bool U16, int R, bool BG>
__global__ __launch_bounds__(256) void fly_farplane_gradient_kernel(
    cf* __restrict__ farplane, const void* __restrict__ data_,
    const unsigned char* __restrict__ mask, float* __restrict__ intensity,
    float* __restrict__ costs, int P, long npix, float ums1, double inv_nmeasured,
    const float* __restrict__ background) {
  constexpr int PX = FLY_PX;
  constexpr int RR = R > 0 ? R : 1;
  __shared__ double red[4];
  const long n = blockIdx.x;
  cf* __restrict__ F = farplane + n * P * npix;
  const float* __restrict__ d32 = U16 ? nullptr : (const float*)data_ + n * npix;
  const unsigned short* __restrict__ d16 =
      U16 ? (const unsigned short*)data_ + n * npix : nullptr;
  double cost = 0.;
  const long nvec = npix / PX;
  for (long v = threadIdx.x; v < nvec; v += blockDim.x) {
    const long p = v * PX;
    // the counts and the mask are requested with the planes, not behind them
    float d[PX];
    tk_counts4<U16>(U16 ? (const void*)d16 : (const void*)d32, p, d);
    bool measured[PX] = {true, true, true, true};
    if (mask != nullptr) tk_mask4(mask, p, measured);
    tk_f4a4 bg;
    if (BG) bg = *reinterpret_cast<const tk_f4a4*>(background + p);
    float I[PX] = {0.f, 0.f, 0.f, 0.f};
    tk_f4a8 r[RR][2];
    if (GRAD && R > 0) {
#pragma unroll
      for (int j = 0; j < RR; ++j) {
        if (j < P) {
          const cf* at = F + j * npix + p;
          r[j][0] = *reinterpret_cast<const tk_f4a8*>(at);
          r[j][1] = *reinterpret_cast<const tk_f4a8*>(at + 2);
        }
      }
#pragma unroll
      for (int j = 0; j < RR; ++j) {
        if (j < P) {
          I[0] += r[j][0].x * r[j][0].x + r[j][0].y * r[j][0].y;
          I[1] += r[j][0].z * r[j][0].z + r[j][0].w * r[j][0].w;
          I[2] += r[j][1].x * r[j][1].x + r[j][1].y * r[j][1].y;
          I[3] += r[j][1].z * r[j][1].z + r[j][1].w * r[j][1].w;
        }
      }
    } else {
      for (int j = 0; j < P; ++j) {
        const cf* at = F + j * npix + p;
        const tk_f4a8 a = *reinterpret_cast<const tk_f4a8*>(at);
        const tk_f4a8 b = *reinterpret_cast<const tk_f4a8*>(at + 2);
        I[0] += a.x * a.x + a.y * a.y;
        I[1] += a.z * a.z + a.w * a.w;
        I[2] += b.x * b.x + b.y * b.y;
        I[3] += b.z * b.z + b.w * b.w;
      }
    }
    float g[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k)
      g[k] = fly_pixel<MODEL>(BG ? I[k] + bg[k] : I[k], d[k], measured[k], ums1, cost);
    if (intensity != nullptr) {
      tk_f4a4 o;
#pragma unroll
      for (int k = 0; k < PX; ++k) o[k] = I[k];
      *reinterpret_cast<tk_f4a4*>(intensity + n * npix + p) = o;
    }
    if (GRAD && R > 0) {
#pragma unroll
      for (int j = 0; j < RR; ++j) {
        if (j < P) {
          cf* at = F + j * npix + p;
          tk_f4a8 a = r[j][0], b = r[j][1];
          a.x *= g[0], a.y *= g[0], a.z *= g[1], a.w *= g[1];
          b.x *= g[2], b.y *= g[2], b.z *= g[3], b.w *= g[3];
          *reinterpret_cast<tk_f4a8*>(at) = a;
          *reinterpret_cast<tk_f4a8*>(at + 2) = b;
        }
      }
    } else if (GRAD) {
      for (int j = 0; j < P; ++j) {
        cf* at = F + j * npix + p;
        tk_f4a8 a = *reinterpret_cast<const tk_f4a8*>(at);
        tk_f4a8 b = *reinterpret_cast<const tk_f4a8*>(at + 2);
        a.x *= g[0], a.y *= g[0], a.z *= g[1], a.w *= g[1];
        b.x *= g[2], b.y *= g[2], b.z *= g[3], b.w *= g[3];
        *reinterpret_cast<tk_f4a8*>(at) = a;
        *reinterpret_cast<tk_f4a8*>(at + 2) = b;
      }
    }
  }
  // scalar tail: fewer than FLY_PX pixels, one per lane
  for (long p = nvec * PX + threadIdx.x; p < npix; p += blockDim.x) {
    const float dv = U16 ? (float)d16[p] : d32[p];
    const bool measured = mask != nullptr ? mask[p] != 0 : true;
    float I = 0.f;
    for (int j = 0; j < P; ++j) I += norm2(F[j * npix + p]);
    const float g = fly_pixel<MODEL>(BG ? I + background[p] : I, dv, measured, ums1, cost);
    if (intensity != nullptr) intensity[n * npix + p] = I;
    if (GRAD)
      for (int j = 0; j < P; ++j) F[j * npix + p] = F[j * npix + p] * g;
  }
  if (costs != nullptr) {
    cost = tk_wave_sum(cost);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cost;
    __syncthreads();
    if (threadIdx.x == 0)
      costs[n] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_nmeasured);
  }
}

}  // namespace
