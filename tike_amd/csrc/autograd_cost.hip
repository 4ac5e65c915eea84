// The noise-model cost of tike_amd.autograd.cost on a far plane, and what its
// backward and its Gauss-Newton product need of a frame's pixels, so that no
// per-pixel quantity of a frame leaves the chunk that formed it (no reference
// counterpart).  With I[f][p] = sum_{j<P} |far[f][j][p]|^2, P = fly * S, d the
// counts, l' the gradient factor of noise_model.h and M the measured pixels:
//
//   tike_cost_factor     costs[f]    = sum_{p in M} term(I, d) / num_measured
//                        table[f][p] = upstream[f] l'(I, d) / num_measured   p in M
//                                    = 0                                     else
//   tike_cost_curvature  dI[f][p]    = 2 sum_j Re( conj(far[f][j][p]) dfar[f][j][p] )
//                        costs[f]    as above
//                        dcosts[f]   = sum_{p in M} l'(I, d) dI / num_measured
//                        table[f][p] = upstream[f] c / (num_measured (I + floor)) dI
//                                      on M, 0 else; c = 1/2 gaussian, 1 poisson
//
// The tables are what tike_ifft2_crop_scaled, tike_ifft2_pass1_scaled and
// tike_farplane_scale take as the upstream gradient dL/dI.
//
// Byte model per frame of P planes of npix pixels: P * npix * 8 bytes of far
// plane read once (twice that with the tangent), npix * 4 (or * 2) bytes of
// counts, npix bytes of mask when there is one, npix * 4 bytes of table
// written; 4 or 8 bytes of costs.  Nothing is read twice.
#include "../../include/tike_amd.h"
#include "cost_factor_kernel.h"

#include <cmath>

namespace {

// cost_factor_kernel and CT_PX are in cost_factor_kernel.h (shared with
// background.hip).

// The same layout over a far plane and its tangent.  dI is the float32 running
// sum of tike_intensity_tangent, doubled; without counts (data NULL: neither
// costs nor dcosts) the noise model is not evaluated.  curv = c / num_measured.
template <int MODEL, bool U16>
__global__ __launch_bounds__(256) void cost_curvature_kernel(
    const cf* __restrict__ farplane, const cf* __restrict__ dfarplane,
    const void* __restrict__ data_, const unsigned char* __restrict__ mask,
    const float* __restrict__ upstream, float* __restrict__ costs, float* __restrict__ dcosts,
    float* __restrict__ table, int P, long npix, float floor_, double curv,
    double inv_nmeasured) {
#pragma clang fp contract(off)
  constexpr int PX = CT_PX;
  __shared__ double red[4];
  __shared__ double dred[4];
  const long n = blockIdx.x;
  const cf* __restrict__ F = farplane + n * P * npix;
  const cf* __restrict__ D = dfarplane + n * P * npix;
  const bool counts = data_ != nullptr;
  const void* __restrict__ data =
      !counts ? nullptr
              : (U16 ? (const void*)((const unsigned short*)data_ + n * npix)
                     : (const void*)((const float*)data_ + n * npix));
  // upstream c / num_measured, rounded once
  const float up = (float)((upstream != nullptr ? (double)upstream[n] : 1.0) * curv);
  float* __restrict__ T = table != nullptr ? table + n * npix : nullptr;
  double cost = 0., dcost = 0.;
  const long nvec = npix / PX;
  for (long v = threadIdx.x; v < nvec; v += blockDim.x) {
    const long p = v * PX;
    // the counts and the mask are requested with the planes, not behind them
    float d[PX] = {0.f, 0.f, 0.f, 0.f};
    if (counts) tk_counts4<U16>(data, p, d);
    bool measured[PX] = {true, true, true, true};
    if (mask != nullptr) tk_mask4(mask, p, measured);
    float I[PX] = {0.f, 0.f, 0.f, 0.f};
    float G[PX] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < P; ++j) {
      const cf* at = F + j * npix + p;
      const cf* dt = D + j * npix + p;
      const tk_f4a8 a = *reinterpret_cast<const tk_f4a8*>(at);
      const tk_f4a8 b = *reinterpret_cast<const tk_f4a8*>(at + 2);
      const tk_f4a8 da = *reinterpret_cast<const tk_f4a8*>(dt);
      const tk_f4a8 db = *reinterpret_cast<const tk_f4a8*>(dt + 2);
      I[0] += a.x * a.x + a.y * a.y;
      I[1] += a.z * a.z + a.w * a.w;
      I[2] += b.x * b.x + b.y * b.y;
      I[3] += b.z * b.z + b.w * b.w;
      G[0] += a.x * da.x + a.y * da.y;
      G[1] += a.z * da.z + a.w * da.w;
      G[2] += b.x * db.x + b.y * db.y;
      G[3] += b.z * db.z + b.w * db.w;
    }
    tk_f4a4 o;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const float dI = 2.0f * G[k];
      if (counts) {
        float term;
        const float lp = tk_noise_pixel<MODEL>(I[k], d[k], term);
        cost += measured[k] ? (double)term : 0.0;
        dcost += measured[k] ? (double)lp * (double)dI : 0.0;
      }
      o[k] = measured[k] ? (up / (I[k] + floor_)) * dI : 0.0f;
    }
    if (T != nullptr) *reinterpret_cast<tk_f4a4*>(T + p) = o;
  }
  // scalar tail: fewer than CT_PX pixels, one per lane
  for (long p = nvec * PX + threadIdx.x; p < npix; p += blockDim.x) {
    const bool measured = mask != nullptr ? mask[p] != 0 : true;
    float I = 0.f, G = 0.f;
    for (int j = 0; j < P; ++j) {
      const cf a = F[j * npix + p], da = D[j * npix + p];
      I += a.x * a.x + a.y * a.y;
      G += a.x * da.x + a.y * da.y;
    }
    const float dI = 2.0f * G;
    if (counts) {
      const float dv = U16 ? (float)((const unsigned short*)data)[p] : ((const float*)data)[p];
      float term;
      const float lp = tk_noise_pixel<MODEL>(I, dv, term);
      cost += measured ? (double)term : 0.0;
      dcost += measured ? (double)lp * (double)dI : 0.0;
    }
    if (T != nullptr) T[p] = measured ? (up / (I + floor_)) * dI : 0.0f;
  }
  if (costs != nullptr) {
    cost = tk_frame_sum_f64(cost, red);
    if (threadIdx.x == 0) costs[n] = (float)(cost * inv_nmeasured);
  }
  if (dcosts != nullptr) {
    dcost = tk_frame_sum_f64(dcost, dred);
    if (threadIdx.x == 0) dcosts[n] = (float)(dcost * inv_nmeasured);
  }
}

}  // namespace

extern "C" int tike_cost_factor(const void* farplane, const void* data, int data_u16,
                                const unsigned char* measured, const float* upstream,
                                float* costs, float* table, long nframe, int P, long npix,
                                int model, long num_measured, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && data);
  TK_CHECK_ARG(nframe >= 0 && P >= 1 && npix >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  if (nframe == 0) return TK_OK;
  TK_CHECK_ARG(nframe <= 0x7fffffffL);  // one workgroup per frame: grid.x
  const double inv = 1.0 / (double)num_measured;
  const dim3 grid((unsigned)nframe), block(256);
#define TK_COST(M, U)                                                                      \
  hipLaunchKernelGGL((cost_factor_kernel<M, U, false>), grid, block, 0, stream,           \
                     (const cf*)farplane, data, measured, upstream, costs, table, P, npix, \
                     inv, (const float*)nullptr)
  if (model == 0 && data_u16)
    TK_COST(0, true);
  else if (model == 0)
    TK_COST(0, false);
  else if (data_u16)
    TK_COST(1, true);
  else
    TK_COST(1, false);
#undef TK_COST
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_cost_curvature(const void* farplane, const void* dfarplane,
                                   const void* data, int data_u16,
                                   const unsigned char* measured, const float* upstream,
                                   float* costs, float* dcosts, float* table, long nframe,
                                   int P, long npix, int model, float floor,
                                   long num_measured, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && dfarplane);
  TK_CHECK_ARG(data || (!costs && !dcosts));
  TK_CHECK_ARG(nframe >= 0 && P >= 1 && npix >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  TK_CHECK_ARG(std::isfinite(floor) && floor >= 0.0f);
  if (nframe == 0) return TK_OK;
  TK_CHECK_ARG(nframe <= 0x7fffffffL);  // one workgroup per frame: grid.x
  const double inv = 1.0 / (double)num_measured;
  const double curv = (model == 0 ? 0.5 : 1.0) * inv;
  const dim3 grid((unsigned)nframe), block(256);
#define TK_CURV(M, U)                                                                   \
  hipLaunchKernelGGL((cost_curvature_kernel<M, U>), grid, block, 0, stream,             \
                     (const cf*)farplane, (const cf*)dfarplane, data, measured, upstream, \
                     costs, dcosts, table, P, npix, floor, curv, inv)
  if (model == 0 && data_u16)
    TK_CURV(0, true);
  else if (model == 0)
    TK_CURV(0, false);
  else if (data_u16)
    TK_CURV(1, true);
  else
    TK_CURV(1, false);
#undef TK_CURV
  TK_LAUNCH_CHECK();
  return TK_OK;
}
