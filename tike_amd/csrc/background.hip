// A fitted incoherent background per detector pixel (no reference
// counterpart): air scatter, fluorescence and dark current add a non-negative
// count b[p] to every frame that does not move with the scan,
//   I_model[f][p] = sum_{j < fly*S} |farplane[f][j][p]|^2 + b[p].
// The noise-model formulas of noise_model.h are taken at Ib = I + b[p]: I the
// float32 running sum over the planes (the bits of tike_intensity), then ONE
// float32 add.
//   tike_background_farplane_gradient  tike_fly_farplane_gradient at Ib
//                                      (the kernel of fly_frame.h)
//   tike_background_cost_factor        tike_cost_factor at Ib
//                                      (the kernel of cost_factor_kernel.h)
//   tike_background_sums               gradient and cost with respect to b on
//                                      STORED intensities: d term / d b =
//                                      l'(Ib, d), and I does not depend on b,
//                                      so a whole CG block on b needs no
//                                      transform
//
// Byte model of tike_background_sums: nframe * npix * (4 + 4 or 2) bytes of
// intensity and counts read once; the mask and b once per workgroup; npix * 4
// bytes of bgrad and 8 bytes of partial per workgroup written.
#include "../../include/tike_amd.h"
#include "cost_factor_kernel.h"
#include "fly_frame.h"

namespace {

constexpr int BS_LANES = 64;  // one wave per workgroup: npix / 4 lanes is all the
                              // parallelism there is, so spread it over the CUs
constexpr int BS_PX = 4;      // pixels of a lane: 16-byte intensity and count loads

// A lane's W consecutive pixels (4, or 1 for the last npix % 4) through every
// frame, ascending.  Per pixel the float32 products up_f l'(Ib, d) -- up_f =
// upstream[f] / num_measured rounded once, the table of tike_cost_factor -- are
// summed in float64 and rounded once into bgrad; an unmeasured pixel gives
// exactly 0, and its count and background (possibly NaN) are selected away,
// never multiplied.  The lane's part of sum_f upstream[f] sum_p term goes to
// `cost` in float64.
template <int MODEL, bool U16, int W>
__device__ __forceinline__ void sums_walk(const float* __restrict__ intensity,
                                          const void* __restrict__ data,
                                          const unsigned char* __restrict__ mask,
                                          const float* __restrict__ background,
                                          const float* __restrict__ upstream,
                                          float* __restrict__ bgrad, long nframe, long npix,
                                          long p, double inv_nmeasured, double& cost) {
#pragma clang fp contract(off)
  bool measured[W];
  float bg[W];
  double acc[W];
  if (W == 4) {
    const tk_f4a4 b4 = *reinterpret_cast<const tk_f4a4*>(background + p);
#pragma unroll
    for (int k = 0; k < W; ++k) bg[k] = b4[k], measured[k] = true, acc[k] = 0.;
    if (mask != nullptr) {
      const tk_m4a1 m4 = *reinterpret_cast<const tk_m4a1*>(mask + p);
#pragma unroll
      for (int k = 0; k < W; ++k) measured[k] = m4[k] != 0;
    }
  } else {
    bg[0] = background[p], acc[0] = 0.;
    measured[0] = mask != nullptr ? mask[p] != 0 : true;
  }
#pragma unroll 4
  for (long f = 0; f < nframe; ++f) {
    float I[W], d[W];
    if (W == 4) {
      const tk_f4a4 i4 = *reinterpret_cast<const tk_f4a4*>(intensity + f * npix + p);
      float d4[4];
      tk_counts4<U16>(U16 ? (const void*)((const unsigned short*)data + f * npix)
                          : (const void*)((const float*)data + f * npix),
                      p, d4);
#pragma unroll
      for (int k = 0; k < W; ++k) I[k] = i4[k], d[k] = d4[k];
    } else {
      I[0] = intensity[f * npix + p];
      d[0] = U16 ? (float)((const unsigned short*)data)[f * npix + p]
                 : ((const float*)data)[f * npix + p];
    }
    const double u = upstream != nullptr ? (double)upstream[f] : 1.0;
    const float up = (float)(u * inv_nmeasured);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float term;
      const float lp = tk_noise_pixel<MODEL>(I[k] + bg[k], d[k], term);
      acc[k] += measured[k] ? (double)(up * lp) : 0.0;
      cost += measured[k] ? u * (double)term : 0.0;
    }
  }
  if (bgrad != nullptr) {
    if (W == 4) {
      tk_f4a4 o;
#pragma unroll
      for (int k = 0; k < W; ++k) o[k] = (float)acc[k];
      *reinterpret_cast<tk_f4a4*>(bgrad + p) = o;
    } else {
      bgrad[p] = (float)acc[0];
    }
  }
}

// Item v < npix / 4 is the four pixels at 4 v; the items behind them are the
// last npix % 4 pixels, one per lane.  A lane owns its pixels through every
// frame, so no sum crosses lanes but the cost: one float64 partial per
// workgroup (a wave), the caller adds them in order.
template <int MODEL, bool U16>
__global__ __launch_bounds__(BS_LANES) void background_sums_kernel(
    const float* __restrict__ intensity, const void* __restrict__ data,
    const unsigned char* __restrict__ mask, const float* __restrict__ background,
    const float* __restrict__ upstream, double* __restrict__ partials,
    float* __restrict__ bgrad, long nframe, long npix, double inv_nmeasured) {
  const long nvec = npix / BS_PX;
  const long item = (long)blockIdx.x * BS_LANES + threadIdx.x;
  double cost = 0.;
  if (item < nvec)
    sums_walk<MODEL, U16, BS_PX>(intensity, data, mask, background, upstream, bgrad, nframe,
                                 npix, item * BS_PX, inv_nmeasured, cost);
  else if (item < nvec + npix % BS_PX)
    sums_walk<MODEL, U16, 1>(intensity, data, mask, background, upstream, bgrad, nframe, npix,
                             nvec * BS_PX + (item - nvec), inv_nmeasured, cost);
  if (partials != nullptr) {
    cost = tk_wave_sum(cost);
    if (threadIdx.x == 0) partials[blockIdx.x] = cost * inv_nmeasured;
  }
}

long sums_workgroups(long npix) {
  const long items = npix / BS_PX + npix % BS_PX;
  return (items + BS_LANES - 1) / BS_LANES;
}

template <int MODEL, bool U16>
void bg_fly_launch(cf* far, const void* data, const unsigned char* measured,
                   const float* background, float* intensity, float* costs, int nframe, int P,
                   long npix, int apply_gradient, float ums1, double inv, hipStream_t stream) {
  const dim3 grid((unsigned)nframe), block(256);
#define TK_BG_FLY(G, R)                                                                     \
  hipLaunchKernelGGL((fly_farplane_gradient_kernel<MODEL, G, U16, R, true>), grid, block, 0, \
                     stream, far, data, measured, intensity, costs, P, npix, ums1, inv,      \
                     background)
  // the register classes of tike_fly_farplane_gradient
  if (!apply_gradient)
    TK_BG_FLY(false, 0);
  else if (P <= 4)
    TK_BG_FLY(true, 4);
  else if (P <= 8)
    TK_BG_FLY(true, 8);
  else if (P <= 16)
    TK_BG_FLY(true, 16);
  else
    TK_BG_FLY(true, 0);
#undef TK_BG_FLY
}

}  // namespace

extern "C" int tike_background_farplane_gradient(
    void* farplane, const void* data, int data_u16, const unsigned char* measured,
    const float* background, float* intensity, float* costs, int nframe, int fly, int S,
    int det, int model, int apply_gradient, float unmeasured_scaling, long num_measured,
    void* stream_) {
  if (background == nullptr)
    return tike_fly_farplane_gradient(farplane, data, data_u16, measured, intensity, costs,
                                      nframe, fly, S, det, model, apply_gradient,
                                      unmeasured_scaling, num_measured, stream_);
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && data);
  TK_CHECK_ARG(nframe >= 0 && fly >= 1 && S >= 1 && det >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured > 0);
  TK_CHECK_ARG((long)fly * S <= 0x7fffffffL);
  if (nframe == 0) return TK_OK;
  const int P = fly * S;
  const long npix = (long)det * det;
  const double inv = 1.0 / (double)num_measured;
  const float ums1 = unmeasured_scaling - 1.0f;
  cf* far = (cf*)farplane;
  if (model == 0 && data_u16)
    bg_fly_launch<0, true>(far, data, measured, background, intensity, costs, nframe, P, npix,
                           apply_gradient, ums1, inv, stream);
  else if (model == 0)
    bg_fly_launch<0, false>(far, data, measured, background, intensity, costs, nframe, P, npix,
                            apply_gradient, ums1, inv, stream);
  else if (data_u16)
    bg_fly_launch<1, true>(far, data, measured, background, intensity, costs, nframe, P, npix,
                           apply_gradient, ums1, inv, stream);
  else
    bg_fly_launch<1, false>(far, data, measured, background, intensity, costs, nframe, P, npix,
                            apply_gradient, ums1, inv, stream);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_background_cost_factor(const void* farplane, const void* data,
                                           int data_u16, const unsigned char* measured,
                                           const float* background, const float* upstream,
                                           float* costs, float* table, long nframe, int P,
                                           long npix, int model, long num_measured,
                                           void* stream_) {
  if (background == nullptr)
    return tike_cost_factor(farplane, data, data_u16, measured, upstream, costs, table, nframe,
                            P, npix, model, num_measured, stream_);
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
#define TK_BG_COST(M, U)                                                                  \
  hipLaunchKernelGGL((cost_factor_kernel<M, U, true>), grid, block, 0, stream,            \
                     (const cf*)farplane, data, measured, upstream, costs, table, P, npix, \
                     inv, background)
  if (model == 0 && data_u16)
    TK_BG_COST(0, true);
  else if (model == 0)
    TK_BG_COST(0, false);
  else if (data_u16)
    TK_BG_COST(1, true);
  else
    TK_BG_COST(1, false);
#undef TK_BG_COST
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_background_sums_partials(long npix) {
  if (npix < 1) return 0;
  const long n = sums_workgroups(npix);
  return n <= 0x7fffffffL ? (int)n : 0;
}

extern "C" int tike_background_sums(const float* intensity, const void* data, int data_u16,
                                    const unsigned char* measured, const float* background,
                                    const float* upstream, double* partials, float* bgrad,
                                    long nframe, long npix, int model, long num_measured,
                                    void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(intensity && data && background);
  TK_CHECK_ARG(nframe >= 0 && npix >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  if (nframe == 0) return TK_OK;
  const long groups = sums_workgroups(npix);
  TK_CHECK_ARG(groups <= 0x7fffffffL);
  const double inv = 1.0 / (double)num_measured;
  const dim3 grid((unsigned)groups), block(BS_LANES);
#define TK_BG_SUMS(M, U)                                                              \
  hipLaunchKernelGGL((background_sums_kernel<M, U>), grid, block, 0, stream, intensity, \
                     data, measured, background, upstream, partials, bgrad, nframe, npix, inv)
  if (model == 0 && data_u16)
    TK_BG_SUMS(0, true);
  else if (model == 0)
    TK_BG_SUMS(0, false);
  else if (data_u16)
    TK_BG_SUMS(1, true);
  else
    TK_BG_SUMS(1, false);
#undef TK_BG_SUMS
  TK_LAUNCH_CHECK();
  return TK_OK;
}
