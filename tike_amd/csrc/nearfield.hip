// Near-field (Fresnel, holographic) ptychography: the detector sits a finite
// distance behind the sample, so a frame is one Fresnel step of the exit wave,
//   w = IFFT2(H . FFT2(patch x probe)),   I = sum_j |w_j|^2,
// with probe window = detector.  multislice.hip already runs that step forward
// (tike_fwd_pass1 -> tike_fresnel_colpass -> inverse pass 2) and back
// (tike_fft2_pass1 -> tike_fresnel_colpass(adjoint) -> tike_ifft2_pass2_products);
// this file is the piece in the middle, in one launch:
//   inverse pass 2 -> intensity over the P = fly * S planes of a frame -> noise
//   model (noise_model.h) -> x gradient factor -> forward pass 1.
// A work item = (frame, q) as in slice_step_[n_]kernel: the inverse column
// stage leaves the rows {q + RB y2} of a plane in registers, which are the 16
// rows of group q of a forward pass 1 (TkSliceItem, multislice.hip), so the
// detector-plane wave of a near-field frame never exists in memory.
//
// Byte model per frame: P det^2 8 bytes of hand-off read once (twice when
// P > NF_KEEP), det^2 (4 or 2) of counts, det^2 of mask, and with `out`
// P det^2 8 written.  tike_fft2_pass2_inplace + tike_fly_farplane_gradient +
// tike_fft2_pass1 move 6 P det^2 8.
//
// Limits: det in {128, 256} (at 512 a radix-32 butterfly beside the kept
// planes spills, as in slice_step_back_kernel: that size takes the three
// launches), S <= 8, any fly.  The planes of a work item stay in registers
// between the two sweeps when P <= NF_KEEP = 3 (16 values = 32 registers per
// plane; 3 planes beside intensity, factor, counts and the row transform's 32
// fit the 256 registers of two waves per SIMD, a fourth spills); above, the
// second sweep reads `work` again, newest plane first, as
// tike_fwd_grad_ifft2_pass1 does.
#include "fft_engine2.h"
#include "internal.h"
#include "noise_model.h"
#include "tike_amd.h"

namespace {

constexpr int NF_KEEP = 3;       // planes a work item holds in registers
constexpr int NF_PARTIALS = 16;  // float64 cost partials per frame (>= items per frame)

// (TkSliceItem of multislice.hip for RB <= 16: one 16-row group per item)
template <int N>
struct NfItem {
  static constexpr int RB = N / 16;
  static constexpr int NI = RB;       // items per frame
  static constexpr int NF = 16 / RB;  // radix-RB stages per item
  static_assert(N == 128 || N == 256, "one 16-row group per work item");
  // the output k2 of stage f is the group's row q + RB y2
  static __device__ __forceinline__ constexpr int y2(int f, int k2) { return NF * k2 + f; }
};

// Inverse pass 2 of the rows {q + RB y2} of one plane, column t: v[y2].
template <int N>
__device__ __forceinline__ void nf_plane(const cf* __restrict__ plane, int q, int t,
                                         float inv_scale, cf (&v)[16]) {
  using It = NfItem<N>;
  constexpr int RB = It::RB;
#pragma unroll
  for (int f = 0; f < It::NF; ++f) {
    const int k1 = q + It::NI * f;
    const cf* __restrict__ p = plane + (long)k1 * N + t;
    cf u[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) u[r] = tk_ld_stream(p + (long)(16 * r) * N);
    Dft<RB, true>::run(u);
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) v[It::y2(f, k2)] = u[k2] * inv_scale;
  }
}

// GRAD: `out` is written.  KEEP > 0 (GRAD, P <= KEEP): one read of `work`.
template <int N, bool GRAD, int KEEP>
__global__ __launch_bounds__(N, 2) void nearfield_plane_gradient_kernel(
    const cf* __restrict__ work, const void* __restrict__ data_, int data_u16,
    const unsigned char* __restrict__ mask, const float* __restrict__ upstream,
    double* __restrict__ partials, float* __restrict__ intensity, cf* __restrict__ out,
    long nframe, int P, int model, float inv_scale, float scale, double inv_nmeasured,
    const cf* __restrict__ twtab) {
  using G2 = Fft2Geom<N>;
  using It = NfItem<N>;
  constexpr int RB = It::RB;
  constexpr int KK = KEEP > 0 ? KEEP : 1;
  constexpr int NW = N / 64;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  __shared__ double red[NW];
  cf* twl = lds + G2::LDS_ELEMS;
  if (GRAD) {
    FftTwLds<N>::fill(twl, twtab);
    __syncthreads();
  }
  const int t = threadIdx.x;
  const long npix = (long)N * N;
  for (long v = blockIdx.x; v < nframe * It::NI; v += gridDim.x) {
    const int q = (int)(v % It::NI);
    const long n = nframe - 1 - v / It::NI;  // descending: the column pass wrote ascending
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    const cf* __restrict__ F = work + n * P * npix;
    const long pix0 = (long)q * N + t;  // pixel of y2: pix0 + RB y2 N
    // the counts and the mask are requested with the planes, not behind them
    float d[16];
    bool measured[16];
    if (data_ != nullptr) {
      if (data_u16) {
        const unsigned short* __restrict__ dp = (const unsigned short*)data_ + n * npix + pix0;
#pragma unroll
        for (int y2 = 0; y2 < 16; ++y2) d[y2] = (float)dp[(long)(RB * y2) * N];
      } else {
        const float* __restrict__ dp = (const float*)data_ + n * npix + pix0;
#pragma unroll
        for (int y2 = 0; y2 < 16; ++y2) d[y2] = dp[(long)(RB * y2) * N];
      }
    } else {
#pragma unroll
      for (int y2 = 0; y2 < 16; ++y2) d[y2] = 0.f;
    }
#pragma unroll
    for (int y2 = 0; y2 < 16; ++y2)
      measured[y2] = mask != nullptr ? mask[pix0 + (long)(RB * y2) * N] != 0 : true;

    // sweep 1: the intensity of the frame
    float I[16];
#pragma unroll
    for (int y2 = 0; y2 < 16; ++y2) I[y2] = 0.f;
    cf w[KK][16];
    if (KEEP > 0) {
#pragma unroll
      for (int p = 0; p < KK; ++p) {
        if (p < P) {  // uniform
          nf_plane<N>(F + p * npix, q, t, inv_scale, w[p]);
#pragma unroll
          for (int y2 = 0; y2 < 16; ++y2) I[y2] += w[p][y2].x * w[p][y2].x + w[p][y2].y * w[p][y2].y;
        }
      }
    } else {
      for (int p = 0; p < P; ++p) {
        nf_plane<N>(F + p * npix, q, t, inv_scale, w[0]);
#pragma unroll
        for (int y2 = 0; y2 < 16; ++y2) I[y2] += w[0][y2].x * w[0][y2].x + w[0][y2].y * w[0][y2].y;
      }
    }
    if (intensity != nullptr) {
      float* __restrict__ ip = intensity + n * npix + pix0;
#pragma unroll
      for (int y2 = 0; y2 < 16; ++y2) tk_st_stream(ip + (long)(RB * y2) * N, I[y2]);
    }

    // the noise model: cost terms, and the factor g the planes are multiplied by
    float g[16];
    if (GRAD || partials != nullptr) {
      // upstream / num_measured, rounded once (tike_cost_factor's table)
      const float up =
          (float)((upstream != nullptr ? (double)upstream[n] : 1.0) * inv_nmeasured);
      double cost = 0.;
#pragma unroll
      for (int y2 = 0; y2 < 16; ++y2) {
        float term;
        const float lp = model == 0 ? tk_noise_pixel<0>(I[y2], d[y2], term)
                                    : tk_noise_pixel<1>(I[y2], d[y2], term);
        cost += measured[y2] ? (double)term : 0.0;
        g[y2] = measured[y2] ? scale * (up * lp) : 0.0f;
      }
      if (partials != nullptr) {  // uniform
        // lane, wave shuffles, the waves in ascending order; the finish
        // kernel adds the items of a frame in ascending order
        cost = tk_wave_sum(cost);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cost;
        __syncthreads();
        if (threadIdx.x == 0) {
          double s = red[0];
#pragma unroll
          for (int i = 1; i < NW; ++i) s += red[i];
          partials[n * NF_PARTIALS + q] = s;
        }
        __syncthreads();
      }
    }

    // sweep 2, newest plane first: g . w into forward pass 1
    if (GRAD) {
      if (KEEP > 0) {
#pragma unroll
        for (int p = KK - 1; p >= 0; --p) {
          if (p < P) {  // uniform
#pragma unroll
            for (int y2 = 0; y2 < 16; ++y2) w[p][y2] = w[p][y2] * g[y2];
            Dft<16, false>::run(w[p]);
#pragma unroll
            for (int ya = 1; ya < 16; ++ya) w[p][ya] = mul_tw<false>(w[p][ya], twtab[N + q * ya]);
            fft2_rows_from_columns<N, false, true>(lds, tw, line, j, w[p],
                                                   out + (n * P + p) * npix + (long)(16 * q) * N);
          }
        }
      } else {
        for (int p = P - 1; p >= 0; --p) {
          nf_plane<N>(F + p * npix, q, t, inv_scale, w[0]);
#pragma unroll
          for (int y2 = 0; y2 < 16; ++y2) w[0][y2] = w[0][y2] * g[y2];
          Dft<16, false>::run(w[0]);
#pragma unroll
          for (int ya = 1; ya < 16; ++ya) w[0][ya] = mul_tw<false>(w[0][ya], twtab[N + q * ya]);
          fft2_rows_from_columns<N, false, true>(lds, tw, line, j, w[0],
                                                 out + (n * P + p) * npix + (long)(16 * q) * N);
        }
      }
    }
  }
}

// costs[f] = (sum of the frame's partials, items ascending) / num_measured
__global__ __launch_bounds__(256) void nearfield_cost_finish_kernel(
    const double* __restrict__ partials, float* __restrict__ costs, long nframe, int nitem,
    double inv_nmeasured) {
  for (long n = blockIdx.x * (long)blockDim.x + threadIdx.x; n < nframe;
       n += (long)gridDim.x * blockDim.x) {
    double s = partials[n * NF_PARTIALS];
    for (int i = 1; i < nitem; ++i) s += partials[n * NF_PARTIALS + i];
    costs[n] = (float)(s * inv_nmeasured);
  }
}

template <int N>
void nf_launch(const cf* work, const void* data, int data_u16, const unsigned char* measured,
               const float* upstream, double* partials, float* intensity, cf* out, long nframe,
               int P, int model, float inv_scale, float scale, double inv, const cf* tw,
               hipStream_t stream) {
  const dim3 grid(tk_grid(nframe * NfItem<N>::NI, N == 128 ? 16 : 8)), block(N);
#define TK_NF(GRAD, KEEP)                                                                      \
  hipLaunchKernelGGL((nearfield_plane_gradient_kernel<N, GRAD, KEEP>), grid, block, 0, stream, \
                     work, data, data_u16, measured, upstream, partials, intensity, out,       \
                     nframe, P, model, inv_scale, scale, inv, tw)
  if (out == nullptr)
    TK_NF(false, 0);
  else if (P == 1)
    TK_NF(true, 1);
  else if (P == 2)
    TK_NF(true, 2);
  else if (P <= NF_KEEP)
    TK_NF(true, NF_KEEP);
  else
    TK_NF(true, 0);
#undef TK_NF
}

}  // namespace

extern "C" int tike_nearfield_cost_partials(long nframe) {
  return nframe < 0 || nframe > 0x7fffffffL / NF_PARTIALS ? -1 : (int)(nframe * NF_PARTIALS);
}

extern "C" int tike_nearfield_plane_gradient(const void* work, const void* data, int data_u16,
                                             const unsigned char* measured,
                                             const float* upstream, float* costs,
                                             double* cost_partials, float* intensity, void* out,
                                             long nframe, int fly, int S, int det, int model,
                                             long num_measured, float inv_scale, float scale,
                                             void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nframe >= 0 && fly >= 1 && S >= 1 && det >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  TK_CHECK_ARG(work != nullptr && out != work);
  TK_CHECK_ARG(data != nullptr || (costs == nullptr && out == nullptr));
  TK_CHECK_ARG(costs == nullptr || cost_partials != nullptr);
  TK_CHECK_ARG((long)fly * S <= 0x7fffffffL);
  TK_CHECK_ARG(nframe <= 0x7fffffffL / NF_PARTIALS);
  if ((det != 128 && det != 256) || S > 8) return TK_ERR_UNSUPPORTED;
  if (nframe == 0) return TK_OK;
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  const int P = fly * S;
  const double inv = 1.0 / (double)num_measured;
  double* partials = costs != nullptr ? cost_partials : nullptr;
  if (det == 128)
    nf_launch<128>((const cf*)work, data, data_u16, measured, upstream, partials, intensity,
                   (cf*)out, nframe, P, model, inv_scale, scale, inv, tw, stream);
  else
    nf_launch<256>((const cf*)work, data, data_u16, measured, upstream, partials, intensity,
                   (cf*)out, nframe, P, model, inv_scale, scale, inv, tw, stream);
  TK_LAUNCH_CHECK();
  if (costs != nullptr) {
    hipLaunchKernelGGL(nearfield_cost_finish_kernel, dim3(tk_grid((nframe + 255) / 256, 8)),
                       dim3(256), 0, stream, (const double*)partials, costs, nframe, det / 16,
                       inv);
    TK_LAUNCH_CHECK();
  }
  return TK_OK;
}
