// The gradient pass of the fused operator for gfx950 (the forward operator is
// forward.hip, the cgrad search cgrad_search.hip, the Poisson step lengths
// poisson.hip; this unit keeps the name of the file they were cut from, so
// that its history follows): intensity, per-pattern cost and far-plane
// gradient (ptycho.py:18-23, objective.py:11-124, lstsq.py:444-502), then
// IFFT2 -> crop to the probe window (propagation.py:59-73 + lstsq.py:504-507).
//   tike_fwd_gradient_scale, tike_grad_ifft2_crop, tike_grad_ifft2_pass1,
//   tike_fwd_grad_ifft2_pass1{,_slices}
//                        from the hand-off of tike_fwd_pass1: the far-plane
//                        waves never go through memory;
//   tike_farplane_gradient, tike_gradient_scale, tike_ifft2_crop{,_scaled,
//   _scaled_modes}, tike_ifft2_pass1_scaled
//                        the same from a stored far plane;
//   tike_intensity, tike_cost_each_pattern, tike_objective_grad
//                        the stand-alone objective ops (objective.py:18-124).
// tk_fwd_gradient_scale and tk_farplane_gradient are shared with
// cgrad_search.hip (internal.h).
#include "fft_engine2.h"
#include "internal.h"
#include "tike_amd.h"
#include "ptycho_shared.h"
#include "fwd_grad_resident.h"

// The cost slots of a speculative launch (a line-search trial enqueued ahead of
// the decisions), zeroed for the atomics -- unless the launch is skipped: a
// trial behind the accepted one leaves the costs of the last trial made.
__global__ __launch_bounds__(256) void zero_costs_unless_skipped_kernel(
    float* __restrict__ costs, long n, const int* __restrict__ skip) {
  if (*skip != 0) return;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) costs[i] = 0.f;
}

static void tk_zero_costs_unless_skipped(float* costs, long n, const int* skip,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(zero_costs_unless_skipped_kernel, dim3(tk_grid((n + 255) / 256, 1)),
                     dim3(256), 0, stream, costs, n, skip);
}

// The column pass as a pure read stream: one workgroup per (position, k1)
// forms F[k1 + 16 k2] of every mode in registers (radix-16 over the rows
// 16 r + k1 of the hand-off), accumulates I = sum_s |F_s|^2 and emits the
// gradient factor and the cost share of those 16 rows (objective.py:11-124,
// lstsq.py:444-502).  costs must be zero on entry (accumulated by atomics).
// DT: float, or unsigned short for detector counts kept as they arrived
// (16-bit data stays 16-bit in HBM, reference ptycho.py:383-390).
template <int N, int MODEL, class DT>
__global__ __launch_bounds__(256, N == 256 ? 4 : 2) void fwd_gradient_scale_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, float* __restrict__ gscale,
    float* __restrict__ intensity, const TkCostSink costs, cf* __restrict__ farplane,
    long nitem, int S, float scale, float unmeasured_scaling, float inv_nmeasured,
    const int* __restrict__ skip) {
  constexpr int RB = N / 16;    // radix of the column pass
  constexpr int NH = N / 256;   // 256-column blocks per row
  __shared__ float red[4];
  if (skip != nullptr && *skip != 0) return;  // speculative launch, not needed
  const float s2 = scale * scale;
  for (long v = blockIdx.x; v < nitem; v += gridDim.x) {
    // item = (position, k1, column block)
    const int hb = (int)(v % NH);
    const int k1 = (int)((v / NH) & 15);
    // positions in DESCENDING order: the last hand-off tiles forward pass 1
    // wrote (ascending) are still in the 256 MB Infinity Cache when this
    // kernel starts, and the ones read last here are the first the next
    // kernel (ascending again) asks for
    const long n = nitem / (16 * NH) - 1 - v / (16 * NH);
    const int t = hb * 256 + threadIdx.x;
    float I[RB];
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) I[k2] = 0.f;
    // 256^2: software pipelined over the modes -- the rows of mode s + 1 are
    // requested before the butterflies of mode s (124 VGPRs, still 4 waves per
    // SIMD; 1.00 -> 0.89 ms per 1000 positions).  At 512^2 (radix 32) the second
    // set of rows costs a wave per SIMD and loses (0.85 -> 0.92 ms).
    constexpr bool PIPE = N == 256;
    cf un[PIPE ? RB : 1];
    if (PIPE) {
      const cf* __restrict__ src0 = colin + (n * S) * (long)N * N + k1 * N + t;
#pragma unroll
      for (int r = 0; r < RB; ++r) un[PIPE ? r : 0] = tk_ld_stream(src0 + (long)(16 * r) * N);
    }
    for (int s = 0; s < S; ++s) {
      cf u[RB];
      if (PIPE) {
#pragma unroll
        for (int r = 0; r < RB; ++r) u[r] = un[PIPE ? r : 0];
        if (s + 1 < S) {
          const cf* __restrict__ src = colin + (n * S + s + 1) * (long)N * N + k1 * N + t;
#pragma unroll
          for (int r = 0; r < RB; ++r)
            un[PIPE ? r : 0] = tk_ld_stream(src + (long)(16 * r) * N);
        }
      } else {
        const cf* __restrict__ src = colin + (n * S + s) * (long)N * N + k1 * N + t;
#pragma unroll
        for (int r = 0; r < RB; ++r) u[r] = tk_ld_stream(src + (long)(16 * r) * N);
      }
      Dft<RB, false>::run(u);
#pragma unroll
      for (int k2 = 0; k2 < RB; ++k2) I[k2] += norm2(u[k2]) * s2;
      if (farplane != nullptr) {
        // the far-plane wave itself, for the pipelines that keep it
        cf* __restrict__ dst = farplane + (n * S + s) * (long)N * N + k1 * N + t;
#pragma unroll
        for (int k2 = 0; k2 < RB; ++k2) tk_st_stream(dst + (long)(16 * k2) * N, u[k2] * scale);
      }
    }
    // counts and mask requested together, the factor selected (not branched)
    DT raw[RB];
    unsigned bits;
    tk_request_data<N, RB>(data, mask, n, k1, t, raw, bits);
    if (intensity) {  // uniform
#pragma unroll
      for (int k2 = 0; k2 < RB; ++k2)
        tk_st_stream(intensity + n * (long)N * N + (long)(k1 + 16 * k2) * N + t, I[k2]);
    }
    float cost = tk_gradient_factor<MODEL, RB>(I, raw, bits, unmeasured_scaling, 1.0f);
    if (gscale) {  // uniform
#pragma unroll
      for (int k2 = 0; k2 < RB; ++k2)
        gscale[n * (long)N * N + (long)(k1 + 16 * k2) * N + t] = I[k2];
    }
    if (costs.costs) {
      cost = tk_block_sum256(cost, red);
      if (threadIdx.x == 0) tk_cost_add(costs, n, k1 * NH + hb, cost * inv_nmeasured);
    }
  }
}

// scratch: from tike_fwd_pass1 (UNSCALED column-pass input; `scale` is the
// forward FFT normalisation applied here).  intensity / costs may be NULL, and
// so may gscale when only the costs are wanted (a line-search probe).
int tk_fwd_gradient_scale(const void* scratch, const void* data, int data_u16,
                                 const unsigned char* measured, float* gscale, float* intensity,
                                 float* costs, void* farplane, int nscan, int S, int det,
                                 float scale, int model, float unmeasured_scaling,
                                 long num_measured, hipStream_t stream, const int* skip) {
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && det >= 1 && (model == 0 || model == 1) &&
               num_measured > 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(scratch && data && (gscale || costs) && farplane != scratch);
  if (det != 256 && det != 512) return TK_ERR_UNSUPPORTED;
  // (a speculative launch may return at once: its cost slots would be stale,
  // so the line searches keep the zeroed atomics)
  TkCostSink sink{costs, nullptr, 0};
  if (skip == nullptr) {
    int rc = tk_cost_sink(costs, nscan, 16 * (det / 256), stream, &sink);
    if (rc) return rc;
  } else if (costs) {
    tk_zero_costs_unless_skipped(costs, nscan, skip, stream);
  }
  const long nitem = (long)nscan * 16 * (det / 256);
  const float inv = 1.0f / (float)num_measured;
  const dim3 grid(tk_grid(nitem, 32)), block(256);
#define TK_FGS(N, M, DT)                                                                     \
  hipLaunchKernelGGL((fwd_gradient_scale_kernel<N, M, DT>), grid, block, 0, stream,             \
                     (const cf*)scratch, (const DT*)data, measured, gscale, intensity, sink,    \
                     (cf*)farplane, nitem, S, scale, unmeasured_scaling, inv, skip)
#define TK_FGS_N(N)                     \
  do {                                  \
    if (model == 0 && data_u16)         \
      TK_FGS(N, 0, unsigned short);     \
    else if (model == 0)                \
      TK_FGS(N, 0, float);              \
    else if (data_u16)                  \
      TK_FGS(N, 1, unsigned short);     \
    else                                \
      TK_FGS(N, 1, float);              \
  } while (0)
  if (det == 256)
    TK_FGS_N(256);
  else
    TK_FGS_N(512);
#undef TK_FGS_N
#undef TK_FGS
  TK_LAUNCH_CHECK();
  return tk_cost_finish(sink, nscan, stream);
}

extern "C" int tike_fwd_gradient_scale(const void* scratch, const void* data, int data_u16,
                                       const unsigned char* measured, float* gscale,
                                       float* intensity, float* costs, void* farplane, int nscan,
                                       int S, int det, float scale, int model,
                                       float unmeasured_scaling, long num_measured,
                                       void* stream_) {
  TK_ENTER();
  return tk_fwd_gradient_scale(scratch, data, data_u16, measured, gscale, intensity, costs,
                               farplane, nscan, S, det, scale, model, unmeasured_scaling,
                               num_measured, (hipStream_t)stream_, nullptr);
}

// ------------------------------------------------------- inverse + crop
template <int N>
__global__ __launch_bounds__(FftPlan<N>::NT, FftPlan<N>::MINW) void ifft2_crop_kernel(
    const cf* farplane, cf* work, cf* chi, long ntile,
    int pw, float scale, const cf* __restrict__ twtab) {
  using G = FftGeom<N>;
  __shared__ cf lds[G::LDS_ELEMS];
  FftTw<N> tw;
  const int pad = (N - pw) / 2;
  const int end = pad + pw;
  for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const cf* src = farplane + tile * (long)N * N;
    cf* mid = work + tile * (long)N * N;
    cf* dst = chi + tile * (long)pw * pw;
    const FftLane<N, false> row = fft_lane<N, false>();
    tw.init(twtab, row.j);
    for (int g = 0; g < N; g += G::L) {
      fft_lines<N, true, false>(
          lds, row, tw, [&](int line, int e) { return src[(g + line) * N + e]; },
          [&](int line, int e, cf v) { mid[(g + line) * N + e] = v; });
    }
    __syncthreads();
    const FftLane<N, true> col = fft_lane<N, true>();
    tw.init(twtab, col.j);
    for (int g = 0; g < N; g += G::L) {
      if (g + G::L <= pad || g >= end) continue;  // columns outside the crop
      fft_lines<N, true, true>(
          lds, col, tw, [&](int line, int e) { return mid[e * N + g + line]; },
          [&](int line, int e, cf v) {
            const int py = e - pad, px = g + line - pad;
            if (py >= 0 && py < pw && px >= 0 && px < pw) tk_st_stream(dst + py * pw + px, v * scale);
          });
    }
    __syncthreads();
  }
}

// v2: pass 1 farplane -> work (must not alias), pass 2 in place / cropped.
#ifndef TK_ICROP_WAVES
#define TK_ICROP_WAVES 4
#endif
// PASS2 = false: stop after pass 1 (`work` then holds the input of the column
// pass, which tike_ifft2_pass2_gradients consumes).
template <int N, int MODE, bool PASS2 = true>
__global__ __launch_bounds__(N, (N <= 256 ? TK_ICROP_WAVES : 2)) void ifft2_crop_v2_kernel(
    const cf* __restrict__ farplane, cf* work, cf* chi, long ntile, int pw, float scale,
    const cf* __restrict__ twtab, const float* __restrict__ gscale, int S,
    const float* __restrict__ mode_scale, const unsigned char* __restrict__ measured) {
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int pad = (N - pw) / 2;
  for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const cf* __restrict__ src = farplane + tile * (long)N * N;
    cf* mid = work + tile * (long)N * N;
    cf* dst = chi + tile * (long)pw * pw;
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    // far-plane gradient applied on the fly: F_s * g, g per (position, pixel);
    // MODE 2 (poisson): times the step of this (position, mode) on measured pixels
    const float* __restrict__ gs = MODE ? gscale + (tile / S) * (long)N * N : nullptr;
    const float ms = MODE >= 2 ? mode_scale[tile] : 1.0f;
    for (int r = 0; r < G2::RB; ++r)
      fft2_pass1<N, true, !PASS2>(
          lds, twtab, tw, line, j, r,
          [&](int y, int e, auto) {
            const cf f = tk_ld_stream(src + y * N + e);
            if (MODE == 0) return f;
            float g = gs[y * N + e];
            // (MODE 3 = MODE 2 with a mask: its byte is requested with the
            // factor and the step selected -- never a test around the load)
            if (MODE == 2) g *= ms;
            if (MODE == 3) g *= measured[y * N + e] ? ms : 1.0f;
            return f * g;
          },
          mid);
    if constexpr (PASS2) {
      __syncthreads();
      for (int k1 = 0; k1 < 16; ++k1)
        fft2_pass2<N, true>(mid, k1, [&](int ky, int t, cf v) {
          const int py = ky - pad, px = t - pad;
          if (py >= 0 && py < pw && px >= 0 && px < pw)
            tk_st_stream(dst + py * pw + px, v * scale);
        });
      __syncthreads();
    }
  }
}

template <int N, bool PASS2 = true>
static int launch_icrop_v2(const cf* far, cf* work, cf* chi, long ntile, int pw, float scale,
                           hipStream_t stream, const float* gscale = nullptr, int S = 1,
                           const float* mode_scale = nullptr,
                           const unsigned char* measured = nullptr) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
#define TK_ICROP(MODE)                                                                        \
  hipLaunchKernelGGL((ifft2_crop_v2_kernel<N, MODE, PASS2>), dim3(tk_grid(ntile, 4)), dim3(N), \
                     0, stream, far, work, chi, ntile, pw, scale, tw, gscale, S, mode_scale, \
                     measured)
  if (gscale && mode_scale && measured)
    TK_ICROP(3);
  else if (gscale && mode_scale)
    TK_ICROP(2);
  else if (gscale)
    TK_ICROP(1);
  else
    TK_ICROP(0);
#undef TK_ICROP
  TK_LAUNCH_CHECK();
  return TK_OK;
}

__global__ __launch_bounds__(256) void crop_kernel(const cf* __restrict__ src,
                                                   cf* __restrict__ dst, long ntile, int det,
                                                   int pw) {
  const int pad = (det - pw) / 2;
  const long nrow = ntile * pw;
  for (long r = blockIdx.x; r < nrow; r += gridDim.x) {
    const long t = r / pw;
    const int py = (int)(r % pw);
    for (int px = threadIdx.x; px < pw; px += blockDim.x)
      dst[(t * pw + py) * pw + px] = src[(t * det + pad + py) * (long)det + pad + px];
  }
}

template <int N>
static int launch_icrop(const cf* far, cf* work, cf* chi, long ntile, int pw, float scale,
                        hipStream_t stream) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  hipLaunchKernelGGL((ifft2_crop_kernel<N>), dim3(tk_grid(ntile, N >= 512 ? 2 : 4)),
                     dim3(FftPlan<N>::NT), 0, stream, far, work, chi, ntile, pw, scale, tw);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// work: (ntile, det, det) scratch for the intermediate; may alias farplane
// (overwrite) and, when pw == det, chi may alias work.
extern "C" int tike_ifft2_crop(const void* farplane, void* work, void* chi, long ntile, int det,
                               int pw, float scale, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && work && chi && ntile >= 0 && pw >= 1 && det >= pw);
  TK_CHECK_ARG(!(chi == work && pw != det));
  if (ntile == 0) return TK_OK;
  const cf* far = (const cf*)farplane;
  cf* wk = (cf*)work;
  cf* out = (cf*)chi;
  if ((const cf*)wk != far) {
    switch (det) {
      case 128: return launch_icrop_v2<128>(far, wk, out, ntile, pw, scale, stream);
      case 256: return launch_icrop_v2<256>(far, wk, out, ntile, pw, scale, stream);
      case 512: return launch_icrop_v2<512>(far, wk, out, ntile, pw, scale, stream);
      default: break;
    }
  }
  switch (det) {
    case 32: return launch_icrop<32>(far, wk, out, ntile, pw, scale, stream);
    case 64: return launch_icrop<64>(far, wk, out, ntile, pw, scale, stream);
    case 128: return launch_icrop<128>(far, wk, out, ntile, pw, scale, stream);
    case 256: return launch_icrop<256>(far, wk, out, ntile, pw, scale, stream);
    case 512: return launch_icrop<512>(far, wk, out, ntile, pw, scale, stream);
    case 1024: return launch_icrop<1024>(far, wk, out, ntile, pw, scale, stream);
    default: break;
  }
  int rc = tk_fft2(far, wk, ntile, det, 1, scale, stream);
  if (rc) return rc;
  if (out == wk) return TK_OK;
  hipLaunchKernelGGL(crop_kernel, dim3(tk_grid(ntile * pw, 16)), dim3(256), 0, stream, wk, out,
                     ntile, det, pw);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ------------------------------------------- intensity / cost / gradient
// One workgroup per position.  For every detector pixel: I = sum_s |F_s|^2;
// cost contribution on measured pixels; F_s *= g with
//   gaussian: g = -(1 - sqrt(d) / (sqrt(I) + 1e-9))       (objective.py:31-44)
//   poisson:  g = -(1 - d / (I + 1e-9))                   (objective.py:97-109)
// on measured pixels and g = (unmeasured_scaling - 1) elsewhere
// (lstsq.py:491-502).  Unmeasured pixels are selected by the mask and their
// data values (possibly NaN) are never read into the arithmetic.
// Grid: (pixel blocks, positions); a workgroup covers TK_FG_PIX pixels of one
// position and adds its share of the cost with one atomic.

template <int MODEL, bool GRAD>
__global__ __launch_bounds__(256) void farplane_gradient_kernel(
    cf* __restrict__ farplane, const float* __restrict__ data,
    const unsigned char* __restrict__ mask, float* __restrict__ intensity,
    const TkCostSink costs, int nscan, int S, int det, float unmeasured_scaling,
    float inv_nmeasured, const int* __restrict__ skip) {
  __shared__ float red[4];
  if (skip != nullptr && *skip != 0) return;  // speculative launch, not needed
  const long npix = (long)det * det;
  const long n = blockIdx.y;
  cf* __restrict__ F = farplane + n * S * npix;
  const float* __restrict__ d = data + n * npix;
  float cost = 0.f;
  const long p0 = (long)blockIdx.x * TK_FG_PIX;
  const long p1 = p0 + TK_FG_PIX < npix ? p0 + TK_FG_PIX : npix;
  for (long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    // the count is requested WITH the wave values, not behind the mask test
    // (a load inside a branch waits for everything in front of the branch);
    // an unmeasured pixel may hold NaN: selected away, never multiplied
    const float dv = d[p];
    const bool measured = mask ? mask[p] != 0 : true;
    float I = 0.f;
    for (int s = 0; s < S; ++s) I += norm2(F[s * npix + p]);
    if (intensity) intensity[n * npix + p] = I;
    float g, term;
    if (MODEL == 0) {
      const float sI = sqrtf(I), sd = sqrtf(dv);
      const float diff = sI - sd;
      term = diff * diff;
      g = -(1.0f - sd / (sI + 1e-9f));
    } else {
      term = I - dv * logf(I + 1e-9f);
      g = -(1.0f - dv / (I + 1e-9f));
    }
    cost += measured ? term : 0.f;
    g = measured ? g : unmeasured_scaling - 1.0f;
    if (GRAD)
      for (int s = 0; s < S; ++s) F[s * npix + p] = F[s * npix + p] * g;
  }
  if (costs.costs) {
    cost = tk_block_sum256(cost, red);
    if (threadIdx.x == 0) tk_cost_add(costs, n, (int)blockIdx.x, cost * inv_nmeasured);
  }
}

int tk_farplane_gradient(void* farplane, const float* data, const unsigned char* measured,
                                float* intensity, float* costs, int nscan, int S, int det,
                                int model, int apply_gradient, float unmeasured_scaling,
                                long num_measured, hipStream_t stream, const int* skip) {
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && det >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured > 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(farplane && data);
  const float inv = 1.0f / (float)num_measured;
  const long npix = (long)det * det;
  // positions in gridDim.y, in slices of at most the device's limit: every
  // pointer (and the cost sink) advanced to the slice's first position
  TK_GRID_Y_LIMIT(ymax);
  const unsigned gx = (unsigned)((npix + TK_FG_PIX - 1) / TK_FG_PIX);
  const dim3 block(256);
  TkCostSink sink{costs, nullptr, 0};
  if (skip == nullptr) {
    int rc = tk_cost_sink(costs, nscan, (int)gx, stream, &sink);
    if (rc) return rc;
  } else if (costs) {
    tk_zero_costs_unless_skipped(costs, nscan, skip, stream);
  }
#define TK_FG(M, G)                                                                          \
  hipLaunchKernelGGL((farplane_gradient_kernel<M, G>), grid, block, 0, stream,               \
                     (cf*)farplane + lo * S * npix, data + lo * npix, measured,              \
                     intensity ? intensity + lo * npix : intensity, part, m, S, det,         \
                     unmeasured_scaling, inv, skip)
  for (long lo = 0; lo < nscan; lo += ymax) {
    const int m = (int)(nscan - lo < ymax ? nscan - lo : ymax);
    const dim3 grid(gx, (unsigned)m);
    const TkCostSink part{sink.costs ? sink.costs + lo : nullptr,
                          sink.part ? sink.part + lo * sink.nslots : nullptr, sink.nslots};
    if (model == 0 && apply_gradient) TK_FG(0, true);
    if (model == 0 && !apply_gradient) TK_FG(0, false);
    if (model == 1 && apply_gradient) TK_FG(1, true);
    if (model == 1 && !apply_gradient) TK_FG(1, false);
  }
#undef TK_FG
#undef TK_FG_K
  TK_LAUNCH_CHECK();
  return tk_cost_finish(sink, nscan, stream);
}

extern "C" int tike_farplane_gradient(void* farplane, const float* data,
                                      const unsigned char* measured, float* intensity,
                                      float* costs, int nscan, int S, int det, int model,
                                      int apply_gradient, float unmeasured_scaling,
                                      long num_measured, void* stream_) {
  TK_ENTER();
  return tk_farplane_gradient(farplane, data, measured, intensity, costs, nscan, S, det, model,
                              apply_gradient, unmeasured_scaling, num_measured,
                              (hipStream_t)stream_, nullptr);
}

// ------------------------------------------------ gradient scale from intensity
// gscale[n][p] = -(1 - sqrt(d)/(sqrt(I)+1e-9))  (gaussian; poisson: -(1 - d/(I+1e-9)))
// on measured pixels, (unmeasured_scaling - 1) elsewhere; costs[n] = mean over
// measured pixels of the per-pixel cost (objective.py:11-124, lstsq.py:444-502).
template <int MODEL>
__global__ __launch_bounds__(256) void gradient_scale_kernel(
    const float* __restrict__ intensity, const float* __restrict__ data,
    const unsigned char* __restrict__ mask, float* __restrict__ gscale,
    const TkCostSink costs, int det, float unmeasured_scaling, float inv_nmeasured) {
  __shared__ float red[4];
  const long npix = (long)det * det;
  const long n = blockIdx.y;
  float cost = 0.f;
  const long p0 = (long)blockIdx.x * TK_FG_PIX;
  const long p1 = p0 + TK_FG_PIX < npix ? p0 + TK_FG_PIX : npix;
  for (long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const float I = intensity[n * npix + p];
    const float dv = data[n * npix + p];  // with I, not behind the mask test
    const bool measured = mask ? mask[p] != 0 : true;
    float g, term;
    if (MODEL == 0) {
      const float sI = sqrtf(I), sd = sqrtf(dv);
      const float diff = sI - sd;
      term = diff * diff;
      g = -(1.0f - sd / (sI + 1e-9f));
    } else {
      term = I - dv * logf(I + 1e-9f);
      g = -(1.0f - dv / (I + 1e-9f));
    }
    cost += measured ? term : 0.f;
    gscale[n * npix + p] = measured ? g : unmeasured_scaling - 1.0f;
  }
  if (costs.costs) {
    cost = tk_block_sum256(cost, red);
    if (threadIdx.x == 0) tk_cost_add(costs, n, (int)blockIdx.x, cost * inv_nmeasured);
  }
}

extern "C" int tike_gradient_scale(const float* intensity, const float* data,
                                   const unsigned char* measured, float* gscale, float* costs,
                                   int nscan, int det, int model, float unmeasured_scaling,
                                   long num_measured, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && det >= 1 && (model == 0 || model == 1) && num_measured > 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(intensity && data && gscale);
  const float inv = 1.0f / (float)num_measured;
  const long npix = (long)det * det;
  TK_GRID_Y_LIMIT(ymax);  // positions in gridDim.y, in slices of at most the limit
  const unsigned gx = (unsigned)((npix + TK_FG_PIX - 1) / TK_FG_PIX);
  const dim3 block(256);
  TkCostSink sink;
  int rc = tk_cost_sink(costs, nscan, (int)gx, stream, &sink);
  if (rc) return rc;
  for (long lo = 0; lo < nscan; lo += ymax) {
    const dim3 grid(gx, (unsigned)(nscan - lo < ymax ? nscan - lo : ymax));
    const TkCostSink part{sink.costs ? sink.costs + lo : nullptr,
                          sink.part ? sink.part + lo * sink.nslots : nullptr, sink.nslots};
    const float* I = intensity + lo * npix;
    const float* d = data + lo * npix;
    float* g = gscale + lo * npix;
    if (model == 0)
      hipLaunchKernelGGL((gradient_scale_kernel<0>), grid, block, 0, stream, I, d, measured, g,
                         part, det, unmeasured_scaling, inv);
    else
      hipLaunchKernelGGL((gradient_scale_kernel<1>), grid, block, 0, stream, I, d, measured, g,
                         part, det, unmeasured_scaling, inv);
  }
  TK_LAUNCH_CHECK();
  return tk_cost_finish(sink, nscan, stream);
}

// IFFT2 + crop of (farplane * gscale): gscale (ntile / S, det, det) f32 is
// shared by the S modes of a position.  work must not alias farplane.
extern "C" int tike_ifft2_crop_scaled(const void* farplane, const float* gscale, int S,
                                      void* work, void* chi, long ntile, int det, int pw,
                                      float scale, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(ntile >= 0 && S >= 1 && pw >= 1 && det >= pw);
  if (ntile == 0) return TK_OK;
  TK_CHECK_ARG(farplane && gscale && work && chi && work != farplane && ntile % S == 0);
  TK_CHECK_ARG(!(chi == work && pw != det));
  switch (det) {
    case 128:
      return launch_icrop_v2<128>((const cf*)farplane, (cf*)work, (cf*)chi, ntile, pw, scale,
                                  stream, gscale, S);
    case 256:
      return launch_icrop_v2<256>((const cf*)farplane, (cf*)work, (cf*)chi, ntile, pw, scale,
                                  stream, gscale, S);
    case 512:
      return launch_icrop_v2<512>((const cf*)farplane, (cf*)work, (cf*)chi, ntile, pw, scale,
                                  stream, gscale, S);
    default:
      return TK_ERR_UNSUPPORTED;
  }
}

// ------------------------------------------- gradient + inverse, no far plane
// Consumes the column-pass input left by tike_ptycho_fwd_intensity_only.  Per
// tile and per k1 (a thread owns one column):
//   F[k1 + 16 k2] = radix-16 over r of rows 16r + k1      (forward column pass)
//   G = F * fwd_scale * gscale                            (lstsq.py:491-502)
// and the inverse transform starts on the same registers: with ky = k1 + 16 k2
// and y = ya + 16 yb,
//   w^-(ky y) = w_16^-(k2 ya) * w_N^-(k1 ya) * w_16^-(k1 yb),
//   A[ya] = w_N^-(k1 ya) * radix-16 over k2 of G          (registers)
//   rows (k1, ya): inverse row transforms                 (LDS, in-wave stages)
//   stored as rows 16 k1 + ya of `work`; after a barrier fft2_pass2 (radix-16
//   over k1, in place, rows {ya + 16 yb}) finishes, crops and scales.
// The far-plane waves are therefore never written to or read from memory.
#ifndef TK_GINV_WAVES
#define TK_GINV_WAVES 4
#endif
template <int N, int MODE, bool PASS2 = true>
__global__ __launch_bounds__(N, TK_GINV_WAVES) void grad_ifft2_crop_kernel(
    const cf* __restrict__ colin, cf* work, cf* chi, long ntile, int pw, float fwd_scale,
    float inv_scale, const cf* __restrict__ twtab, const float* __restrict__ gscale, int S,
    const float* __restrict__ mode_scale, const unsigned char* __restrict__ measured,
    int ksplit) {
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int pad = (N - pw) / 2;
  const int t = threadIdx.x;
  const long nscan = ntile / S;
  // work item = (tile, group of 16 / ksplit values of k1); ksplit > 1 (only
  // without pass 2) lets a small launch fill the chip
  const long nvirt = ((nscan + 7) / 8) * 8 * S;
  const int kn = 16 / ksplit;
  for (long w = blockIdx.x; w < nvirt * ksplit; w += gridDim.x) {
    const long v = w % nvirt;
    const int kbeg = (int)(w / nvirt) * kn;
    const long tile = tk_xcd_tile(v, S, nscan);
    if (tile < 0) continue;  // uniform
    const cf* __restrict__ src = colin + tile * (long)N * N;
    cf* mid = work + tile * (long)N * N;
    cf* dst = chi + tile * (long)pw * pw;
    const float* __restrict__ gs = gscale + (tile / S) * (long)N * N;
    const float ms = MODE == 2 ? mode_scale[tile] : 1.0f;
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    // software pipelined over k1: the 16 rows of k1 + 1 are requested before
    // the butterflies of k1 (1.64 -> 1.60 ms; 7 registers go to scratch at the
    // 128-register cap, a third wave less per SIMD would cost more)
    cf un[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) un[r] = tk_ld_stream(src + (16 * r + kbeg) * N + t);
    for (int k1 = kbeg; k1 < kbeg + kn; ++k1) {
      cf u[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) u[r] = un[r];
      if (k1 + 1 < kbeg + kn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) un[r] = tk_ld_stream(src + (16 * r + k1 + 1) * N + t);
      }
      Dft<16, false>::run(u);
      if constexpr (MODE == 2) {
        // per-mode step on measured pixels: the 16 factors (and mask bytes)
        // are requested together, the step is SELECTED -- a test per pixel
        // around its mask load made 16 serial round trips of them (3.29 ms
        // per 1000 positions x 8 modes against 1.6 ms without the steps)
        float g[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) g[k2] = gs[(k1 + 16 * k2) * N + t];
        if (measured != nullptr) {  // uniform
          unsigned char mb[16];
#pragma unroll
          for (int k2 = 0; k2 < 16; ++k2) mb[k2] = measured[(k1 + 16 * k2) * N + t];
#pragma unroll
          for (int k2 = 0; k2 < 16; ++k2) g[k2] *= mb[k2] ? ms : 1.0f;
        } else {
#pragma unroll
          for (int k2 = 0; k2 < 16; ++k2) g[k2] *= ms;
        }
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) u[k2] = u[k2] * (g[k2] * fwd_scale);
      } else {
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
          const int p = (k1 + 16 * k2) * N + t;
          float g = gs[p] * fwd_scale;
          u[k2] = u[k2] * g;
        }
      }
      Dft<16, true>::run(u);
#pragma unroll
      for (int ya = 1; ya < 16; ++ya) u[ya] = mul_tw<true>(u[ya], twtab[N + k1 * ya]);
      fft2_rows_from_columns<N, true, !PASS2>(lds, tw, line, j, u, mid + (long)(16 * k1) * N);
    }
    if constexpr (PASS2) {
      __syncthreads();
      for (int ya = 0; ya < 16; ++ya)
        fft2_pass2<N, true>(mid, ya, [&](int y, int x, cf v) {
          const int py = y - pad, px = x - pad;
          if (py >= 0 && py < pw && px >= 0 && px < pw)
            tk_st_stream(dst + py * pw + px, v * inv_scale);
        });
      __syncthreads();
    }
  }
}

// ---- column pass + gradient factor + inverse pass 1 in ONE kernel (256^2)
// tike_fwd_gradient_scale and tike_grad_ifft2_pass1 both stream the hand-off:
// the factor g of rows {k1 + 16 k2} needs |F_s|^2 of ALL modes of exactly those
// rows, and the inverse's pass 1 for (tile, k1) needs exactly that g -- so one
// work item (position, k1) can do both: sweep A re-forms F_s row by row for
// the intensity (F discarded), g stays in 16 registers, sweep B re-reads the
// same 16 rows of every mode -- newest first, they are the likeliest to be
// cached still -- re-forms F_s, scales, and runs the inverse's pass 1 on the
// same registers.  The factor never goes through memory and the second read
// of the hand-off is served partly by the caches.  Gaussian / poisson without
// per-mode steps (those need the intensity between the two sweeps).  The path
// for S < TK_FG_RESIDENT_MIN_MODES; more modes: the resident kernel (fwd_grad_resident.h).
// measured (tools/fg_probe.py, 8000 tiles): S = 3 1.91 vs 2.22 ms, 4 1.87 / 1.89, 5 1.86 / 1.91,
// 6 1.89 / 1.77, 7 1.86 / 1.78, 8 1.97 / 1.67 (two sweeps / resident)

//
// BACK (the last slice of a multislice object, rpie.py:444-472): the wave the
// slices in front receive is FresnelSpectProp.adj applied b times to chi =
// IFFT2(G), i.e. IFFT2(conj(H) FFT2(IFFT2(G))) = IFFT2(conj(H)^b G) -- the
// forward transform of the step back cancels against the inverse that formed
// chi (probe window = detector).  G is in registers here, so the kernel also
// emits the inverse's pass 1 of conj(H)^b G, b = 1 .. nback, into work + b *
// back_stride: the steps back cost one more store each instead of a stored
// chi, a forward pass 1 and a column pass.
template <int MODEL, class DT, bool BACK = false, bool MK = true>
__global__ __launch_bounds__(256, BACK ? 2 : 3) void fwd_grad_ifft2_pass1_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, const TkCostSink costs, cf* __restrict__ work,
    long nscan, int S, float fwd_scale, float unmeasured_scaling, float inv_nmeasured,
    const cf* __restrict__ twtab, const cf* __restrict__ backprop = nullptr, int nback = 0,
    long back_stride = 0) {
  constexpr int N = 256;
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  __shared__ float red[4];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int t = threadIdx.x;
  const float s2 = fwd_scale * fwd_scale;
  for (long v = blockIdx.x; v < nscan * 16; v += gridDim.x) {
    const int k1 = (int)(v & 15);
    const long n = nscan - 1 - (v >> 4);  // descending: see fwd_gradient_scale_kernel
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    // ---- sweep A: intensity of rows k1 + 16 k2, all modes (pipelined loads)
    float I[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) I[k2] = 0.f;
    cf un[16];
    {
      const cf* __restrict__ src0 = colin + (n * S) * (long)N * N + k1 * N + t;
#pragma unroll
      for (int r = 0; r < 16; ++r) un[r] = tk_ld_stream(src0 + (long)(16 * r) * N);
    }
    for (int s = 0; s < S; ++s) {
      cf u[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) u[r] = un[r];
      // next: mode s + 1 of sweep A, or the first mode of sweep B (S - 1 again)
      {
        const int sn = s + 1 < S ? s + 1 : S - 1;
        const cf* __restrict__ src = colin + (n * S + sn) * (long)N * N + k1 * N + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) un[r] = src[(long)(16 * r) * N];
      }
      Dft<16, false>::run(u);
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) I[k2] += norm2(u[k2]) * s2;
    }
    // ---- the factor (times the forward scale the inverse applies to F) and the cost
    float cost;
    {
      DT raw[16];
      unsigned bits;
      tk_request_data16(data, !MK ? (const unsigned char*)nullptr : mask, n, k1, t, raw, bits);
      cost = tk_gradient_factor16<MODEL>(I, raw, bits, unmeasured_scaling, fwd_scale);
    }
    if (costs.costs) {
      cost = tk_block_sum256(cost, red);
      if (threadIdx.x == 0) tk_cost_add(costs, n, k1, cost * inv_nmeasured);
    }
    // ---- sweep B: modes S - 1 .. 0, gradient and the inverse's pass 1
    for (int s = S - 1; s >= 0; --s) {
      cf u[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) u[r] = un[r];
      if (s > 0) {
        const cf* __restrict__ src = colin + (n * S + s - 1) * (long)N * N + k1 * N + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) un[r] = src[(long)(16 * r) * N];
      }
      Dft<16, false>::run(u);
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) u[k2] = u[k2] * I[k2];
      cf g[BACK ? 16 : 1];
      if (BACK) {
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) g[BACK ? k2 : 0] = u[k2];
      }
      Dft<16, true>::run(u);
#pragma unroll
      for (int ya = 1; ya < 16; ++ya) u[ya] = mul_tw<true>(u[ya], twtab[N + k1 * ya]);
      cf* mid = work + (n * S + s) * (long)N * N;
      fft2_rows_from_columns<N, true, true>(lds, tw, line, j, u, mid + (long)(16 * k1) * N);
      if (BACK) {
        for (int b = 1; b <= nback; ++b) {
#pragma unroll
          for (int k2 = 0; k2 < 16; ++k2) {
            g[BACK ? k2 : 0] = g[BACK ? k2 : 0] * conjf(*tk_at_pinned(backprop + (k1 + 16 * k2) * N, (unsigned)t * 8u));
            u[k2] = g[BACK ? k2 : 0];
          }
          Dft<16, true>::run(u);
#pragma unroll
          for (int ya = 1; ya < 16; ++ya) u[ya] = mul_tw<true>(u[ya], twtab[N + k1 * ya]);
          fft2_rows_from_columns<N, true, true>(lds, tw, line, j, u,
                                                mid + b * back_stride + (long)(16 * k1) * N);
        }
      }
    }
  }
}

// ---- one mode: the column-pass values of the work item are 16 registers per
// thread, so there is no second sweep at all (cgrad's gradient pass, S = 1)
template <int MODEL, class DT, bool MK = true>
__global__ __launch_bounds__(256, 4) void fwd_grad_ifft2_pass1_single_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, const TkCostSink costs, cf* __restrict__ work,
    long nscan, float fwd_scale, float unmeasured_scaling, float inv_nmeasured,
    const cf* __restrict__ twtab) {
  constexpr int N = 256;
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  __shared__ float red[4];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int t = threadIdx.x;
  const float s2 = fwd_scale * fwd_scale;
  for (long v = blockIdx.x; v < nscan * 16; v += gridDim.x) {
    const int k1 = (int)(v & 15);
    const long n = nscan - 1 - (v >> 4);  // descending: see fwd_gradient_scale_kernel
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    cf u[16];
    {
      const cf* __restrict__ src = colin + n * (long)N * N + k1 * N;  // uniform
#pragma unroll
      for (int r = 0; r < 16; ++r) u[r] = tk_ld_stream(tk_at_pinned(src + (16 * r) * N, t * 8u));
    }
    DT raw[16];
    unsigned bits;
    tk_request_data16(data, !MK ? (const unsigned char*)nullptr : mask, n, k1, t, raw, bits);
    Dft<16, false>::run(u);
    float I[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) I[k2] = norm2(u[k2]) * s2;
    float cost = tk_gradient_factor16<MODEL>(I, raw, bits, unmeasured_scaling, fwd_scale);
    if (costs.costs) {
      cost = tk_block_sum256(cost, red);
      if (threadIdx.x == 0) tk_cost_add(costs, n, k1, cost * inv_nmeasured);
    }
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) u[k2] = u[k2] * I[k2];
    Dft<16, true>::run(u);
#pragma unroll
    for (int ya = 1; ya < 16; ++ya) u[ya] = mul_tw<true>(u[ya], twtab[N + k1 * ya]);
    cf* mid = work + n * (long)N * N;
    fft2_rows_from_columns<N, true, true>(lds, tw, line, j, u, mid + (long)(16 * k1) * N);
  }
}

// The same at 512^2 (RB = 32): per tile and k1 a thread owns one column,
//   F[k1 + 16 k2] = radix-32 over r of rows 16 r + k1 of the hand-off, times g;
// the 32 rows it then holds are exactly TWO input groups of the inverse's pass
// 1 (rows of residue k1 and k1 + 16 mod 32: k2 even / odd), so they go through
// LDS into the row layout and through fft2_pass1 -- the result is the
// intermediate tike_ifft2_pass1_scaled would have produced from a stored far
// plane, which tike_ifft2_pass2_gradients finishes.
template <int MODE>
__global__ __launch_bounds__(512, 2) void grad_ifft2_pass1_512_kernel(
    const cf* __restrict__ colin, cf* __restrict__ work, long ntile, float fwd_scale,
    const cf* __restrict__ twtab, const float* __restrict__ gscale, int S,
    const float* __restrict__ mode_scale, const unsigned char* __restrict__ measured) {
  constexpr int N = 512;
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int t = threadIdx.x;
  const long nscan = ntile / S;
  const long nvirt = ((nscan + 7) / 8) * 8 * S;
  for (long w = blockIdx.x; w < nvirt * 16; w += gridDim.x) {
    const long tile = tk_xcd_tile(w % nvirt, S, nscan);
    const int k1 = (int)(w / nvirt);
    if (tile < 0) continue;  // uniform
    const cf* __restrict__ src = colin + tile * (long)N * N;
    cf* __restrict__ mid = work + tile * (long)N * N;
    const float* __restrict__ gs = gscale + (tile / S) * (long)N * N;
    const float ms = MODE == 2 ? mode_scale[tile] : 1.0f;
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    cf u[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) u[r] = tk_ld_stream(src + (16 * r + k1) * N + t);
    Dft<32, false>::run(u);
    if constexpr (MODE == 2) {
      // (factors and mask bytes requested together, the step selected: see
      // grad_ifft2_crop_kernel)
      float g[32];
#pragma unroll
      for (int k2 = 0; k2 < 32; ++k2) g[k2] = gs[(k1 + 16 * k2) * N + t];
      if (measured != nullptr) {  // uniform
        unsigned char mb[32];
#pragma unroll
        for (int k2 = 0; k2 < 32; ++k2) mb[k2] = measured[(k1 + 16 * k2) * N + t];
#pragma unroll
        for (int k2 = 0; k2 < 32; ++k2) g[k2] *= mb[k2] ? ms : 1.0f;
      } else {
#pragma unroll
        for (int k2 = 0; k2 < 32; ++k2) g[k2] *= ms;
      }
#pragma unroll
      for (int k2 = 0; k2 < 32; ++k2) u[k2] = u[k2] * (g[k2] * fwd_scale);
    } else {
#pragma unroll
      for (int k2 = 0; k2 < 32; ++k2) {
        const int p = (k1 + 16 * k2) * N + t;
        float g = gs[p] * fwd_scale;
        u[k2] = u[k2] * g;
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // rows k1 + 16 h + 32 y2 (column t) -> row layout of pass-1 group k1 + 16 h
#pragma unroll
      for (int y2 = 0; y2 < 16; ++y2) lds[y2 * G2::LS + tk_pad16(t)] = u[2 * y2 + h];
      __syncthreads();
      const cf* __restrict__ lrow = lds + line * G2::LS;
      fft2_pass1<N, true, true>(
          lds, twtab, tw, line, j, k1 + 16 * h,
          [&](int, int e, auto) { return lrow[tk_pad16(e)]; }, mid);
    }
  }
}

// ---- 512^2: column pass + gradient factor + inverse pass 1 in ONE launch.
// The resident form of 256^2 does not exist here -- F of four modes is 4 x 32
// values per column = 256 registers before anything else, and splitting the
// 512 columns over two half-workgroups (as the modes are split at 256^2) would
// break the inverse's row transforms, which need whole rows -- so this is the
// two-sweep form: sweep A re-forms F_s mode by mode for the intensity (F
// discarded, the factor stays in 32 registers), sweep B re-reads the 32 rows
// of every mode, newest first -- 512 KiB per work item, in flight 128 MiB over
// the chip: the second read is the Infinity Cache's, not HBM's -- applies the
// factor and sends the two 16-row groups it holds (residues k1 and k1 + 16 mod
// 32) through the inverse's pass 1.  Against the two launches it replaces
// (tike_fwd_gradient_scale + tike_grad_ifft2_pass1) the factor never goes
// through memory and HBM sees the hand-off once.

template <int MODEL, class DT, bool MK = true>
__global__ __launch_bounds__(512, 2) void fwd_grad_ifft2_pass1_512_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, const TkCostSink costs, cf* __restrict__ work,
    long nscan, int S, float fwd_scale, float unmeasured_scaling, float inv_nmeasured,
    const cf* __restrict__ twtab) {
  constexpr int N = 512;
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  __shared__ float red[8];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int t = threadIdx.x;
  const float s2 = fwd_scale * fwd_scale;
  for (long v = blockIdx.x; v < nscan * 16; v += gridDim.x) {
    const int k1 = (int)(v & 15);
    const long n = nscan - 1 - (v >> 4);  // descending: see fwd_gradient_scale_kernel
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    // ---- sweep A: intensity of rows k1 + 16 k2 over the modes
    float I[32];
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) I[k2] = 0.f;
    for (int s = 0; s < S; ++s) {
      const cf* __restrict__ src = colin + (n * S + s) * (long)N * N + k1 * N + t;
      cf u[32];
#pragma unroll
      for (int r = 0; r < 32; ++r) u[r] = src[(long)(16 * r) * N];
      Dft<32, false>::run(u);
#pragma unroll
      for (int k2 = 0; k2 < 32; ++k2) I[k2] += norm2(u[k2]) * s2;
    }
    // ---- the factor (times the forward scale the inverse applies to F), the cost
    float cost;
    {
      DT raw[32];
      unsigned bits;
      tk_request_data<N, 32>(data, !MK ? (const unsigned char*)nullptr : mask, n, k1, t, raw, bits);
      cost = tk_gradient_factor<MODEL, 32>(I, raw, bits, unmeasured_scaling, fwd_scale);
    }
    if (costs.costs) {
      cost = tk_block_sum512(cost, red);
      if (threadIdx.x == 0) tk_cost_add(costs, n, k1, cost * inv_nmeasured);
    }
    // ---- sweep B: modes S - 1 .. 0 (the likeliest to be cached still first)
    for (int s = S - 1; s >= 0; --s) {
      const cf* __restrict__ src = colin + (n * S + s) * (long)N * N + k1 * N + t;
      cf* __restrict__ mid = work + (n * S + s) * (long)N * N;
      cf u[32];
#pragma unroll
      for (int r = 0; r < 32; ++r) u[r] = tk_ld_stream(src + (long)(16 * r) * N);
      Dft<32, false>::run(u);
#pragma unroll
      for (int k2 = 0; k2 < 32; ++k2) u[k2] = u[k2] * I[k2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // rows k1 + 16 h + 32 y2 (column t) -> row layout of pass-1 group k1 + 16 h
#pragma unroll
        for (int y2 = 0; y2 < 16; ++y2) lds[y2 * G2::LS + tk_pad16(t)] = u[2 * y2 + h];
        __syncthreads();
        const cf* __restrict__ lrow = lds + line * G2::LS;
        fft2_pass1<N, true, true>(
            lds, twtab, tw, line, j, k1 + 16 * h,
            [&](int, int e, auto) { return lrow[tk_pad16(e)]; }, mid);
      }
    }
  }
}

static int launch_grad_ifft2(const void* colin, const float* gscale, const float* mode_scale,
                             const unsigned char* measured, int S, void* work, void* chi,
                             long ntile, int pw, float fwd_scale, float inv_scale,
                             hipStream_t stream, bool pass2) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  constexpr int N = 256;
  // a multiple of 8 workgroups keeps "virtual block % 8" equal to the XCD of
  // the workgroup across the grid-stride loop
  const long nvirt = ((ntile / S + 7) / 8) * 8 * S;
  // without pass 2 the 16 values of k1 of a tile are independent: split them
  // when there are fewer tiles than the chip holds workgroups
  int ksplit = 1;
  if (!pass2)
    while (ksplit < 16 && nvirt * ksplit < 2048) ksplit *= 2;
  const int grid8 = (tk_grid(nvirt * ksplit, 4) + 7) / 8 * 8;
#define TK_GINV(MODE, P2)                                                                      \
  hipLaunchKernelGGL((grad_ifft2_crop_kernel<N, MODE, P2>), dim3(grid8), dim3(N), 0,            \
                     stream, (const cf*)colin, (cf*)work, (cf*)chi, ntile, pw, fwd_scale,      \
                     inv_scale, tw, gscale, S, mode_scale, measured, ksplit)
  if (mode_scale && pass2)
    TK_GINV(2, true);
  else if (mode_scale)
    TK_GINV(2, false);
  else if (pass2)
    TK_GINV(1, true);
  else
    TK_GINV(1, false);
#undef TK_GINV
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_grad_ifft2_crop(const void* colin, const float* gscale,
                                    const float* mode_scale, const unsigned char* measured,
                                    int S, void* work, void* chi, long ntile, int det, int pw,
                                    float fwd_scale, float inv_scale, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(ntile >= 0 && S >= 1 && pw >= 1 && det >= pw);
  if (ntile == 0) return TK_OK;
  TK_CHECK_ARG(colin && gscale && work && chi && work != colin && ntile % S == 0);
  TK_CHECK_ARG(!(chi == work && pw != det));
  if (det != 256) return TK_ERR_UNSUPPORTED;
  return launch_grad_ifft2(colin, gscale, mode_scale, measured, S, work, chi, ntile, pw,
                           fwd_scale, inv_scale, stream, true);
}

// Pass 1 only of tike_grad_ifft2_crop: `work` receives the input of the inverse
// column pass (rows 16 k1 + ya), consumed by tike_ifft2_pass2_gradients.
// scratch: from tike_fwd_pass1.  costs (may be NULL) must not need zeroing by
// the caller (done here); work must not alias scratch.  det = 256 or 512.
static int launch_fwd_grad_ifft2_pass1(const void* scratch, const void* data, int data_u16,
                                       const unsigned char* measured, float* costs, void* work,
                                       int nscan, int S, int det, float fwd_scale, int model,
                                       float unmeasured_scaling, long num_measured,
                                       const cf* backprop, int nback, hipStream_t stream) {
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && det >= 1 && (model == 0 || model == 1) &&
               num_measured > 0 && nback >= 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(scratch && data && work && work != scratch && (nback == 0 || backprop));
  if (det != 256 && (det != 512 || nback > 0)) return TK_ERR_UNSUPPORTED;
  const long back_stride = (long)nscan * S * det * det;
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  if (det == 512) {
    TkCostSink sink512;
    int rc = tk_cost_sink(costs, nscan, 16, stream, &sink512);
    if (rc) return rc;
    const float inv512 = 1.0f / (float)num_measured;
    const dim3 grid(tk_grid((long)nscan * 16, 2)), block(512);
#define TK_FG512_K(M, DT, MK_)                                                                \
  hipLaunchKernelGGL((fwd_grad_ifft2_pass1_512_kernel<M, DT, MK_>), grid, block, 0, stream,   \
                     (const cf*)scratch, (const DT*)data, measured, sink512, (cf*)work,       \
                     (long)nscan, S, fwd_scale, unmeasured_scaling, inv512, tw)
#define TK_FG512(M, DT)           \
  do {                            \
    if (measured != nullptr)      \
      TK_FG512_K(M, DT, true);    \
    else                          \
      TK_FG512_K(M, DT, false);   \
  } while (0)
    if (model == 0 && data_u16)
      TK_FG512(0, unsigned short);
    else if (model == 0)
      TK_FG512(0, float);
    else if (data_u16)
      TK_FG512(1, unsigned short);
    else
      TK_FG512(1, float);
#undef TK_FG512
#undef TK_FG512_K
    TK_LAUNCH_CHECK();
    return tk_cost_finish(sink512, nscan, stream);
  }
  // (nback > 0: the two-sweep kernel for any number of modes -- a BACK form of
  // the resident kernel, G of the mode in hand parked in LDS, was 10 % slower:
  // 3.13 vs 2.81 ms per 1000 positions x 8 modes x 2 slices)
  const bool resident = S >= TK_FG_RESIDENT_MIN_MODES && S <= 8 && nback == 0;
  // contributors per pattern: (k1, wave of the first half) / (k1)
  TkCostSink sink;
  {
    int rc = tk_cost_sink(costs, nscan, resident ? 64 : 16, stream, &sink);
    if (rc) return rc;
  }
  const float inv = 1.0f / (float)num_measured;
  if (resident) {
    // one 512-thread workgroup per CU (it takes the whole register file)
    const dim3 grid(tk_grid((long)nscan * 16, 1)), block(512);
#define TK_FGR_K(MH, M, DT, MK_)                                                              \
  hipLaunchKernelGGL((fwd_grad_ifft2_pass1_resident_kernel<MH, M, DT, 0, MK_>), grid, block,  \
                     0, stream, (const cf*)scratch, (const DT*)data, measured, sink,          \
                     (cf*)work, (long)nscan, S, fwd_scale, unmeasured_scaling, inv, tw)
#define TK_FGR(MH, M, DT)          \
  do {                             \
    if (measured != nullptr)       \
      TK_FGR_K(MH, M, DT, true);   \
    else                           \
      TK_FGR_K(MH, M, DT, false);  \
  } while (0)
#define TK_FGR_M(MH)                                                                          \
  do {                                                                                        \
    if (model == 0 && data_u16)                                                               \
      TK_FGR(MH, 0, unsigned short);                                                          \
    else if (model == 0)                                                                      \
      TK_FGR(MH, 0, float);                                                                   \
    else if (data_u16)                                                                        \
      TK_FGR(MH, 1, unsigned short);                                                          \
    else                                                                                      \
      TK_FGR(MH, 1, float);                                                                   \
  } while (0)
    if (S == 6)
      TK_FGR_M(3);
    else
      TK_FGR_M(4);
#undef TK_FGR_M
#undef TK_FGR
#undef TK_FGR_K
    TK_LAUNCH_CHECK();
    return tk_cost_finish(sink, nscan, stream);
  }
  const dim3 grid(tk_grid((long)nscan * 16, 12)), block(256);
  if (nback > 0) {  // (one mode too: the two-sweep kernel reads it twice)
#define TK_FGB(M, DT)                                                                         \
  hipLaunchKernelGGL((fwd_grad_ifft2_pass1_kernel<M, DT, true>), grid, block, 0, stream,      \
                     (const cf*)scratch, (const DT*)data, measured, sink, (cf*)work,         \
                     (long)nscan, S, fwd_scale, unmeasured_scaling, inv, tw, backprop, nback, \
                     back_stride)
    if (model == 0 && data_u16)
      TK_FGB(0, unsigned short);
    else if (model == 0)
      TK_FGB(0, float);
    else if (data_u16)
      TK_FGB(1, unsigned short);
    else
      TK_FGB(1, float);
#undef TK_FGB
    TK_LAUNCH_CHECK();
    return tk_cost_finish(sink, nscan, stream);
  }
  if (S == 1) {
#define TK_FG1_K(M, DT, MK_)                                                                  \
  hipLaunchKernelGGL((fwd_grad_ifft2_pass1_single_kernel<M, DT, MK_>), grid, block, 0, stream, \
                     (const cf*)scratch, (const DT*)data, measured, sink, (cf*)work,         \
                     (long)nscan, fwd_scale, unmeasured_scaling, inv, tw)
#define TK_FG1(M, DT)           \
  do {                          \
    if (measured != nullptr)    \
      TK_FG1_K(M, DT, true);    \
    else                        \
      TK_FG1_K(M, DT, false);   \
  } while (0)
    if (model == 0 && data_u16)
      TK_FG1(0, unsigned short);
    else if (model == 0)
      TK_FG1(0, float);
    else if (data_u16)
      TK_FG1(1, unsigned short);
    else
      TK_FG1(1, float);
#undef TK_FG1
#undef TK_FG1_K
    TK_LAUNCH_CHECK();
    return tk_cost_finish(sink, nscan, stream);
  }
#define TK_FG_K(M, DT, MK_)                                                                   \
  hipLaunchKernelGGL((fwd_grad_ifft2_pass1_kernel<M, DT, false, MK_>), grid, block, 0, stream, \
                     (const cf*)scratch, (const DT*)data, measured, sink, (cf*)work,         \
                     (long)nscan, S, fwd_scale, unmeasured_scaling, inv, tw)
#define TK_FG(M, DT)           \
  do {                         \
    if (measured != nullptr)   \
      TK_FG_K(M, DT, true);    \
    else                       \
      TK_FG_K(M, DT, false);   \
  } while (0)
  if (model == 0 && data_u16)
    TK_FG(0, unsigned short);
  else if (model == 0)
    TK_FG(0, float);
  else if (data_u16)
    TK_FG(1, unsigned short);
  else
    TK_FG(1, float);
#undef TK_FG
  TK_LAUNCH_CHECK();
  return tk_cost_finish(sink, nscan, stream);
}

extern "C" int tike_fwd_grad_ifft2_pass1(const void* scratch, const void* data, int data_u16,
                                         const unsigned char* measured, float* costs,
                                         void* work, int nscan, int S, int det, float fwd_scale,
                                         int model, float unmeasured_scaling, long num_measured,
                                         void* stream) {
  TK_ENTER();
  return launch_fwd_grad_ifft2_pass1(scratch, data, data_u16, measured, costs, work, nscan, S,
                                     det, fwd_scale, model, unmeasured_scaling, num_measured,
                                     nullptr, 0, (hipStream_t)stream);
}

// The last slice of a multislice object: work (nslices, nscan, S, det, det);
// work[b] = the inverse's pass 1 of conj(propagator)^b x (far-plane gradient)
// -- what tike_ifft2_pass2_products of slice nslices - 1 - b finishes.
extern "C" int tike_fwd_grad_ifft2_pass1_slices(const void* scratch, const void* data,
                                                int data_u16, const unsigned char* measured,
                                                float* costs, void* work, int nscan, int S,
                                                int det, float fwd_scale, int model,
                                                float unmeasured_scaling, long num_measured,
                                                const void* propagator, int nslices,
                                                void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nslices >= 1);
  return launch_fwd_grad_ifft2_pass1(scratch, data, data_u16, measured, costs, work, nscan, S,
                                     det, fwd_scale, model, unmeasured_scaling, num_measured,
                                     (const cf*)propagator, nslices - 1, (hipStream_t)stream);
}

extern "C" int tike_grad_ifft2_pass1(const void* colin, const float* gscale,
                                     const float* mode_scale, const unsigned char* measured,
                                     int S, void* work, long ntile, int det, float fwd_scale,
                                     void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(ntile >= 0 && S >= 1 && det >= 1);
  if (ntile == 0) return TK_OK;
  TK_CHECK_ARG(colin && gscale && work && work != colin && ntile % S == 0);
  if (det == 512) {
    const cf* tw = tk_twiddles();
    if (!tw) return (int)hipErrorNotInitialized;
    const long nvirt = ((ntile / S + 7) / 8) * 8 * S;
    const int grid8 = (tk_grid(nvirt * 16, 2) + 7) / 8 * 8;
    if (mode_scale)
      hipLaunchKernelGGL((grad_ifft2_pass1_512_kernel<2>), dim3(grid8), dim3(512), 0, stream,
                         (const cf*)colin, (cf*)work, ntile, fwd_scale, tw, gscale, S, mode_scale,
                         measured);
    else
      hipLaunchKernelGGL((grad_ifft2_pass1_512_kernel<1>), dim3(grid8), dim3(512), 0, stream,
                         (const cf*)colin, (cf*)work, ntile, fwd_scale, tw, gscale, S, mode_scale,
                         measured);
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  if (det != 256) return TK_ERR_UNSUPPORTED;
  return launch_grad_ifft2(colin, gscale, mode_scale, measured, S, work, work, ntile, det,
                           fwd_scale, 1.0f, stream, false);
}

// Pass 1 only of tike_ifft2_crop_scaled / _scaled_modes (stored far plane).
extern "C" int tike_ifft2_pass1_scaled(const void* farplane, const float* gscale,
                                       const float* mode_scale, const unsigned char* measured,
                                       int S, void* work, long ntile, int det, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(ntile >= 0 && S >= 1 && det >= 1);
  if (ntile == 0) return TK_OK;
  TK_CHECK_ARG(farplane && gscale && work && work != farplane && ntile % S == 0);
  const cf* far = (const cf*)farplane;
  cf* wk = (cf*)work;
  switch (det) {
    case 128:
      return launch_icrop_v2<128, false>(far, wk, wk, ntile, det, 1.0f, stream, gscale, S,
                                         mode_scale, measured);
    case 256:
      return launch_icrop_v2<256, false>(far, wk, wk, ntile, det, 1.0f, stream, gscale, S,
                                         mode_scale, measured);
    case 512:
      return launch_icrop_v2<512, false>(far, wk, wk, ntile, det, 1.0f, stream, gscale, S,
                                         mode_scale, measured);
    default:
      return TK_ERR_UNSUPPORTED;
  }
}

// Poisson variant (lstsq.py:454-489): the gradient factor of mode s at a
// measured pixel is gscale[n][p] * mode_scale[n][s]; unmeasured pixels keep
// gscale alone.  measured == NULL: every pixel is measured.
extern "C" int tike_ifft2_crop_scaled_modes(const void* farplane, const float* gscale,
                                            const float* mode_scale,
                                            const unsigned char* measured, int S, void* work,
                                            void* chi, long ntile, int det, int pw, float scale,
                                            void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(ntile >= 0 && S >= 1 && pw >= 1 && det >= pw);
  if (ntile == 0) return TK_OK;
  TK_CHECK_ARG(farplane && gscale && mode_scale && work && chi && work != farplane &&
               ntile % S == 0);
  TK_CHECK_ARG(!(chi == work && pw != det));
  switch (det) {
    case 128:
      return launch_icrop_v2<128>((const cf*)farplane, (cf*)work, (cf*)chi, ntile, pw, scale,
                                  stream, gscale, S, mode_scale, measured);
    case 256:
      return launch_icrop_v2<256>((const cf*)farplane, (cf*)work, (cf*)chi, ntile, pw, scale,
                                  stream, gscale, S, mode_scale, measured);
    case 512:
      return launch_icrop_v2<512>((const cf*)farplane, (cf*)work, (cf*)chi, ntile, pw, scale,
                                  stream, gscale, S, mode_scale, measured);
    default:
      return TK_ERR_UNSUPPORTED;
  }
}

// ------------------------------------------------ stand-alone objective ops
// The free functions tike.operators.{gaussian,poisson}{_each_pattern,_grad}
// (objective.py:18-124) and _intensity_from_farplane (ptycho.py:18-23).
__global__ __launch_bounds__(256) void intensity_kernel(const cf* __restrict__ F,
                                                        float* __restrict__ I, long nscan, int S,
                                                        long npix) {
  const long total = nscan * npix;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i / npix, p = i % npix;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += norm2(F[(n * S + s) * npix + p]);
    I[i] = a;
  }
}

template <int MODEL>
__global__ __launch_bounds__(256) void cost_each_kernel(const float* __restrict__ data,
                                                        const float* __restrict__ I,
                                                        float* __restrict__ costs, long nscan,
                                                        long npix) {
  __shared__ float red[4];
  for (long n = blockIdx.x; n < nscan; n += gridDim.x) {
    float c = 0.f;
    for (long p = threadIdx.x; p < npix; p += blockDim.x) {
      const float d = data[n * npix + p], iv = I[n * npix + p];
      if (MODEL == 0) {
        const float diff = sqrtf(iv) - sqrtf(d);
        c += diff * diff;
      } else {
        c += iv - d * logf(iv + 1e-9f);
      }
    }
    c = tk_block_sum256(c, red);
    if (threadIdx.x == 0) costs[n] = c / (float)npix;
  }
}

template <int MODEL>
__global__ __launch_bounds__(256) void objective_grad_kernel(const float* __restrict__ data,
                                                             const cf* __restrict__ F,
                                                             const float* __restrict__ I,
                                                             cf* __restrict__ out, long nscan,
                                                             int S, long npix) {
  const long total = nscan * npix;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i / npix, p = i % npix;
    const float d = data[i], iv = I[i];
    const float g = MODEL == 0 ? 1.0f - sqrtf(d) / (sqrtf(iv) + 1e-9f) : 1.0f - d / (iv + 1e-9f);
    for (int s = 0; s < S; ++s) out[(n * S + s) * npix + p] = F[(n * S + s) * npix + p] * g;
  }
}

extern "C" int tike_intensity(const void* farplane, float* intensity, long nscan, int S,
                              long npix, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(farplane && intensity && nscan >= 0 && S >= 1 && npix >= 1);
  if (nscan == 0) return TK_OK;
  hipLaunchKernelGGL(intensity_kernel, dim3(tk_grid((nscan * npix + 255) / 256, 16)), dim3(256),
                     0, (hipStream_t)stream, (const cf*)farplane, intensity, nscan, S, npix);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_cost_each_pattern(const float* data, const float* intensity, float* costs,
                                      long nscan, long npix, int model, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(data && intensity && costs && nscan >= 0 && npix >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  if (nscan == 0) return TK_OK;
  const dim3 grid(tk_grid(nscan, 16)), block(256);
  if (model == 0)
    hipLaunchKernelGGL((cost_each_kernel<0>), grid, block, 0, (hipStream_t)stream, data,
                       intensity, costs, nscan, npix);
  else
    hipLaunchKernelGGL((cost_each_kernel<1>), grid, block, 0, (hipStream_t)stream, data,
                       intensity, costs, nscan, npix);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_objective_grad(const float* data, const void* farplane,
                                   const float* intensity, void* out, long nscan, int S,
                                   long npix, int model, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(data && farplane && intensity && out && nscan >= 0 && S >= 1 && npix >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  if (nscan == 0) return TK_OK;
  const dim3 grid(tk_grid((nscan * npix + 255) / 256, 16)), block(256);
  if (model == 0)
    hipLaunchKernelGGL((objective_grad_kernel<0>), grid, block, 0, (hipStream_t)stream, data,
                       (const cf*)farplane, intensity, (cf*)out, nscan, S, npix);
  else
    hipLaunchKernelGGL((objective_grad_kernel<1>), grid, block, 0, (hipStream_t)stream, data,
                       (const cf*)farplane, intensity, (cf*)out, nscan, S, npix);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
