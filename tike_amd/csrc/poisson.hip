// Step lengths of the Poisson noise model (reference exitwave.py:122-234),
// for gfx950.
//   tike_poisson_steps*  the per-mode or dominant-mode step lengths, from a
//                        stored far plane or from the hand-off of tike_fwd_pass1;
//   tike_scale_modes     far plane *= the step length of its mode.
#include "fft_engine2.h"
#include "internal.h"
#include "tike_amd.h"
#include "ptycho_shared.h"
#include "fwd_grad_resident.h"

// ---------------------------------------------------- poisson step lengths
// exitwave.py:122-234.  One workgroup per (position, mode) tile; three sweeps
// over the measured pixels (denominator, then two fixed-point updates of the
// step), each closed by a block reduction.  xi = 1 - d / (I + 1e-9).
//   all modes:     denom = sum xi^2 a,   a = |F_s|^2
//                  numer = sum xi a (1 + d (xi alpha - 1) / (a (xi alpha - 1)^2 + I - a))
//   dominant mode: denom = sum xi^2 I
//                  numer = sum xi (I - d / (1 - alpha xi))      (same for all modes)
//   alpha <- (1 - w) alpha + w numer / denom
template <bool DOMINANT>
__global__ __launch_bounds__(256) void poisson_steps_kernel(
    const cf* __restrict__ farplane, const float* __restrict__ intensity,
    const float* __restrict__ data, const unsigned char* __restrict__ mask,
    float* __restrict__ steps, int S, long npix, float start, float w) {
  __shared__ float red[4];
  const long tile = blockIdx.x;  // DOMINANT: position; else position * S + mode
  const long n = DOMINANT ? tile : tile / S;
  const cf* __restrict__ F = farplane + tile * npix;
  const float* __restrict__ I = intensity + n * npix;
  const float* __restrict__ d = data + n * npix;
  float denom = 0.f;
  for (long p = threadIdx.x; p < npix; p += blockDim.x) {
    if (mask && !mask[p]) continue;
    const float Ie = I[p];
    const float xi = 1.0f - d[p] / (Ie + 1e-9f);
    denom += xi * xi * (DOMINANT ? Ie : norm2(F[p]));
  }
  denom = tk_block_sum256(denom, red);
  float alpha = start;
  for (int it = 0; it < 2; ++it) {
    float numer = 0.f;
    for (long p = threadIdx.x; p < npix; p += blockDim.x) {
      if (mask && !mask[p]) continue;
      const float Ie = I[p], Im = d[p];
      const float xi = 1.0f - Im / (Ie + 1e-9f);
      if (DOMINANT) {
        numer += xi * (Ie - Im / (1.0f - alpha * xi));
      } else {
        const float a = norm2(F[p]);
        const float xam1 = xi * alpha - 1.0f;
        numer += xi * a * (1.0f + Im * xam1 / (a * xam1 * xam1 + Ie - a));
      }
    }
    numer = tk_block_sum256(numer, red);
    alpha = alpha * (1.0f - w) + (numer / denom) * w;
  }
  if (threadIdx.x == 0) {
    if (DOMINANT) {
      for (int s = 0; s < S; ++s) steps[n * S + s] = alpha;
    } else {
      steps[tile] = alpha;
    }
  }
}

// All modes of a position in ONE workgroup and TWO sweeps (S <= 8, even pixel
// count): the intensity and the counts of a pixel are read once for its S
// modes, and the first fixed-point update (alpha = start: known) shares its
// sweep with the denominator -- 9 MiB instead of 24 MiB per position at
// 256^2 x 8.  A thread takes U pairs of neighbouring pixels per trip (16-byte
// loads of the waves, 8-byte loads of intensity and counts), every operand
// requested before the first is used: one workgroup per position, nothing else
// hides the latency.  Unmeasured pixels (their counts may be NaN) are selected
// away, never multiplied.
template <int MAXS, int U>
__global__ __launch_bounds__(256) void poisson_steps_allmodes_kernel(
    const cf* __restrict__ farplane, const float* __restrict__ intensity,
    const float* __restrict__ data, const unsigned char* __restrict__ mask,
    float* __restrict__ steps, int S, long npix, float start, float w) {
  typedef float tk_v4 __attribute__((ext_vector_type(4)));
  typedef float tk_v2 __attribute__((ext_vector_type(2)));
  __shared__ float red[4];
  const long n = blockIdx.x;
  const cf* __restrict__ F = farplane + n * S * npix;
  const float* __restrict__ I = intensity + n * npix;
  const float* __restrict__ d = data + n * npix;
  const long npair = npix / 2;
  float denom[MAXS], numer[MAXS], alpha[MAXS];
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    denom[s] = numer[s] = 0.f;
    alpha[s] = start;
  }
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (long q0 = threadIdx.x; q0 < npair; q0 += (long)U * 256) {
      tk_v2 Ie[U], Im[U];
      tk_v4 f[U][MAXS];
      bool meas[U][2];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const long q = q0 + 256L * j;
        const bool in = q < npair;
        const long p = 2 * (in ? q : q0);
        Ie[j] = *reinterpret_cast<const tk_v2*>(I + p);
        Im[j] = *reinterpret_cast<const tk_v2*>(d + p);
        meas[j][0] = in && (mask ? mask[p] != 0 : true);
        meas[j][1] = in && (mask ? mask[p + 1] != 0 : true);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
          if (s < S) f[j][s] = *reinterpret_cast<const tk_v4*>(F + s * npix + p);
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float ie = h ? Ie[j].y : Ie[j].x, im = h ? Im[j].y : Im[j].x;
          const float xi = 1.0f - im / (ie + 1e-9f);
#pragma unroll
          for (int s = 0; s < MAXS; ++s) {
            if (s < S) {
              const float a = h ? f[j][s].z * f[j][s].z + f[j][s].w * f[j][s].w
                                : f[j][s].x * f[j][s].x + f[j][s].y * f[j][s].y;
              const float xam1 = xi * alpha[s] - 1.0f;
              const float t = xi * a * (1.0f + im * xam1 / (a * xam1 * xam1 + ie - a));
              numer[s] += meas[j][h] ? t : 0.f;
              if (sweep == 0) denom[s] += meas[j][h] ? xi * xi * a : 0.f;
            }
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < S) {  // uniform
        if (sweep == 0) denom[s] = tk_block_sum256(denom[s], red);
        const float nm = tk_block_sum256(numer[s], red);
        alpha[s] = alpha[s] * (1.0f - w) + (nm / denom[s]) * w;
        numer[s] = 0.f;
      }
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
      if (s < S) steps[n * S + s] = alpha[s];
  }
}

// ---- the same step lengths WITHOUT a stored far plane (256^2 / 512^2): the
// column pass of fwd_gradient_scale_kernel with |F_s|^2 of all S modes kept in
// registers (S x RB floats), so that one read of the forward hand-off gives
//   FIRST: the poisson gradient factor and the costs (what
//          fwd_gradient_scale_kernel<N, 1, DT> stores) AND the first sweep of
//          exitwave.py:122-184 (denominator; numerator at alpha = start);
//   else : the second sweep (numerator at the alpha of the first).
// sums (nscan, S, 2) = { denominator, numerator } accumulate by atomics (one per
// wave, mode and sum); poisson_alpha_kernel turns them into alpha between and
// after the sweeps.  The far plane itself is never written: the inverse that
// follows (tike_grad_ifft2_pass1) re-forms it from the same hand-off.
template <int N, class DT, bool FIRST>
__global__ __launch_bounds__(256, 2) void poisson_colpass_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, float* __restrict__ gscale,
    float* __restrict__ costs, const float* __restrict__ alpha, float start,
    float* __restrict__ sums, long nitem, int S, float scale, float unmeasured_scaling,
    float inv_nmeasured) {
  constexpr int RB = N / 16, NH = N / 256, MAXS = N == 256 ? 8 : 4;
  __shared__ float red[4];
  __shared__ float wsum[4][2 * MAXS];
  const float s2 = scale * scale;
  for (long v = blockIdx.x; v < nitem; v += gridDim.x) {
    const int hb = (int)(v % NH);
    const int k1 = (int)((v / NH) & 15);
    const long n = nitem / (16 * NH) - 1 - v / (16 * NH);  // descending, as its siblings
    const int t = hb * 256 + threadIdx.x;
    float a[MAXS][RB], I[RB];
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) I[k2] = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < S) {  // uniform
        const cf* __restrict__ src = colin + (n * S + s) * (long)N * N + k1 * N + t;
        cf u[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) u[r] = tk_ld_stream(src + (long)(16 * r) * N);
        Dft<RB, false>::run(u);
#pragma unroll
        for (int k2 = 0; k2 < RB; ++k2) {
          a[s][k2] = norm2(u[k2]) * s2;
          I[k2] += a[s][k2];
        }
      }
    }
    DT raw[RB];
    unsigned bits;
    tk_request_data<N, RB>(data, mask, n, k1, t, raw, bits);
    float den[MAXS], num[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) den[s] = num[s] = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < S) {
        const float al = FIRST ? start : alpha[n * S + s];  // uniform
#pragma unroll
        for (int k2 = 0; k2 < RB; ++k2) {
          const bool meas = (bits >> k2) & 1u;
          const float dv = (float)raw[k2];
          const float xi = 1.0f - dv / (I[k2] + 1e-9f);
          const float xam1 = xi * al - 1.0f;
          const float av = a[s][k2];
          const float tn = xi * av * (1.0f + dv * xam1 / (av * xam1 * xam1 + I[k2] - av));
          num[s] += meas ? tn : 0.f;
          if (FIRST) den[s] += meas ? xi * xi * av : 0.f;
        }
      }
    }
    if (FIRST) {
      float cost = tk_gradient_factor<1, RB>(I, raw, bits, unmeasured_scaling, 1.0f);
      if (gscale != nullptr) {
#pragma unroll
        for (int k2 = 0; k2 < RB; ++k2)
          gscale[n * (long)N * N + (long)(k1 + 16 * k2) * N + t] = I[k2];
      }
      if (costs) {
        cost = tk_block_sum256(cost, red);
        if (threadIdx.x == 0) unsafeAtomicAdd(&costs[n], cost * inv_nmeasured);
      }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      if (s < S) {
        num[s] = tk_wave_sum(num[s]);
        if (FIRST) den[s] = tk_wave_sum(den[s]);
      }
    }
    __syncthreads();  // the previous item's sums have been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int s = 0; s < MAXS; ++s) {
        wsum[threadIdx.x >> 6][2 * s] = den[s];
        wsum[threadIdx.x >> 6][2 * s + 1] = num[s];
      }
    }
    __syncthreads();
    const int q = threadIdx.x;  // q = 2 s + {0: denominator, 1: numerator}
    if (q < 2 * S && (FIRST || (q & 1)))
      unsafeAtomicAdd(&sums[n * 2 * S + q], wsum[0][q] + wsum[1][q] + wsum[2][q] + wsum[3][q]);
  }
}

// ---- every pixel measured, 256^2: the SECOND sweep and the gradient pass in
// one launch.  With no unmeasured pixels the far-plane gradient of mode s is
// alpha_s x (F_s x poisson factor) -- linear in the step length -- so pass 1 of
// the inverse can be written BEFORE alpha_s of the second sweep is known and
// the factor applied by pass 2 (tike_ifft2_pass2_gradients_scaled).  The
// structure is fwd_grad_ifft2_pass1_kernel's two sweeps: sweep A re-forms F_s
// of every mode for the intensity; sweep B re-reads the rows, newest first,
// re-forms F_s -- whose |F_s|^2 gives the mode's numerator of the second sweep
// at the alpha of the first (a first version held |F_s|^2 of all modes across
// sweep A for them: 256 VGPRs + scratch, 2.3 ms; this one 2.0) -- applies the
// factor and runs the inverse's pass 1.  Replaces
// poisson_colpass_kernel<.., false> + tike_grad_ifft2_pass1 (the factor table
// written and read, the hand-off read once more from HBM).
template <class DT>
__global__ __launch_bounds__(256, 3) void poisson_sweep2_grad_ifft2_pass1_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, const float* __restrict__ alpha,
    float* __restrict__ sums, cf* __restrict__ work, long nscan, int S, float fwd_scale,
    float unmeasured_scaling, const cf* __restrict__ twtab) {
  constexpr int N = 256;
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
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
    // ---- sweep A: the intensity of rows k1 + 16 k2 (F_s discarded)
    float I[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) I[k2] = 0.f;
    for (int s = 0; s < S; ++s) {
      const cf* __restrict__ src = colin + (n * S + s) * (long)N * N + k1 * N;  // uniform
      cf u[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) u[r] = *tk_at_pinned(src + (16 * r) * N, t * 8u);
      Dft<16, false>::run(u);
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) I[k2] += norm2(u[k2]) * s2;
    }
    DT raw[16];
    unsigned bits;
    tk_request_data16(data, mask, n, k1, t, raw, bits);
    // xi = 1 - d / (I + eps); the gradient factor is -xi (x the forward scale).
    // (the counts are not kept: d = (1 - xi)(I + eps) where sweep B needs them;
    // an unmeasured pixel -- its count may be NaN: selected, never used -- has
    // xi = 0 here: no term in the sums, factor 0, what
    // unmeasured_pixels_scaling = 1 asks for)
    float xi[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2)
      xi[k2] = ((bits >> k2) & 1u) ? 1.0f - (float)raw[k2] / (I[k2] + 1e-9f) : 0.f;
    // ---- sweep B: modes S - 1 .. 0.  F_s re-formed: |F_s|^2 gives the mode's
    // numerator of the second sweep (exitwave.py:160-172, one atomic per wave),
    // F_s x factor goes through the inverse's pass 1 without its step length
    for (int s = S - 1; s >= 0; --s) {
      const cf* __restrict__ src = colin + (n * S + s) * (long)N * N + k1 * N;  // uniform
      cf u[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) u[r] = tk_ld_stream(tk_at_pinned(src + (16 * r) * N, t * 8u));
      Dft<16, false>::run(u);
      const float al = alpha[n * S + s];  // uniform
      float num = 0.f;
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) {
        const float av = norm2(u[k2]) * s2;
        const float xam1 = xi[k2] * al - 1.0f;
        const float dv = (1.0f - xi[k2]) * (I[k2] + 1e-9f);
        const float tn = xi[k2] * av * (1.0f + dv * xam1 / (av * xam1 * xam1 + I[k2] - av));
        num += xi[k2] != 0.f ? tn : 0.f;  // (0 x NaN of a dark unmeasured pixel)
        u[k2] = u[k2] * (-xi[k2] * fwd_scale);
      }
      num = tk_wave_sum(num);
      if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(&sums[n * 2 * S + 2 * s + 1], num);
      Dft<16, true>::run(u);
#pragma unroll
      for (int ya = 1; ya < 16; ++ya) u[ya] = mul_tw<true>(u[ya], twtab[N + k1 * ya]);
      cf* mid = work + (n * S + s) * (long)N * N;
      fft2_rows_from_columns<N, true, true>(lds, tw, line, j, u, mid + (long)(16 * k1) * N);
    }
  }
}

// alpha <- (1 - w) alpha + w numerator / denominator per (position, mode); the
// numerator is cleared for the next sweep.  first: alpha = start on entry.
__global__ __launch_bounds__(256) void poisson_alpha_kernel(float* __restrict__ sums,
                                                            float* __restrict__ alpha, long ntile,
                                                            float start, float w, int first) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < ntile; i += gridDim.x * 256L) {
    const float prev = first ? start : alpha[i];
    alpha[i] = prev * (1.0f - w) + (sums[2 * i + 1] / sums[2 * i]) * w;
    sums[2 * i + 1] = 0.f;
  }
}

extern "C" int tike_poisson_steps_handoff(const void* scratch, const void* data, int data_u16,
                                          const unsigned char* measured, float* gscale,
                                          float* costs, float* steps, float* sums, int nscan,
                                          int S, int det, float scale, float unmeasured_scaling,
                                          long num_measured, float step_start, float weight,
                                          void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && num_measured > 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(scratch && data && gscale && steps && sums);
  if (!((det == 256 && S <= 8) || (det == 512 && S <= 4))) return TK_ERR_UNSUPPORTED;
  const long ntile = (long)nscan * S;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * 2 * (size_t)ntile, stream);
  if (e == hipSuccess && costs) e = hipMemsetAsync(costs, 0, sizeof(float) * (size_t)nscan, stream);
  if (e != hipSuccess) return (int)e;
  const long nitem = (long)nscan * 16 * (det / 256);
  const float inv = 1.0f / (float)num_measured;
  const dim3 grid(tk_grid(nitem, 32)), block(256);
  const dim3 agrid(tk_grid((ntile + 255) / 256, 4));
#define TK_PC(N, DT, FIRST)                                                                     \
  hipLaunchKernelGGL((poisson_colpass_kernel<N, DT, FIRST>), grid, block, 0, stream,               \
                     (const cf*)scratch, (const DT*)data, measured, gscale, costs, steps,          \
                     step_start, sums, nitem, S, scale, unmeasured_scaling, inv)
#define TK_PC_N(FIRST)                        \
  do {                                        \
    if (det == 256 && data_u16)               \
      TK_PC(256, unsigned short, FIRST);      \
    else if (det == 256)                      \
      TK_PC(256, float, FIRST);               \
    else if (data_u16)                        \
      TK_PC(512, unsigned short, FIRST);      \
    else                                      \
      TK_PC(512, float, FIRST);               \
  } while (0)
  TK_PC_N(true);
  hipLaunchKernelGGL(poisson_alpha_kernel, agrid, dim3(256), 0, stream, sums, steps, ntile,
                     step_start, weight, 1);
  TK_PC_N(false);
  hipLaunchKernelGGL(poisson_alpha_kernel, agrid, dim3(256), 0, stream, sums, steps, ntile,
                     step_start, weight, 0);
#undef TK_PC_N
#undef TK_PC
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// Every pixel measured, det = 256: the step lengths AND pass 1 of the inverse
// of F_s x factor (WITHOUT the step lengths: tike_ifft2_pass2_gradients_scaled
// applies `steps`) -- sweep 1, alpha, sweep 2 + gradient pass, alpha.
extern "C" int tike_poisson_steps_grad_ifft2_pass1(const void* scratch, const void* data,
                                                   int data_u16, const unsigned char* measured,
                                                   float* costs, float* steps, float* sums,
                                                   void* work, int nscan, int S, int det,
                                                   float scale, float unmeasured_scaling,
                                                   long num_measured, float step_start,
                                                   float weight, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && num_measured > 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(scratch && data && steps && sums && work && work != scratch);
  // (unmeasured pixels keep F x (unmeasured_scaling - 1), which no step length
  // multiplies: linear in the steps only when that is zero)
  if (det != 256 || S > 8 || (measured != nullptr && unmeasured_scaling != 1.0f))
    return TK_ERR_UNSUPPORTED;
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  const long ntile = (long)nscan * S;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * 2 * (size_t)ntile, stream);
  if (e == hipSuccess && costs) e = hipMemsetAsync(costs, 0, sizeof(float) * (size_t)nscan, stream);
  if (e != hipSuccess) return (int)e;
  const long nitem = (long)nscan * 16;
  const float inv = 1.0f / (float)num_measured;
  const dim3 grid(tk_grid(nitem, 32)), block(256);
  const dim3 agrid(tk_grid((ntile + 255) / 256, 4));
  if (S >= TK_FG_RESIDENT_MIN_MODES) {
    // F of all modes in registers (fwd_grad_ifft2_pass1_resident_kernel): each
    // sweep reads the hand-off once
    TkCostSink sink;
    int rc = tk_cost_sink(costs, nscan, 64, stream, &sink);
    if (rc) return rc;
    const TkCostSink none = {nullptr, nullptr, 0};
    const dim3 rgrid(tk_grid(nitem, 1)), rblock(512);
#define TK_PR_K(MH, DT, ST, SINK, AL, MK_)                                                    \
  hipLaunchKernelGGL((fwd_grad_ifft2_pass1_resident_kernel<MH, 1, DT, ST, MK_>), rgrid, rblock, \
                     0, stream, (const cf*)scratch, (const DT*)data, measured, SINK,          \
                     (cf*)work, (long)nscan, S, scale, unmeasured_scaling, inv, tw, AL,       \
                     step_start, sums)
#define TK_PR(MH, DT, ST, SINK, AL)        \
  do {                                     \
    if (measured != nullptr)               \
      TK_PR_K(MH, DT, ST, SINK, AL, true); \
    else                                   \
      TK_PR_K(MH, DT, ST, SINK, AL, false);\
  } while (0)
#define TK_PR_S(ST, SINK, AL)                      \
  do {                                             \
    if (S == 6 && data_u16)                        \
      TK_PR(3, unsigned short, ST, SINK, AL);      \
    else if (S == 6)                               \
      TK_PR(3, float, ST, SINK, AL);               \
    else if (data_u16)                             \
      TK_PR(4, unsigned short, ST, SINK, AL);      \
    else                                           \
      TK_PR(4, float, ST, SINK, AL);               \
  } while (0)
    TK_PR_S(1, sink, (const float*)nullptr);
    hipLaunchKernelGGL(poisson_alpha_kernel, agrid, dim3(256), 0, stream, sums, steps, ntile,
                       step_start, weight, 1);
    TK_PR_S(2, none, (const float*)steps);
    hipLaunchKernelGGL(poisson_alpha_kernel, agrid, dim3(256), 0, stream, sums, steps, ntile,
                       step_start, weight, 0);
#undef TK_PR_S
#undef TK_PR
#undef TK_PR_K
    TK_LAUNCH_CHECK();
    return tk_cost_finish(sink, nscan, stream);
  }
  if (data_u16)
    hipLaunchKernelGGL((poisson_colpass_kernel<256, unsigned short, true>), grid, block, 0, stream,
                       (const cf*)scratch, (const unsigned short*)data, measured,
                       (float*)nullptr, costs, steps, step_start, sums, nitem, S, scale,
                       unmeasured_scaling, inv);
  else
    hipLaunchKernelGGL((poisson_colpass_kernel<256, float, true>), grid, block, 0, stream,
                       (const cf*)scratch, (const float*)data, measured, (float*)nullptr, costs,
                       steps, step_start, sums, nitem, S, scale, unmeasured_scaling, inv);
  hipLaunchKernelGGL(poisson_alpha_kernel, agrid, dim3(256), 0, stream, sums, steps, ntile,
                     step_start, weight, 1);
  const dim3 ggrid(tk_grid(nitem, 8));
  if (data_u16)
    hipLaunchKernelGGL((poisson_sweep2_grad_ifft2_pass1_kernel<unsigned short>), ggrid, block, 0,
                       stream, (const cf*)scratch, (const unsigned short*)data, measured, steps,
                       sums, (cf*)work, (long)nscan, S, scale, unmeasured_scaling, tw);
  else
    hipLaunchKernelGGL((poisson_sweep2_grad_ifft2_pass1_kernel<float>), ggrid, block, 0, stream,
                       (const cf*)scratch, (const float*)data, measured, steps, sums, (cf*)work,
                       (long)nscan, S, scale, unmeasured_scaling, tw);
  hipLaunchKernelGGL(poisson_alpha_kernel, agrid, dim3(256), 0, stream, sums, steps, ntile,
                     step_start, weight, 0);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_poisson_steps(const void* farplane, const float* intensity,
                                  const float* data, const unsigned char* measured,
                                  float* steps, int nscan, int S, int det, float step_start,
                                  float weight, int dominant_mode, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && det >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(intensity && data && steps && (dominant_mode || farplane));
  const long npix = (long)det * det;
  if (dominant_mode)
    hipLaunchKernelGGL((poisson_steps_kernel<true>), dim3(nscan), dim3(256), 0, stream,
                       (const cf*)farplane, intensity, data, measured, steps, S, npix,
                       step_start, weight);
  else if (S <= 8 && npix % 2 == 0)
    hipLaunchKernelGGL((poisson_steps_allmodes_kernel<8, 2>), dim3(nscan), dim3(256), 0, stream,
                       (const cf*)farplane, intensity, data, measured, steps, S, npix,
                       step_start, weight);
  else
    hipLaunchKernelGGL((poisson_steps_kernel<false>), dim3((unsigned)nscan * S), dim3(256), 0,
                       stream, (const cf*)farplane, intensity, data, measured, steps, S, npix,
                       step_start, weight);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// farplane[n][s][p] *= mode_scale[n][s] on measured pixels (the generic-size
// poisson path applies it after tike_farplane_gradient).
__global__ __launch_bounds__(256) void scale_modes_kernel(cf* __restrict__ farplane,
                                                          const float* __restrict__ mode_scale,
                                                          const unsigned char* __restrict__ mask,
                                                          long npix) {
  const long tile = blockIdx.y;
  const float ms = mode_scale[tile];
  cf* __restrict__ F = farplane + tile * npix;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix;
       p += (long)gridDim.x * blockDim.x)
    if (!mask || mask[p]) F[p] = F[p] * ms;
}

extern "C" int tike_scale_modes(void* farplane, const float* mode_scale,
                                const unsigned char* measured, long ntile, int det,
                                void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(ntile >= 0 && det >= 1);
  if (ntile == 0) return TK_OK;
  TK_CHECK_ARG(farplane && mode_scale);
  const long npix = (long)det * det;
  const unsigned gx = (unsigned)((npix + 1023) / 1024);
  TK_GRID_Y_LIMIT(ymax);  // tiles in gridDim.y, in slices of at most the limit
  for (long lo = 0; lo < ntile; lo += ymax)
    hipLaunchKernelGGL(scale_modes_kernel,
                       dim3(gx, (unsigned)(ntile - lo < ymax ? ntile - lo : ymax)), dim3(256), 0,
                       stream, (cf*)farplane + lo * npix, mode_scale + lo, measured, npix);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
