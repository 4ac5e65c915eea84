// fwd_grad_ifft2_pass1_resident_kernel: column pass + gradient factor + inverse
// pass 1 at 256^2 with the column-pass values of all modes in registers.
// A template in a header because two units instantiate it: ptycho.hip
// with STEPS = 0, poisson.hip with STEPS = 1, 2 (the per-mode step lengths).
#pragma once
#include "fft_engine2.h"
#include "internal.h"
#include "ptycho_shared.h"

#if defined(__HIPCC__)
// ---- the same with the column-pass values RESIDENT IN REGISTERS (256^2)
// The kernel above streams the hand-off twice, and its second sweep misses L2
// (96 work items x 256 KiB per XCD).  Here a 512-thread workgroup -- one per
// CU, 2 waves/SIMD, the whole register file -- owns a work item (position,
// k1): half h of the workgroup holds F of modes [h*MH, h*MH + MH) of its
// column, 32 registers per mode; the halves exchange their partial
// intensities through LDS, form the same g, and each sends its modes through
// the inverse's pass 1 in its own LDS transpose region.  The hand-off is read
// ONCE.  With a single workgroup per CU nothing else hides the memory
// latency, so the loop is rotated: as soon as mode m of this work item has
// left its registers, the rows of mode m of the NEXT work item are requested
// into them -- a full work item (256 KiB per CU) is always in flight.
template <int N, bool INV, class Tw>
__device__ __forceinline__ void fft2_rows_from_columns_half(cf* __restrict__ lds, const Tw& tw,
                                                            int t, int line, int j, cf (&a)[16],
                                                            cf* __restrict__ rows, bool store) {
  using G2 = Fft2Geom<N>;
#pragma unroll
  for (int ya = 0; ya < 16; ++ya) lds[ya * G2::LS + tk_pad16(t)] = a[ya];
  __syncthreads();
  cf v[16];
  cf* lbase = lds + line * G2::LS;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = lbase[tk_pad16(j + i * G2::T)];
  FftStageWave<N, INV, 0>::run(v, lbase, j, tw);
  if (store) {
    const unsigned lo = (unsigned)(line * N + j) * 8u;  // `rows` is uniform
#pragma unroll
    for (int i = 0; i < 16; ++i) tk_st_stream(tk_at(rows + i * G2::T, lo), v[i]);
  }
  __syncthreads();
}

// STEPS (poisson model, every pixel measured; see
// poisson_sweep2_grad_ifft2_pass1_kernel): with F of all modes in registers the
// sweeps of the per-mode step lengths (exitwave.py:122-184) cost no re-read --
//   1: the FIRST sweep alone: denominators and numerators at alpha = start, the
//      costs; nothing is transformed back or written;
//   2: the SECOND sweep's numerators at alpha[n][s], then the gradient pass as
//      usual (pass 1 of the inverse WITHOUT the step length).
// sums (nscan, S, 2) = { denominator, numerator }, one atomic per wave.
// MK (STEPS only): a mask may be given; without it the selects on `measured`
// and the mask loads are compiled out (2.87 against 3.04 ms per 1000 positions
// for both sweeps).
template <int MH, int MODEL, class DT, int STEPS = 0, bool MK = true>
__global__ __launch_bounds__(512, 1) void fwd_grad_ifft2_pass1_resident_kernel(
    const cf* __restrict__ colin, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, const TkCostSink costs, cf* __restrict__ work,
    long nscan, int S, float fwd_scale, float unmeasured_scaling, float inv_nmeasured,
    const cf* __restrict__ twtab, const float* __restrict__ alpha = nullptr, float start = 0.f,
    float* __restrict__ sums = nullptr) {
  constexpr int N = 256;
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[2 * G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  // (STEPS: the counts of a work item wait in LDS, a private slot per thread
  // and pixel, while the modes go through their registers)
  __shared__ float dvp[STEPS != 0 ? 16 * 512 : 1];
  __shared__ float ivp[STEPS == 2 ? 16 * 512 : 1];  // ... and, beside the inverse, the intensity
  cf* twl = lds + 2 * G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int h = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const int t = threadIdx.x & 255;
  cf* const mylds = lds + h * G2::LDS_ELEMS;
  int line = t / G2::T, j = t % G2::T;
  asm volatile("" : "+v"(line), "+v"(j));
  const FftTwLds<N> tw{twl, j};
  const int m0 = h * MH;
  const float s2 = fwd_scale * fwd_scale;
  const long total = nscan * 16;
  cf F[MH][16];
  auto request = [&](long v, int m) {  // rows 16 r + k1 of mode m0 + m into F[m]
    const int k1 = (int)(v & 15);
    const long n = nscan - 1 - (v >> 4);
    if (m0 + m < S) {
      const cf* __restrict__ src = colin + (n * S + m0 + m) * (long)N * N + k1 * N;  // uniform
#pragma unroll
      for (int r = 0; r < 16; ++r)
        F[m][r] = tk_ld_stream(tk_at_pinned(src + (16 * r) * N, t * 8u));
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) F[m][r] = cf{0.f, 0.f};
    }
  };
  long v = blockIdx.x;
  if (v < total) {
#pragma unroll
    for (int m = 0; m < MH; ++m) request(v, m);
  }
  for (; v < total; v += gridDim.x) {
    const int k1 = (int)(v & 15);
    const long n = nscan - 1 - (v >> 4);  // descending: see fwd_gradient_scale_kernel
    DT raw[16];
    unsigned bits;
    float I[16];
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) I[k2] = 0.f;
#pragma unroll
    for (int m = 0; m < MH; ++m) {
      // the counts: requested behind the last hand-off rows, used after the
      // last butterfly and the exchange
      if (m == MH - 1)
        tk_request_data16(data, !MK ? (const unsigned char*)nullptr : mask, n, k1, t, raw, bits);
      Dft<16, false>::run(F[m]);
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) I[k2] += norm2(F[m][k2]) * s2;
    }
    {
      float* const myI = reinterpret_cast<float*>(mylds);
      const float* const otherI =
          reinterpret_cast<const float*>(lds + (1 - h) * G2::LDS_ELEMS);
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) myI[k2 * N + t] = I[k2];
      __syncthreads();
      // both halves add in the same order: they must form the SAME factor
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) {
        const float o = otherI[k2 * N + t];
        I[k2] = h == 0 ? I[k2] + o : o + I[k2];
      }
      __syncthreads();
    }
    float cost;
    if (STEPS == 0) {
      cost = tk_gradient_factor16<MODEL>(I, raw, bits, unmeasured_scaling, fwd_scale);
    } else {
      // (I stays the intensity: the sweeps need it next to every mode; the
      // factor -xi x scale is formed per mode below)
      cost = 0.f;
#pragma unroll
      for (int k2 = 0; k2 < 16; ++k2) {
        // an unmeasured pixel (its count may be NaN: selected, never used in
        // arithmetic) is parked as -1: no term in any sum, factor 0
        // (unmeasured_pixels_scaling = 1, the only value this path serves)
        const bool meas = !MK || ((bits >> k2) & 1u);
        const float dv = meas ? (float)raw[k2] : -1.0f;
        // (the costs come out of the FIRST sweep's launch: sixteen logarithms
        // beside 128 registers of F are what the second one spilled for)
        if (STEPS == 1) cost += meas ? I[k2] - dv * logf(I[k2] + 1e-9f) : 0.f;
        dvp[k2 * 512 + threadIdx.x] = dv;
        if (STEPS == 2) ivp[k2 * 512 + threadIdx.x] = I[k2];
      }
    }
    if (STEPS != 2 && costs.costs && h == 0) {
      cost = tk_wave_sum(cost);
      if ((threadIdx.x & 63) == 0)
        tk_cost_add(costs, n, k1 * 4 + (int)(threadIdx.x >> 6), cost * inv_nmeasured);
    }
    const long vn = v + gridDim.x;
#pragma unroll
    for (int m = 0; m < MH; ++m) {
      if (STEPS != 0) {
        // the sweep's sums of this mode over this thread's 16 pixels
        const float al = (STEPS == 1 || m0 + m >= S) ? start : alpha[n * S + m0 + m];  // uniform
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
          // (in quarters: all sixteen pairs of parked values in flight at once
          // do not fit next to the other modes)
          if (STEPS == 2 && (k2 & 3) == 0) asm volatile("" ::: "memory");
          const float dv = dvp[k2 * 512 + threadIdx.x];
          const float ie = STEPS == 2 ? ivp[k2 * 512 + threadIdx.x] : I[k2];
          // (v_rcp_f32, 1 ulp: an IEEE division is a dozen instructions and
          // five temporaries, twice per pixel and mode, next to 128 registers
          // of F)
          const bool meas = !MK || dv >= 0.f;
          const float xi = 1.0f - dv * __builtin_amdgcn_rcpf(ie + 1e-9f);
          // (|F|^2 formed AGAIN here: kept from the intensity loop -- the same
          // expression -- sixteen values per mode lived across the exchange,
          // in scratch: 108-140 bytes per lane until round 6)
          if (STEPS == 2) asm volatile("" : "+v"(F[m][k2].x), "+v"(F[m][k2].y));
          const float av = norm2(F[m][k2]) * s2;
          const float xam1 = xi * al - 1.0f;
          const float tn =
              xi * av * (1.0f + dv * xam1 * __builtin_amdgcn_rcpf(av * xam1 * xam1 + ie - av));
          num += meas ? tn : 0.f;
          if (STEPS == 1) den += meas ? xi * xi * av : 0.f;
          if (STEPS == 2) F[m][k2] = F[m][k2] * (meas ? -xi * fwd_scale : 0.f);
        }
        if (m0 + m < S) {  // uniform
          num = tk_wave_sum(num);
          if (STEPS == 1) den = tk_wave_sum(den);
          if ((threadIdx.x & 63) == 0) {
            unsafeAtomicAdd(&sums[(n * S + m0 + m) * 2 + 1], num);
            if (STEPS == 1) unsafeAtomicAdd(&sums[(n * S + m0 + m) * 2], den);
          }
        }
      } else {
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) F[m][k2] = F[m][k2] * I[k2];
      }
      if (STEPS != 1) {
        Dft<16, true>::run(F[m]);
#pragma unroll
        for (int ya = 1; ya < 16; ++ya)
          F[m][ya] = mul_tw<true>(F[m][ya], twtab[N + k1 * ya]);
        cf* mid = work + (n * S + m0 + m) * (long)N * N;
        fft2_rows_from_columns_half<N, true>(mylds, tw, t, line, j, F[m],
                                             mid + (long)(16 * k1) * N, m0 + m < S);
      }
      if (vn < total) request(vn, m);
    }
  }
}

#endif
