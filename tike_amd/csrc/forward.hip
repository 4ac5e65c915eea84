// The forward operator, fused, for gfx950: bilinear patch gather * probe ->
// zero pad -> FFT2 (reference ptycho.py:114-129 = convolution.py:58-101 +
// propagation.py:43-57), no patch array, no memset, no separate multiply pass.
//   tike_ptycho_fwd      the far-plane waves;
//   tike_ptycho_fwd_intensity{,_only}, tike_ptycho_fwd_gradient_scale
//                        position-major, the intensity (ptycho.py:18-23) and
//                        the gradient factor accumulated in registers;
//   tike_fwd_pass1       pass 1 alone: the column-pass input ("hand-off") that
//                        the other stages consume in place of a far plane.
// launch_fwd128_lds and tk_fwd_pass1 are shared with them (internal.h).
#include "fft_engine2.h"
#include "internal.h"
#include "tike_amd.h"

// --------------------------------------------------------------- forward
// The small-size fallbacks (ptycho_fwd_kernel, ptycho_fwd_v2_kernel):
// one workgroup owns one (position, mode) tile and runs the row pass and the
// column pass back to back; the intermediate lives in the tile's own output
// (L2 / Infinity Cache resident between the passes).
template <int N>
__global__ __launch_bounds__(FftPlan<N>::NT, FftPlan<N>::MINW) void ptycho_fwd_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const TkProbe probe,
    cf* __restrict__ farplane, long ntile, int S, int pw, int H, int W, float scale,
    const cf* __restrict__ twtab) {
  using G = FftGeom<N>;
  __shared__ cf lds[G::LDS_ELEMS];
  FftTw<N> tw;
  const int pad = (N - pw) / 2;
  const int end = pad + pw;
  const long total = (long)H * W;
  for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const long n = tile / S;
    const int s = (int)(tile % S);
    const TkCorner c = tk_corner(scan, n);
    cf* __restrict__ dst = farplane + tile * (long)N * N;
    const FftLane<N, false> row = fft_lane<N, false>();
    tw.init(twtab, row.j);
    for (int g = 0; g < N; g += G::L) {
      if (g + G::L <= pad || g >= end) {
        // rows entirely inside the zero padding transform to zero
        for (int i = threadIdx.x; i < G::L * N; i += G::NT) dst[g * N + i] = mk(0.f, 0.f);
        continue;
      }
      // Stage the L input rows (patch * probe, zero padded) into the LDS line
      // buffers with row-contiguous, fully coalesced loads: thread -> column,
      // loop over rows, re-using the lower taps of one row as the upper taps
      // of the next (2 new object loads per pixel instead of 4).
      for (int x0 = 0; x0 < N; x0 += G::NT) {
        const int dx = x0 + threadIdx.x;
        const int px = dx - pad;
        const int x = c.sx + px;
        const bool col_ok = dx < N && px >= 0 && px < pw && x >= 0 && x < W;
        cf t0 = mk(0.f, 0.f), t1 = mk(0.f, 0.f);  // taps of the current object row
        bool have = false;
#pragma unroll 4
        for (int line = 0; line < G::L; ++line) {
          const int py = g + line - pad;
          const int y = c.sy + py;
          cf o = mk(0.f, 0.f);
          if (col_ok && py >= 0 && py < pw && y >= 0 && y < H) {
            const long ii = (long)y * W + x;
            if (!have) {
              t0 = psi[ii];
              t1 = (ii + 1 < total) ? psi[ii + 1] : mk(0.f, 0.f);
            }
            cf b0 = mk(0.f, 0.f), b1 = mk(0.f, 0.f);
            // lower taps are loaded whenever they lie inside the allocation
            // (they become the next row's upper taps); a zero weight makes
            // their contribution exactly zero, as in the reference kernel.
            if (ii + W < total) {
              b0 = psi[ii + W];
              if (ii + W + 1 < total) b1 = psi[ii + W + 1];
            }
            cf v = mk(t0.x * c.w00, t0.y * c.w00);
            v.x += t1.x * c.w01;
            v.y += t1.y * c.w01;
            v.x += b0.x * c.w10;
            v.y += b0.y * c.w10;
            v.x += b1.x * c.w11;
            v.y += b1.y * c.w11;
            o = v * probe.at(n, s, (long)py * pw + px);
            t0 = b0;
            t1 = b1;
            have = true;
          } else {
            have = false;
          }
          if (dx < N) lds[line * G::LS + tk_pad16(dx)] = o;
        }
      }
      __syncthreads();
      fft_lines<N, false, false>(
          lds, row, tw,
          [&](int line, int e) { return lds[line * G::LS + tk_pad16(e)]; },
          [&](int line, int e, cf v) { dst[(g + line) * N + e] = v; }, /*sync_after_load=*/true);
    }
    __syncthreads();
    const FftLane<N, true> col = fft_lane<N, true>();
    tw.init(twtab, col.j);
    for (int g = 0; g < N; g += G::L) {
      fft_lines<N, false, true>(
          lds, col, tw, [&](int line, int e) { return dst[e * N + g + line]; },
          [&](int line, int e, cf v) { dst[e * N + g + line] = v * scale; });
    }
    __syncthreads();
  }
}

// v2 structure (fft_engine2.h): N threads per workgroup, thread = column.
template <int N>
__global__ __launch_bounds__(N, TK_V2_MINW(N)) void ptycho_fwd_v2_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const TkProbe probe,
    cf* __restrict__ farplane, long ntile, int S, int pw, int H, int W, float scale,
    const cf* __restrict__ twtab) {
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int pad = (N - pw) / 2;
  const long total = (long)H * W;
  for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const long n = tile / S;
    const int s = (int)(tile % S);
    const TkCorner c = tk_corner(scan, n);
    cf* __restrict__ dst = farplane + tile * (long)N * N;
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    const int t = threadIdx.x;
    const int px = t - pad;
    const int x = c.sx + px;
    const bool col_ok = px >= 0 && px < pw && x >= 0 && x < W;
    // clamped coordinates: every load is unconditional and in bounds, the
    // padding / out-of-image pixels are zeroed by a select afterwards
    const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
    const int xc = c.sx + pxc < 0 ? 0 : (c.sx + pxc >= W ? W - 1 : c.sx + pxc);
    // Fast path (every position that passes check_allowed_positions): all four
    // taps of every patch pixel lie inside the image, so rows are addressed as
    // uniform row offset + per-thread column with no clamping, and the probe
    // weights of this (position, mode) are hoisted into scalars.
    const bool interior = c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W;
    const long PP = (long)pw * pw;
    const cf* __restrict__ Pn = probe.probe + n * probe.pos_stride + s * PP;
    float w0 = 1.0f;
    int nE = 0;
    if (probe.weights != nullptr) {
      w0 = probe.weights[n * (long)(probe.C + 1) * probe.S + s];
      if (probe.eigen != nullptr && s < probe.Sm) nE = probe.C;
    }
    for (int r = 0; r < G2::RB; ++r) {
      // stage the 16 rows {r + RB*l} of patch * probe (zero padded) into LDS
      if (interior) {
#pragma unroll 8
        for (int l = 0; l < 16; ++l) {
          const int py = r + G2::RB * l - pad;           // uniform
          const bool row_ok = py >= 0 && py < pw;        // uniform
          const int pyc = py < 0 ? 0 : (py >= pw ? pw - 1 : py);
          const cf* __restrict__ q = psi + (long)(c.sy + pyc) * W + c.sx + pxc;
          const cf a = q[0], b = q[1], d = q[W], e = q[W + 1];
          const long pi = (long)pyc * pw + pxc;
          cf pr = Pn[pi] * w0;
          for (int k = 0; k < nE; ++k) {
            const cf ev = probe.eigen[((long)k * probe.Sm + s) * PP + pi];
            const float wk =
                probe.weights[n * (long)(probe.C + 1) * probe.S + (k + 1) * probe.S + s];
            pr.x += wk * ev.x;
            pr.y += wk * ev.y;
          }
          cf o = mk(a.x * c.w00, a.y * c.w00);
          o.x += b.x * c.w01;
          o.y += b.y * c.w01;
          o.x += d.x * c.w10;
          o.y += d.y * c.w10;
          o.x += e.x * c.w11;
          o.y += e.y * c.w11;
          o = o * pr;
          lds[l * G2::LS + tk_pad16(t)] = (row_ok && col_ok) ? o : mk(0.f, 0.f);
        }
      } else {
#pragma unroll 4
        for (int l = 0; l < 16; ++l) {
          const int py = r + G2::RB * l - pad;
          const int y = c.sy + py;
          const bool ok = col_ok && py >= 0 && py < pw && y >= 0 && y < H;
          const int pyc = py < 0 ? 0 : (py >= pw ? pw - 1 : py);
          const int yc = c.sy + pyc < 0 ? 0 : (c.sy + pyc >= H ? H - 1 : c.sy + pyc);
          const cf o = tk_gather(psi, (long)yc * W + xc, W, total, c) *
                       probe.at(n, s, (long)pyc * pw + pxc);
          lds[l * G2::LS + tk_pad16(t)] = ok ? o : mk(0.f, 0.f);
        }
      }
      __syncthreads();
      fft2_pass1<N, false>(lds, twtab, tw, line, j, r,
                           [&](int y, int e, auto) { return lds[line * G2::LS + tk_pad16(e)]; }, dst);
    }
    __syncthreads();
    for (int k1 = 0; k1 < 16; ++k1)
      fft2_pass2<N, false>(dst, k1, [&](int ky, int tt, cf v) { dst[ky * N + tt] = v * scale; });
    __syncthreads();
  }
}

// Position-major forward: one workgroup owns ALL S modes of a position, so the
// bilinear patch is gathered once per 16-row group (registers) and re-used by
// every mode, and the intensity sum_s |F_s|^2 accumulates in registers during
// pass 2 -- the far-plane is never re-read to form it (ptycho.py:18-23,
// lstsq.py:444-447).
#ifndef TK_POS_WAVES
#define TK_POS_WAVES 2
#endif
// Optional epilogue of the intensity-only forward kernel: the far-plane
// gradient factor and the per-pattern cost (objective.py:11-124,
// lstsq.py:444-502) straight from the intensity in registers.
struct TkGradScale {
  const float* data;           // (nscan, det, det) or nullptr: epilogue off
  const unsigned char* mask;   // (det, det) or nullptr (all measured)
  float* gscale;               // (nscan, det, det)
  float* costs;                // (nscan) or nullptr
  int model;                   // 0 gaussian, 1 poisson
  float unmeasured_scaling;
  float inv_nmeasured;
};

// STORE = false: the far-plane waves are formed in registers for the intensity
// only; `farplane` then keeps the INPUT of the column pass (rows 16r + k1 of
// fft2_pass1), which tike_grad_ifft2_crop consumes.
template <int N, bool STORE = true>
__global__ __launch_bounds__(N, (N <= 256 ? TK_POS_WAVES : 2)) void ptycho_fwd_pos_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const TkProbe probe,
    cf* __restrict__ farplane, float* __restrict__ intensity, int nscan, int S, int pw, int H,
    int W, float scale, const cf* __restrict__ twtab, const TkGradScale gsc,
    cf* __restrict__ patches) {
  using G2 = Fft2Geom<N>;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int pad = (N - pw) / 2;
  const long total = (long)H * W;
  const long PP = (long)pw * pw;
  for (long n = blockIdx.x; n < nscan; n += gridDim.x) {
    const TkCorner c = tk_corner(scan, n);
    cf* __restrict__ dst0 = farplane + n * S * (long)N * N;
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    const int t = threadIdx.x;
    for (int r = 0; r < G2::RB; ++r) {
      // Patch values of row y = r + RB*line in the FFT register layout
      // (element e = j + i*T), gathered once and shared by all S modes: the
      // row FFT consumes them straight from registers (no LDS staging pass).
      const int py = r + G2::RB * line - pad;
      const int y = c.sy + py;
      const bool row_ok = py >= 0 && py < pw && y >= 0 && y < H;
      const int pyc = py < 0 ? 0 : (py >= pw ? pw - 1 : py);
      const int yc = c.sy + pyc < 0 ? 0 : (c.sy + pyc >= H ? H - 1 : c.sy + pyc);
      cf pv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int px = j + i * G2::T - pad;
        const int x = c.sx + px;
        const bool ok = row_ok && px >= 0 && px < pw && x >= 0 && x < W;
        const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
        const int xc = c.sx + pxc < 0 ? 0 : (c.sx + pxc >= W ? W - 1 : c.sx + pxc);
        const cf o = tk_gather(psi, (long)yc * W + xc, W, total, c);
        pv[i] = ok ? o : mk(0.f, 0.f);
        // bound the taps in flight (4 elements = 16 loads) and with them the
        // register footprint of this phase
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      if (patches != nullptr && py >= 0 && py < pw) {
        // the object patch O_n (Patch.fwd, lstsq.py:524-531) for the gradient
        // and step-size passes, while it is in registers
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int px = j + i * G2::T - pad;
          if (px >= 0 && px < pw) patches[n * PP + (long)py * pw + px] = pv[i];
        }
      }
      for (int s = 0; s < S; ++s) {
        // probe of this (position, mode): a base pointer and a scale, both
        // uniform -- either the shared probe times its weight or the varying
        // probe synthesised beforehand by tike_varying_probe
        const cf* __restrict__ Pn = probe.probe + n * probe.pos_stride + s * PP;
        float w0 = 1.0f;
        if (probe.weights != nullptr) {
          if (probe.unique != nullptr && s < probe.Sm)
            Pn = probe.unique + (n * probe.Sm + s) * PP;
          else
            w0 = probe.weights[n * (long)(probe.C + 1) * probe.S + s];
        }
        fft2_pass1<N, false>(
            lds, twtab, tw, line, j, r,
            [&](int, int e, auto I) {
              constexpr int i = decltype(I)::value;
              const int px = e - pad;
              const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
              return pv[i] * (Pn[pyc * pw + pxc] * w0);
            },
            dst0 + s * (long)N * N);
      }
    }
    __syncthreads();
    if constexpr (!STORE) {
      // intensity only: nothing is stored per tile, so the column pass is a
      // pure read stream -- keep the rows of the NEXT (k1, mode) in flight
      // while the current ones go through the butterfly
      cf nxt[G2::RB];
      float cost = 0.f;
#pragma unroll
      for (int r = 0; r < G2::RB; ++r) nxt[r] = dst0[(16 * r) * N + t];
      for (int k1 = 0; k1 < 16; ++k1) {
        float I[G2::RB];
#pragma unroll
        for (int k2 = 0; k2 < G2::RB; ++k2) I[k2] = 0.f;
        for (int s = 0; s < S; ++s) {
          cf u[G2::RB];
#pragma unroll
          for (int r = 0; r < G2::RB; ++r) u[r] = nxt[r];
          const int s2 = s + 1 < S ? s + 1 : 0;
          const int k2n = s + 1 < S ? k1 : (k1 + 1 < 16 ? k1 + 1 : k1);
          const cf* __restrict__ nsrc = dst0 + s2 * (long)N * N;
#pragma unroll
          for (int r = 0; r < G2::RB; ++r) nxt[r] = nsrc[(16 * r + k2n) * N + t];
          Dft<G2::RB, false>::run(u);
#pragma unroll
          for (int k2 = 0; k2 < G2::RB; ++k2) I[k2] += norm2(u[k2] * scale);
        }
        if (intensity) {
#pragma unroll
          for (int k2 = 0; k2 < G2::RB; ++k2)
            tk_st_stream(intensity + n * (long)N * N + (k1 + 16 * k2) * N + t, I[k2]);
        }
        if (gsc.data) {
          // gradient factor and cost from the intensity in registers
#pragma unroll
          for (int k2 = 0; k2 < G2::RB; ++k2) {
            const long p = (long)(k1 + 16 * k2) * N + t;
            float g = gsc.unmeasured_scaling - 1.0f;
            if (gsc.mask == nullptr || gsc.mask[p]) {
              const float dv = gsc.data[n * (long)N * N + p];
              if (gsc.model == 0) {
                const float sI = sqrtf(I[k2]), sd = sqrtf(dv);
                const float diff = sI - sd;
                cost += diff * diff;
                g = -(1.0f - sd / (sI + 1e-9f));
              } else {
                cost += I[k2] - dv * logf(I[k2] + 1e-9f);
                g = -(1.0f - dv / (I[k2] + 1e-9f));
              }
            }
            gsc.gscale[n * (long)N * N + p] = g;
          }
        }
      }
      if (gsc.data && gsc.costs) {
        // block sum through the (now idle) FFT exchange area
        float* red = reinterpret_cast<float*>(lds);
        __syncthreads();
        cost = tk_wave_sum(cost);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cost;
        __syncthreads();
        if (threadIdx.x == 0) {
          float tot = 0.f;
          for (int w = 0; w < N / 64; ++w) tot += red[w];
          gsc.costs[n] = tot * gsc.inv_nmeasured;
        }
      }
    } else
    for (int k1 = 0; k1 < 16; ++k1) {
      float I[G2::RB];
#pragma unroll
      for (int k2 = 0; k2 < G2::RB; ++k2) I[k2] = 0.f;
      for (int s = 0; s < S; ++s) {
        cf* __restrict__ dst = dst0 + s * (long)N * N;
        fft2_pass2<N, false>(dst, k1, [&](int ky, int tt, cf v) {
          const cf o = v * scale;
          if (STORE) tk_st_stream(dst + ky * N + tt, o);
          I[(ky - k1) >> 4] += norm2(o);
        });
      }
      if (intensity) {
#pragma unroll
        for (int k2 = 0; k2 < G2::RB; ++k2)
          tk_st_stream(intensity + n * (long)N * N + (k1 + 16 * k2) * N + t, I[k2]);
      }
    }
    __syncthreads();
  }
}

template <int N, bool STORE = true>
static int launch_fwd_pos(const cf* psi, const float* scan, const TkProbe& probe, cf* farplane,
                          float* intensity, int nscan, int S, int pw, int H, int W, float scale,
                          hipStream_t stream, const TkGradScale* gsc = nullptr,
                          cf* patches = nullptr) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  TkGradScale g = {};
  if (gsc) g = *gsc;
  hipLaunchKernelGGL((ptycho_fwd_pos_kernel<N, STORE>), dim3(tk_grid(nscan, 4)), dim3(N), 0,
                     stream, psi, scan, probe, farplane, intensity, nscan, S, pw, H, W, scale, tw,
                     g, patches);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

#ifndef TK_LDS128_MAX_MODES
#define TK_LDS128_MAX_MODES 8
#endif

extern "C" int tike_ptycho_fwd_intensity(const void* psi, const float* scan, const void* probe,
                                         int probe_per_scan, const void* unique_probe,
                                         const float* eigen_weights, int num_eigen,
                                         int eigen_modes, void* farplane, float* intensity,
                                         void* patches, int nscan, int S, int pw, int det, int H,
                                         int W, float scale, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  TK_CHECK_ARG(!(eigen_weights && probe_per_scan));
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(psi && scan && probe && farplane);
  TK_CHECK_ARG(!(eigen_weights && eigen_modes > 0 && !unique_probe));
  const TkProbe P = tk_make_probe(probe, probe_per_scan, nullptr, eigen_weights, num_eigen,
                                  eigen_modes, S, pw, unique_probe);
  switch (det) {
    case 128:
      // probe window = detector: the whole-tile-in-LDS kernel (no intermediate
      // in memory); a few modes only -- it re-reads nothing, but keeps the
      // patch in registers across the modes at the 128-register cap
      if (pw == 128 && intensity != nullptr && S <= TK_LDS128_MAX_MODES)
        return launch_fwd128_lds((const cf*)psi, scan, P, (cf*)farplane, intensity, nscan, S, H,
                                 W, scale, stream, (cf*)patches);
      return launch_fwd_pos<128>((const cf*)psi, scan, P, (cf*)farplane, intensity, nscan, S, pw,
                                 H, W, scale, stream, nullptr, (cf*)patches);
    case 256:
      return launch_fwd_pos<256>((const cf*)psi, scan, P, (cf*)farplane, intensity, nscan, S, pw,
                                 H, W, scale, stream, nullptr, (cf*)patches);
    case 512:
      return launch_fwd_pos<512>((const cf*)psi, scan, P, (cf*)farplane, intensity, nscan, S, pw,
                                 H, W, scale, stream, nullptr, (cf*)patches);
    default:
      return TK_ERR_UNSUPPORTED;
  }
}

// Forward model for the intensity only (det = 256): `scratch` (nscan,S,det,det)
// receives the column-pass input of every tile instead of the far-plane waves.
extern "C" int tike_ptycho_fwd_intensity_only(const void* psi, const float* scan,
                                              const void* probe, int probe_per_scan,
                                              const void* unique_probe,
                                              const float* eigen_weights, int num_eigen,
                                              int eigen_modes, void* scratch, float* intensity,
                                              int nscan, int S, int pw, int det, int H, int W,
                                              float scale, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  TK_CHECK_ARG(!(eigen_weights && probe_per_scan));
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(psi && scan && probe && scratch && intensity);
  TK_CHECK_ARG(!(eigen_weights && eigen_modes > 0 && !unique_probe));
  if (det != 256) return TK_ERR_UNSUPPORTED;
  const TkProbe P = tk_make_probe(probe, probe_per_scan, nullptr, eigen_weights, num_eigen,
                                  eigen_modes, S, pw, unique_probe);
  return launch_fwd_pos<256, false>((const cf*)psi, scan, P, (cf*)scratch, intensity, nscan, S,
                                    pw, H, W, scale, stream);
}

// tike_ptycho_fwd_intensity_only + tike_gradient_scale in one launch: the
// gradient factor and the per-pattern cost are formed from the intensity while
// it is still in registers (intensity itself is stored only if asked for).
extern "C" int tike_ptycho_fwd_gradient_scale(
    const void* psi, const float* scan, const void* probe, int probe_per_scan,
    const void* unique_probe, const float* eigen_weights, int num_eigen, int eigen_modes,
    void* scratch, float* intensity, void* patches, const float* data,
    const unsigned char* measured, float* gscale, float* costs, int nscan, int S, int pw, int det,
    int H, int W, float scale, int model, float unmeasured_scaling, long num_measured,
    void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  TK_CHECK_ARG(!(eigen_weights && probe_per_scan) && (model == 0 || model == 1) &&
               num_measured > 0);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(psi && scan && probe && scratch && data && gscale);
  TK_CHECK_ARG(!(eigen_weights && eigen_modes > 0 && !unique_probe));
  if (det != 256) return TK_ERR_UNSUPPORTED;
  const TkProbe P = tk_make_probe(probe, probe_per_scan, nullptr, eigen_weights, num_eigen,
                                  eigen_modes, S, pw, unique_probe);
  TkGradScale g;
  g.data = data;
  g.mask = measured;
  g.gscale = gscale;
  g.costs = costs;
  g.model = model;
  g.unmeasured_scaling = unmeasured_scaling;
  g.inv_nmeasured = 1.0f / (float)num_measured;
  return launch_fwd_pos<256, false>((const cf*)psi, scan, P, (cf*)scratch, intensity, nscan, S,
                                    pw, H, W, scale, stream, &g, (cf*)patches);
}

// ---- the 256^2 forward split in two launches (both far-plane free) ----------
// Pass 1 alone: bilinear gather * probe -> row transforms -> radix-16 column
// stage; `scratch` receives the column-pass input of every tile and `patches`
// the object patches.  A work item is (position, 16-row group) and covers all S
// modes (the patch of the group is gathered once and shared by the modes).
// 167 VGPRs at 256^2: three waves per SIMD hide the probe loads of a mode behind
// the other waves' butterflies and stores (an earlier version requested the
// next mode's probe values ahead of the stores instead, at 255 VGPRs and two
// waves: 13 % slower).
// FULL: probe window = detector (pw == N, no padding): every probe / patch
// access of a thread is `uniform base + one 32-bit lane offset + 8 T i` bytes.
// KEEP: plain stores of the hand-off instead of non-temporal ones -- they stay
// in the Infinity Cache for a consumer that follows within ~256 MiB (the
// forward operator's sub-batched column pass); the solver's minibatch-sized
// hand-off does not fit and keeps the non-temporal stores.
template <int N, bool FULL, bool KEEP = false>
__global__ __launch_bounds__(N, N == 512 ? 2 : 3) void fwd_pass1_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const TkProbe probe,
    cf* __restrict__ scratch, cf* __restrict__ patches, int nscan, int S, int pw, int H, int W,
    const cf* __restrict__ twtab, const int* __restrict__ skip) {
  using G2 = Fft2Geom<N>;
  constexpr unsigned EB = G2::T * sizeof(cf);  // bytes between a thread's elements
  // a speculative launch (device-side line search) whose result is not needed
  if (skip != nullptr && *skip != 0) return;
  __shared__ cf lds[G2::LDS_ELEMS + FftTwLds<N>::ELEMS];
  cf* twl = lds + G2::LDS_ELEMS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  const int pad = FULL ? 0 : (N - pw) / 2;
  const long total = (long)H * W;
  const long PP = (long)pw * pw;
  const int t = threadIdx.x;
  auto at = [](const cf* base, unsigned byte_off) -> const cf* {
    return reinterpret_cast<const cf*>(reinterpret_cast<const char*>(base) + byte_off);
  };
  // work item = (position, 16-row group): small launches (the sub-chunked
  // pipeline keeps the hand-off inside the Infinity Cache) still fill the chip
  for (long item = blockIdx.x; item < (long)nscan * G2::RB; item += gridDim.x) {
    const long n = item / G2::RB;
    const int r = (int)(item % G2::RB);
    const TkCorner c = tk_corner(scan, n);
    cf* __restrict__ dst0 = scratch + n * S * (long)N * N;
    int line = threadIdx.x / G2::T, j = threadIdx.x % G2::T;
    asm volatile("" : "+v"(line), "+v"(j));
    const FftTwLds<N> tw{twl, j};
    const float* __restrict__ wn =
        probe.weights ? probe.weights + n * (long)(probe.C + 1) * probe.S : nullptr;
    // every tap of every patch pixel inside the image (any position that
    // passes check_allowed_positions) and 32-bit byte offsets suffice
    const bool interior = FULL && c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W &&
                          total < (1L << 28);
    {
      // patch values of row y = r + RB*line in the FFT register layout
      // (element e = j + i*T), gathered once and shared by all S modes
      const int py = r + G2::RB * line - pad;
      const int pyc = py < 0 ? 0 : (py >= pw ? pw - 1 : py);
      // byte offset of this thread's first pixel inside a probe mode / patch
      const unsigned pbo = (unsigned)(pyc * pw + j) * (unsigned)sizeof(cf);
      cf pv[16];
      if (interior) {
        const unsigned g0 = (unsigned)((c.sy + py) * W + c.sx + j) * (unsigned)sizeof(cf);
        const unsigned g1 = g0 + (unsigned)W * (unsigned)sizeof(cf);
        // The two taps of a row are adjacent complex values: one 16-byte load.
        // 8 elements = 16 loads are requested together; the empty asm reads
        // all of them, so none can be sunk next to its use (which would
        // cost one L2 round trip per element).
        typedef float tk_v4f __attribute__((ext_vector_type(4)));
        auto ld4 = [](const cf* base, unsigned byte_off) {
          tk_v4f v;
          __builtin_memcpy(&v, reinterpret_cast<const char*>(base) + byte_off, sizeof(v));
          return v;
        };
#pragma unroll
        for (int h = 0; h < 16; h += 8) {
          tk_v4f u[8], l[8];  // upper row (a, b), lower row (d, e)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            u[i] = ld4(psi, g0 + EB * (h + i));
            l[i] = ld4(psi, g1 + EB * (h + i));
          }
          asm volatile(""
                       : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]),
                         "+v"(u[6]), "+v"(u[7]), "+v"(l[0]), "+v"(l[1]), "+v"(l[2]), "+v"(l[3]),
                         "+v"(l[4]), "+v"(l[5]), "+v"(l[6]), "+v"(l[7]));
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            cf o = mk(u[i].x * c.w00, u[i].y * c.w00);
            o.x += u[i].z * c.w01;
            o.y += u[i].w * c.w01;
            o.x += l[i].x * c.w10;
            o.y += l[i].y * c.w10;
            o.x += l[i].z * c.w11;
            o.y += l[i].w * c.w11;
            pv[h + i] = o;
          }
        }
      } else {
        const int y = c.sy + py;
        const bool row_ok = py >= 0 && py < pw && y >= 0 && y < H;
        const int yc = c.sy + pyc < 0 ? 0 : (c.sy + pyc >= H ? H - 1 : c.sy + pyc);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int px = j + i * G2::T - pad;
          const int x = c.sx + px;
          const bool ok = row_ok && px >= 0 && px < pw && x >= 0 && x < W;
          const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
          const int xc = c.sx + pxc < 0 ? 0 : (c.sx + pxc >= W ? W - 1 : c.sx + pxc);
          const cf o = tk_gather(psi, (long)yc * W + xc, W, total, c);
          pv[i] = ok ? o : mk(0.f, 0.f);
          __builtin_amdgcn_sched_barrier(0);  // rare path: one element in flight
        }
      }
      if (patches != nullptr && py >= 0 && py < pw) {
        cf* __restrict__ On = patches + n * PP;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int px = j + i * G2::T - pad;
          if (FULL)
            tk_st_stream(const_cast<cf*>(at(On, pbo + EB * i)), pv[i]);
          else if (px >= 0 && px < pw)
            tk_st_stream(On + (long)py * pw + px, pv[i]);
        }
      }
      // probe of (position, mode): shared probe times its weight, plus the
      // eigen probes of the first Sm modes (probe.py:272-303) -- from the
      // synthesised array when given, else on the fly
      auto load_probe = [&](int s, cf (&pn)[16]) {
        const cf* __restrict__ Pn = probe.probe + n * probe.pos_stride + s * PP;
        float w0 = 1.0f;
        int nE = 0;
        if (wn != nullptr) {
          if (probe.unique != nullptr && s < probe.Sm) {
            Pn = probe.unique + (n * probe.Sm + s) * PP;
          } else {
            w0 = wn[s];
            if (probe.eigen != nullptr && s < probe.Sm) nE = probe.C;
          }
        }
        auto pix = [&](const cf* base, int i) {
          if (FULL) return *at(base, pbo + EB * i);
          const int px = j + i * G2::T - pad;
          const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
          return base[pyc * pw + pxc];
        };
#pragma unroll
        for (int i = 0; i < 16; ++i) pn[i] = pix(Pn, i) * w0;
        for (int k = 0; k < nE; ++k) {  // uniform, rare (modes owning eigen probes)
          const cf* __restrict__ E = probe.eigen + ((long)k * probe.Sm + s) * PP;
          const float wk = wn[(k + 1) * probe.S + s];
          cf e[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) e[i] = pix(E, i);
          __builtin_amdgcn_sched_barrier(0);  // all 16 in flight before the first use
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            pn[i].x += wk * e[i].x;
            pn[i].y += wk * e[i].y;
          }
        }
      };
      for (int s = 0; s < S; ++s) {
        // (requesting the next mode's probe values ahead of this mode's stores
        // hid one load latency but cost 32 registers: without it the kernel
        // fits 167 VGPRs = 3 waves/SIMD at 256^2 and runs 13 % faster.  At
        // 512^2, where one 512-thread workgroup owns the CU either way and the
        // registers are there, the same request ahead is 5 % slower too:
        // 2.77 -> 2.91 ms per 1000 positions x 4 modes, round 5)
        cf pn[16];
        load_probe(s, pn);
        cf v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = pv[i] * pn[i];
        cf* lbase = lds + line * G2::LS;
        FftStageWave<N, false, 0>::run(v, lbase, j, tw);
#pragma unroll
        for (int i = 0; i < 16; ++i) lbase[tk_pad16(j + i * G2::T)] = v[i];
        __syncthreads();
#pragma unroll
        for (int y2 = 0; y2 < 16; ++y2) v[y2] = lds[y2 * G2::LS + tk_pad16(t)];
        __syncthreads();
        Dft<16, false>::run(v);
        cf* __restrict__ mid = dst0 + s * (long)N * N + (long)(16 * r) * N + t;
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) {
          cf o = v[k1];
          if (k1 > 0) o = mul_tw<false>(o, twtab[N + r * k1]);  // uniform -> scalar load
          if (KEEP)
            mid[k1 * N] = o;
          else
            tk_st_stream(mid + k1 * N, o);
        }
      }
    }
  }
}

// ---- pass 1 at 512^2, one WAVE per row (round 6) ----------------
// fwd_pass1_kernel<512> holds 16 elements per thread (32 threads per row, one
// 512-thread workgroup per CU at 204-244 VGPRs, two waves per SIMD) and moves
// its bytes at 4.1 TB/s where the 256^2 form reaches 5.4.  Here a thread holds
// EIGHT elements (e = lane + 64 i): a row is one wave, 512 = 8 x 8 x 8 in three
// radix-8 stages with two exchanges inside the wave through the row's LDS
// slot; 1024 threads per workgroup = the 16 rows of a group, and in the column
// phase TWO threads share a column (the radix-16 over y2 as one
// decimation-in-frequency step and a radix-8 each: even / odd k1).
// <= 128 VGPRs: four waves per SIMD.  LDS: 16 rows x 545 + 1024 twiddles.
struct TkRow8 {
  static constexpr int N = 512, T = 64, LS = N + N / 16 + 1;
  // twiddles of stages 1 and 2: tab[((s - 1) * 8 + r) * 64 + lane]
  static constexpr int TW_ELEMS = 2 * 8 * 64;
  static __device__ __forceinline__ void fill(cf* tab, const cf* __restrict__ g_tw) {
    for (int idx = threadIdx.x; idx < TW_ELEMS; idx += blockDim.x) {
      const int l = idx & 63, r = (idx >> 6) & 7, st = (idx >> 9) + 1;
      const int Ns = st == 1 ? 8 : 64;
      tab[idx] = g_tw[N + (l & (Ns - 1)) * r * (N / (Ns * 8))];
    }
  }
  // v[i] = element lane + 64 i of the row, in and out (natural order)
  template <bool INV>
  static __device__ __forceinline__ void run(cf (&v)[8], cf* __restrict__ lbase, int l,
                                             const cf* __restrict__ tab) {
#pragma unroll
    for (int st = 0; st < 3; ++st) {
      const int Ns = st == 0 ? 1 : (st == 1 ? 8 : 64);
      if (st > 0) {
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = mul_tw<INV>(v[r], tab[((st - 1) * 8 + r) * 64 + l]);
      }
      Dft<8, INV>::run(v);
      if (st < 2) {
        const int k = l & (Ns - 1);
        const int j0 = (l - k) * 8 + k;
#pragma unroll
        for (int r = 0; r < 8; ++r) lbase[tk_pad16(j0 + r * Ns)] = v[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = lbase[tk_pad16(l + 64 * i)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
};

template <bool FULL, bool KEEP>
__global__ __launch_bounds__(1024, 1) void fwd_pass1_512w_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const TkProbe probe,
    cf* __restrict__ scratch, cf* __restrict__ patches, int nscan, int S, int pw, int H, int W,
    const cf* __restrict__ twtab, const int* __restrict__ skip) {
  constexpr int N = 512, RB = 32, LS = TkRow8::LS;
  constexpr unsigned EB = 64 * sizeof(cf);  // bytes between a thread's elements
  if (skip != nullptr && *skip != 0) return;
  // two sets of 16 rows: mode s + 1 writes its rows while the columns of mode s
  // are still being read -- ONE barrier per mode (the only workgroup of its CU
  // has nobody to hide a second one behind)
  __shared__ cf lds[2 * 16 * LS + TkRow8::TW_ELEMS];
  cf* twl = lds + 2 * 16 * LS;
  TkRow8::fill(twl, twtab);
  __syncthreads();
  const int pad = FULL ? 0 : (N - pw) / 2;
  const long total = (long)H * W;
  const long PP = (long)pw * pw;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int l = threadIdx.x & 63;
  asm volatile("" : "+v"(l));
  const int col = threadIdx.x & 511;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 9));  // even / odd k1
  auto at = [](const cf* base, unsigned byte_off) -> const cf* {
    return reinterpret_cast<const cf*>(reinterpret_cast<const char*>(base) + byte_off);
  };
  for (long item = blockIdx.x; item < (long)nscan * RB; item += gridDim.x) {
    const long n = item / RB;
    const int r = (int)(item % RB);
    const TkCorner c = tk_corner(scan, n);
    cf* __restrict__ dst0 = scratch + n * S * (long)N * N;
    const float* __restrict__ wn =
        probe.weights ? probe.weights + n * (long)(probe.C + 1) * probe.S : nullptr;
    const bool interior = FULL && c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W &&
                          total < (1L << 28);
    // this wave's row: y = r + 32 w, elements e = l + 64 i
    const int py = r + RB * w - pad;
    const int pyc = py < 0 ? 0 : (py >= pw ? pw - 1 : py);
    const unsigned pbo = (unsigned)(pyc * pw + l) * (unsigned)sizeof(cf);
    cf pv[8];
    if (interior) {
      const unsigned g0 = (unsigned)((c.sy + py) * W + c.sx + l) * (unsigned)sizeof(cf);
      const unsigned g1 = g0 + (unsigned)W * (unsigned)sizeof(cf);
      typedef float tk_v4f __attribute__((ext_vector_type(4)));
      auto ld4 = [](const cf* base, unsigned byte_off) {
        tk_v4f v;
        __builtin_memcpy(&v, reinterpret_cast<const char*>(base) + byte_off, sizeof(v));
        return v;
      };
      tk_v4f u[8], lo[8];  // upper row (a, b), lower row (d, e)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u[i] = ld4(psi, g0 + EB * i);
        lo[i] = ld4(psi, g1 + EB * i);
      }
      asm volatile(""
                   : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]),
                     "+v"(u[6]), "+v"(u[7]), "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]),
                     "+v"(lo[4]), "+v"(lo[5]), "+v"(lo[6]), "+v"(lo[7]));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        cf o = mk(u[i].x * c.w00, u[i].y * c.w00);
        o.x += u[i].z * c.w01;
        o.y += u[i].w * c.w01;
        o.x += lo[i].x * c.w10;
        o.y += lo[i].y * c.w10;
        o.x += lo[i].z * c.w11;
        o.y += lo[i].w * c.w11;
        pv[i] = o;
      }
    } else {
      const int y = c.sy + py;
      const bool row_ok = py >= 0 && py < pw && y >= 0 && y < H;
      const int yc = c.sy + pyc < 0 ? 0 : (c.sy + pyc >= H ? H - 1 : c.sy + pyc);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int px = l + 64 * i - pad;
        const int x = c.sx + px;
        const bool ok = row_ok && px >= 0 && px < pw && x >= 0 && x < W;
        const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
        const int xc = c.sx + pxc < 0 ? 0 : (c.sx + pxc >= W ? W - 1 : c.sx + pxc);
        const cf o = tk_gather(psi, (long)yc * W + xc, W, total, c);
        pv[i] = ok ? o : mk(0.f, 0.f);
        __builtin_amdgcn_sched_barrier(0);  // rare path: one element in flight
      }
    }
    if (patches != nullptr && py >= 0 && py < pw) {
      cf* __restrict__ On = patches + n * PP;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int px = l + 64 * i - pad;
        if (FULL)
          tk_st_stream(const_cast<cf*>(at(On, pbo + EB * i)), pv[i]);
        else if (px >= 0 && px < pw)
          tk_st_stream(On + (long)py * pw + px, pv[i]);
      }
    }
    auto pix = [&](const cf* base, int i) {
      if (FULL) return *at(base, pbo + EB * i);
      const int px = l + 64 * i - pad;
      const int pxc = px < 0 ? 0 : (px >= pw ? pw - 1 : px);
      return base[pyc * pw + pxc];
    };
    // probe of (position, mode) (probe.py:272-303, as fwd_pass1_kernel).
    // (Requested one mode ahead, before the transforms of the mode in hand: 12
    // bytes of scratch per lane and 2.76 instead of 2.62 ms per 1000 x 4.)
    auto load_probe = [&](int s, cf (&pn)[8]) {
      const cf* __restrict__ Pn = probe.probe + n * probe.pos_stride + s * PP;
      float w0 = 1.0f;
      int nE = 0;
      if (wn != nullptr) {
        if (probe.unique != nullptr && s < probe.Sm) {
          Pn = probe.unique + (n * probe.Sm + s) * PP;
        } else {
          w0 = wn[s];
          if (probe.eigen != nullptr && s < probe.Sm) nE = probe.C;
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) pn[i] = pix(Pn, i) * w0;
      for (int k = 0; k < nE; ++k) {  // uniform, rare (modes owning eigen probes)
        const cf* __restrict__ E = probe.eigen + ((long)k * probe.Sm + s) * PP;
        const float wk = wn[(k + 1) * probe.S + s];
        cf e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = pix(E, i);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          pn[i].x += wk * e[i].x;
          pn[i].y += wk * e[i].y;
        }
      }
    };
    for (int s = 0; s < S; ++s) {
      cf v[8];
      load_probe(s, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = pv[i] * v[i];
      cf* const set = lds + (s & 1) * 16 * LS;
      cf* lbase = set + w * LS;
      TkRow8::run<false>(v, lbase, l, twl);
#pragma unroll
      for (int i = 0; i < 8; ++i) lbase[tk_pad16(l + 64 * i)] = v[i];
      __syncthreads();
      // column `col` of the 16 rows: the radix-16 over y2 split between TWO
      // threads by one decimation-in-frequency step -- q = 0 the even k1 (radix-8
      // of x[n] + x[n + 8]), q = 1 the odd ones (radix-8 of (x[n] - x[n + 8])
      // w_16^n): all 1024 threads work, eight values each
      cf t[8];
      {
        constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f;
        constexpr float H2 = 0.70710678118654752f;
        const cf w16[8] = {mk(1.f, 0.f),  mk(C1, -S1),  mk(H2, -H2),  mk(S1, -C1),
                           mk(0.f, -1.f), mk(-S1, -C1), mk(-H2, -H2), mk(-C1, -S1)};
#pragma unroll
        for (int y2 = 0; y2 < 8; ++y2) {
          const cf a = set[y2 * LS + tk_pad16(col)];
          const cf b = set[(y2 + 8) * LS + tk_pad16(col)];
          t[y2] = q == 0 ? a + b : (a - b) * w16[y2];
        }
      }
      Dft<8, false>::run(t);
      cf* __restrict__ mid = dst0 + s * (long)N * N + (long)(16 * r) * N + col;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int k1 = 2 * m + q;
        cf o = t[m];
        o = mul_tw<false>(o, twtab[N + r * k1]);  // uniform -> scalar load (k1 = 0: 1)
        if (KEEP)
          mid[k1 * N] = o;
        else
          tk_st_stream(mid + k1 * N, o);
      }
    }
    // (the next item starts at set 0 again: after an odd number of modes that
    // is the set just read)
    if (S & 1) __syncthreads();
  }
}

// unique_probe: the varying probe of the first eigen_modes modes from
// tike_varying_probe, or NULL with eigen_probe given: formed on the fly.
int tk_fwd_pass1(const void* psi, const float* scan, const void* probe,
                        int probe_per_scan, const void* unique_probe, const void* eigen_probe,
                        const float* eigen_weights, int num_eigen, int eigen_modes, void* scratch,
                        void* patches, int nscan, int S, int pw, int det, int H, int W,
                        hipStream_t stream, const int* skip, bool keep) {
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  TK_CHECK_ARG(!(eigen_weights && probe_per_scan));
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(psi && scan && probe && scratch);
  TK_CHECK_ARG(!(eigen_weights && eigen_modes > 0 && !unique_probe && !eigen_probe));
  if (det != 128 && det != 256 && det != 512) return TK_ERR_UNSUPPORTED;
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  const TkProbe P = tk_make_probe(probe, probe_per_scan, unique_probe ? nullptr : eigen_probe,
                                  eigen_weights, num_eigen, eigen_modes, S, pw, unique_probe);
#define TK_F1K(N, FULL, KEEP)                                                                   \
  hipLaunchKernelGGL((fwd_pass1_kernel<N, FULL, KEEP>),                                        \
                     dim3(tk_grid((long)nscan * (N / 16), N == 512 ? 1 : (N == 256 ? 8 : 16))), \
                     dim3(N), 0, stream, (const cf*)psi, scan, P, (cf*)scratch, (cf*)patches,   \
                     nscan, S, pw, H, W, tw, skip)
#define TK_F1(N, FULL)      \
  do {                      \
    if (keep)               \
      TK_F1K(N, FULL, true);  \
    else                    \
      TK_F1K(N, FULL, false); \
  } while (0)
  if (det == 128 && pw == det)  // (a multislice object: tike_slice_step's partner)
    TK_F1(128, true);
  else if (det == 128)
    TK_F1(128, false);
  else if (det == 256 && pw == det)
    TK_F1(256, true);
  else if (det == 256)
    TK_F1(256, false);
  else {
    // 512^2: one wave per row, 1024 threads (fwd_pass1_kernel<512>: 2.77 ms per
    // 1000 positions x 4 modes; this one 2.61)
#define TK_F1W(FULL, KEEP)                                                                      \
  hipLaunchKernelGGL((fwd_pass1_512w_kernel<FULL, KEEP>), dim3(tk_grid((long)nscan * 32, 1)),   \
                     dim3(1024), 0, stream, (const cf*)psi, scan, P, (cf*)scratch,              \
                     (cf*)patches, nscan, S, pw, H, W, tw, skip)
    if (pw == det && keep)
      TK_F1W(true, true);
    else if (pw == det)
      TK_F1W(true, false);
    else if (keep)
      TK_F1W(false, true);
    else
      TK_F1W(false, false);
#undef TK_F1W
  }
#undef TK_F1
#undef TK_F1K
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_fwd_pass1(const void* psi, const float* scan, const void* probe,
                              int probe_per_scan, const void* unique_probe,
                              const void* eigen_probe, const float* eigen_weights,
                              int num_eigen, int eigen_modes, void* scratch, void* patches,
                              int nscan, int S, int pw, int det, int H, int W, void* stream_) {
  TK_ENTER();
  return tk_fwd_pass1(psi, scan, probe, probe_per_scan, unique_probe, eigen_probe, eigen_weights,
                      num_eigen, eigen_modes, scratch, patches, nscan, S, pw, det, H, W,
                      (hipStream_t)stream_, nullptr);
}

// ------------------------------------------- 128^2: the whole tile in LDS
// A 128 x 128 complex tile is 128 KiB: it fits the 160 KiB LDS of a CU, so the
// 2-D transform needs NO intermediate in memory -- the only HBM traffic of the
// forward operator is its output, written once, straight from registers.
// One workgroup of 1024 threads (one per CU) per position; per mode:
//   rows     thread (row, j) gathers its 16 pixels (bilinear taps * probe)
//            straight into the FFT register layout, runs the 128-point row
//            transform (radix 16 x 8, the exchange stays inside its wave) and
//            leaves the row spectrum in the LDS tile;
//   columns  the same 8 threads then own COLUMN `line`: its 128 elements
//            (stride LS) go through the same in-wave radix 16 x 8 plan, the
//            column itself being the exchange buffer -- no workgroup barrier
//            and no second trip of the tile through LDS -- and leave for the
//            far plane from registers (8 rows x 64 contiguous bytes per wave
//            store; the neighbouring wave writes the other half of each line).
//            Two workgroup barriers per mode (rows done / columns done).
// The intensity sum_s |F_s|^2 accumulates in registers across the modes.
// LDS row stride: 136 elements = 272 dwords = 16 (mod 64 banks), so the four
// rows a 32-lane read group touches (8 lanes x 16 dwords each) tile the 64
// banks exactly; 136 also holds the padded row (127 + 127/16 = 134).
// (TK_L128_LS, tk_l128_swizzle: fft_engine2.h -- csrc/pfa.hip runs the same tile)
template <bool WITH_I>
__global__ __launch_bounds__(1024, 4) void fwd128_lds_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const TkProbe probe,
    cf* __restrict__ farplane, float* __restrict__ intensity, cf* __restrict__ patches, int nscan,
    int S, int H, int W, float scale, const cf* __restrict__ twtab,
    const int* __restrict__ skip) {
  constexpr int N = 128, T = 8, LS = TK_L128_LS;
  static_assert(FftPlan<N>::E == 16 && LS >= N + N / 16, "row plan: 16 elements x 8 threads");
  __shared__ cf lds[N * LS + FftTwLds<N>::ELEMS];
  if (skip != nullptr && *skip != 0) return;  // speculative launch, not needed
  cf* twl = lds + N * LS;
  FftTwLds<N>::fill(twl, twtab);
  __syncthreads();
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  int line = tid / T, j = tid % T;
  asm volatile("" : "+v"(line), "+v"(j));
  const FftTwLds<N> tw{twl, j};
  __builtin_assume(j >= 0 && j < T && line >= 0 && line < N);
  const long PP = (long)N * N;
  const long total = (long)H * W;
  auto at = [](const cf* base, unsigned byte_off) -> const cf* {
    return reinterpret_cast<const cf*>(reinterpret_cast<const char*>(base) + byte_off);
  };
  for (long n = blockIdx.x; n < nscan; n += gridDim.x) {
    const TkCorner c = tk_corner(scan, n);
    const bool interior = c.sy >= 0 && c.sx >= 0 && c.sy + N < H && c.sx + N < W &&
                          total < (1L << 28);
    // ---- bilinear patch of row `line`, elements e = j + 8 i
    cf pv[16];
    if (interior) {
      // One 8-byte load per pixel and row: the tap to the right (x + 1) is the
      // neighbouring lane's pixel (lane + 1 holds x + 1 for j < 7; for j == 7
      // it is slot i + 1 of the lane with j = 0, seven lanes down), fetched
      // with DPP row shifts.  Slot 16 is the pixel x = 128 + j that closes the
      // row (only j = 0's is used).  Two batches of loads: row y, then row y+1.
      const unsigned g0 = (unsigned)((c.sy + line) * W + c.sx + j) * (unsigned)sizeof(cf);
      const unsigned g1 = g0 + (unsigned)W * (unsigned)sizeof(cf);
      // slot 16 of the lanes j > 0 would lie past x = 128: read x = 128 too
      const unsigned gx = (unsigned)(128 - j) * (unsigned)sizeof(cf);
      auto right = [&](const cf (&a)[17], int i) {
        // value of pixel x + 1 for slot i
        auto dpp = [](float v, int ctrl_shl) {
          return ctrl_shl
                     ? __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                                     0, __builtin_bit_cast(int, v), 0x101, 0xF,
                                                     0xF, true))   // row_shl:1  (lane + 1)
                     : __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                                     0, __builtin_bit_cast(int, v), 0x117, 0xF,
                                                     0xF, true));  // row_shr:7  (lane - 7)
        };
        const cf nx = mk(dpp(a[i].x, 1), dpp(a[i].y, 1));
        const cf wr = mk(dpp(a[i + 1].x, 0), dpp(a[i + 1].y, 0));
        return j < 7 ? nx : wr;
      };
      cf up[17], lo[17];
#pragma unroll
      for (int i = 0; i < 16; ++i) up[i] = *at(psi, g0 + 64 * i);
      up[16] = *at(psi, g0 + gx);
      asm volatile(""
                   : "+v"(up[0].x), "+v"(up[1].x), "+v"(up[2].x), "+v"(up[3].x), "+v"(up[4].x),
                     "+v"(up[5].x), "+v"(up[6].x), "+v"(up[7].x), "+v"(up[8].x), "+v"(up[9].x),
                     "+v"(up[10].x), "+v"(up[11].x), "+v"(up[12].x), "+v"(up[13].x),
                     "+v"(up[14].x), "+v"(up[15].x), "+v"(up[16].x));
#pragma unroll
      for (int i = 0; i < 16; ++i) lo[i] = *at(psi, g1 + 64 * i);
      lo[16] = *at(psi, g1 + gx);
      asm volatile(""
                   : "+v"(lo[0].x), "+v"(lo[1].x), "+v"(lo[2].x), "+v"(lo[3].x), "+v"(lo[4].x),
                     "+v"(lo[5].x), "+v"(lo[6].x), "+v"(lo[7].x), "+v"(lo[8].x), "+v"(lo[9].x),
                     "+v"(lo[10].x), "+v"(lo[11].x), "+v"(lo[12].x), "+v"(lo[13].x),
                     "+v"(lo[14].x), "+v"(lo[15].x), "+v"(lo[16].x));
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const cf b = right(up, i), e = right(lo, i);
        cf o = mk(up[i].x * c.w00, up[i].y * c.w00);
        o.x += b.x * c.w01;
        o.y += b.y * c.w01;
        o.x += lo[i].x * c.w10;
        o.y += lo[i].y * c.w10;
        o.x += e.x * c.w11;
        o.y += e.y * c.w11;
        pv[i] = o;
      }
    } else {
      const int y = c.sy + line;
      const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int x = c.sx + j + i * T;
        const bool ok = y >= 0 && y < H && x >= 0 && x < W;
        const int xc = x < 0 ? 0 : (x >= W ? W - 1 : x);
        const cf o = tk_gather(psi, (long)yc * W + xc, W, total, c);
        pv[i] = ok ? o : mk(0.f, 0.f);
        __builtin_amdgcn_sched_barrier(0);  // rare path: one element in flight
      }
    }
    if (patches != nullptr) {
      // O_n for the gradient kernels (uniform branch; the solver's 128^2 path)
      cf* __restrict__ On = patches + n * PP + line * N + j;
#pragma unroll
      for (int i = 0; i < 16; ++i) tk_st_stream(On + i * T, pv[i]);
    }
    float I[16];
    if (WITH_I) {
#pragma unroll
      for (int i = 0; i < 16; ++i) I[i] = 0.f;
    }
    const unsigned pbo = (unsigned)(line * N + j) * (unsigned)sizeof(cf);
    for (int s = 0; s < S; ++s) {
      // probe of (position, mode)
      const cf* __restrict__ Pn = probe.probe + n * probe.pos_stride + s * PP;
      float w0 = 1.0f;
      if (probe.weights != nullptr) {
        if (probe.unique != nullptr && s < probe.Sm)
          Pn = probe.unique + (n * probe.Sm + s) * PP;
        else
          w0 = probe.weights[n * (long)(probe.C + 1) * probe.S + s];
      }
      cf v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = pv[i] * (*at(Pn, pbo + 64 * i) * w0);
      // ---- row transform (the row of the tile is its own exchange buffer),
      // spectrum into the tile at the swizzled columns
      cf* lbase = lds + line * LS;
      FftStageWave<N, false, 0>::run(v, lbase, j, tw);
      const int rsw = tk_l128_swizzle(line);
#pragma unroll
      for (int i = 0; i < 16; ++i) lbase[(j + i * T + rsw) & (N - 1)] = v[i];
      __syncthreads();
      // ---- column transform: the 8 threads that shared row `line` now share
      // COLUMN `line`; its 128 elements (stride LS) are their exchange buffer
      const int col = line;
      auto cat = [&](int e) { return e * LS + ((col + tk_l128_swizzle(e)) & (N - 1)); };
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = lds[cat(j + i * T)];
      FftStageWave<N, false, 0>::run_at(v, lds, j, tw, cat);
      cf* __restrict__ dst = farplane + (n * S + s) * PP + col;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const cf o = v[i] * scale;
        if (farplane != nullptr) tk_st_stream(dst + (long)(j + i * T) * N, o);
        if (WITH_I) I[i] += norm2(o);
      }
      __syncthreads();  // the next mode's rows overwrite the tile
    }
    if (WITH_I) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        tk_st_stream(intensity + n * PP + (long)(j + i * T) * N + line, I[i]);
    }
  }
}

int launch_fwd128_lds(const cf* psi, const float* scan, const TkProbe& probe, cf* farplane,
                             float* intensity, int nscan, int S, int H, int W, float scale,
                             hipStream_t stream, cf* patches, const int* skip) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  const dim3 grid(tk_grid(nscan, 1)), block(1024);
  if (intensity)
    hipLaunchKernelGGL((fwd128_lds_kernel<true>), grid, block, 0, stream, psi, scan, probe,
                       farplane, intensity, patches, nscan, S, H, W, scale, tw, skip);
  else
    hipLaunchKernelGGL((fwd128_lds_kernel<false>), grid, block, 0, stream, psi, scan, probe,
                       farplane, intensity, patches, nscan, S, H, W, scale, tw, skip);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

template <int N>
static int launch_fwd_v2(const cf* psi, const float* scan, const TkProbe& probe, cf* farplane,
                         long ntile, int S, int pw, int H, int W, float scale,
                         hipStream_t stream) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  hipLaunchKernelGGL((ptycho_fwd_v2_kernel<N>), dim3(tk_grid(ntile, 4)), dim3(N), 0, stream, psi,
                     scan, probe, farplane, ntile, S, pw, H, W, scale, tw);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

template <int N>
static int launch_fwd(const cf* psi, const float* scan, const TkProbe& probe, cf* farplane,
                      long ntile, int S, int pw, int H, int W, float scale, hipStream_t stream) {
  const cf* tw = tk_twiddles();
  if (!tw) return (int)hipErrorNotInitialized;
  hipLaunchKernelGGL((ptycho_fwd_kernel<N>), dim3(tk_grid(ntile, N >= 512 ? 2 : 4)),
                     dim3(FftPlan<N>::NT), 0, stream, psi, scan, probe, farplane, ntile, S, pw, H,
                     W, scale, tw);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// The forward column pass alone, in place on the far-plane array: rows
// {k1 + 16 r} of a tile in, the same rows out (fft_engine2.h pass 2), so a
// tile written by forward pass 1 becomes the far plane without a second array.
// Work item = (tile, k1, 256-column block); tiles in descending order (pass 1
// wrote them ascending: its last tiles are still in the Infinity Cache).
template <int N>
__global__ __launch_bounds__(256, N == 256 ? 4 : 2) void fwd_colpass_inplace_kernel(
    cf* far, long ntile, float scale) {
  constexpr int RB = N / 16, NH = N / 256;
  const long nitem = ntile * 16 * NH;
  for (long v = blockIdx.x; v < nitem; v += gridDim.x) {
    const int hb = (int)(v % NH);
    const int k1 = (int)((v / NH) & 15);
    const long tile = ntile - 1 - v / (16 * NH);
    cf* p = far + tile * (long)N * N + (long)k1 * N + hb * 256 + threadIdx.x;
    cf u[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) u[r] = p[(long)(16 * r) * N];
    Dft<RB, false>::run(u);
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) tk_st_stream(p + (long)(16 * k2) * N, u[k2] * scale);
  }
}

extern "C" int tike_ptycho_fwd(const void* psi, const float* scan, const void* probe,
                               int probe_per_scan, const void* eigen_probe,
                               const float* eigen_weights, int num_eigen, int eigen_modes,
                               void* farplane, int nscan, int S, int pw, int det, int H, int W,
                               float scale, int sub_batch, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(psi && scan && probe && farplane);
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  TK_CHECK_ARG(!(eigen_weights && probe_per_scan));
  if (nscan == 0) return TK_OK;
  const TkProbe P = tk_make_probe(probe, probe_per_scan, eigen_probe, eigen_weights, num_eigen,
                                  eigen_modes, S, pw);
  const long ntile = (long)nscan * S;
  const cf* psi_ = (const cf*)psi;
  cf* far = (cf*)farplane;
  if (det == 128 && pw == 128 && !(eigen_weights && eigen_modes > 0))
    return launch_fwd128_lds(psi_, scan, P, far, nullptr, nscan, S, H, W, scale, stream, nullptr);
  if (det == 512 || det == 256) {
    // forward pass 1 (the patch of a row group gathered once for all modes,
    // eigen probes on the fly) straight into the far-plane array, then the
    // column pass in place -- two streaming kernels; faster than one workgroup
    // per tile / per position (below) for every mode count: 256^2 x 1 mode
    // 2.57 -> 2.75 M tiles/s, x 3 modes +22 %, 512^2 +47 %
    // ... in sub-batches of about 256 MiB of far plane: pass 1 keeps its
    // hand-off in the Infinity Cache (plain stores), the column pass that
    // follows reads it from there and overwrites it in place, so HBM sees the
    // far plane once (256^2 x 1 mode: 2.83 -> 2.95 M patterns/s; smaller
    // sub-batches lose more to their launches than the cache returns,
    // profiles/r04_experiments.md).  sub_batch = positions per sub-batch
    // (0: the 256 MiB default; < 0: one batch) -- an argument, the entry
    // reads no environment.
    const size_t tile_bytes = sizeof(cf) * (size_t)det * det;
    long sub = sub_batch > 0   ? sub_batch
               : sub_batch < 0 ? nscan
                               : (256L << 20) / (long)(tile_bytes * S);
    if (sub < 1) sub = 1;
    const bool keep = sub < nscan;
    for (long lo = 0; lo < nscan; lo += sub) {
      const int m = (int)(nscan - lo < sub ? nscan - lo : sub);
      int rc = tk_fwd_pass1(psi, scan + 2 * lo,
                            (const char*)probe +
                                (probe_per_scan ? sizeof(cf) * (size_t)S * pw * pw * lo : 0),
                            probe_per_scan, nullptr, eigen_probe,
                            eigen_weights ? eigen_weights + lo * (num_eigen + 1) * S : nullptr,
                            num_eigen, eigen_modes, (char*)farplane + tile_bytes * S * lo,
                            nullptr, m, S, pw, det, H, W, stream, nullptr, keep);
      if (rc) return rc;
      const long mt = (long)m * S;
      const long nitem = mt * 16 * (det / 256);
      cf* fm = far + lo * S * det * det;
      if (det == 256)
        hipLaunchKernelGGL((fwd_colpass_inplace_kernel<256>), dim3(tk_grid(nitem, 32)),
                           dim3(256), 0, stream, fm, mt, scale);
      else
        hipLaunchKernelGGL((fwd_colpass_inplace_kernel<512>), dim3(tk_grid(nitem, 32)),
                           dim3(256), 0, stream, fm, mt, scale);
    }
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  if (S > 1 && !(eigen_weights && eigen_modes > 0)) {
    // position-major kernel (patch gathered once per position and shared by
    // the modes, straight-line loader; with a single mode there is nothing to
    // share and the tile-major kernel below, with its higher occupancy, is
    // 7 % faster); the varying-probe case needs tike_varying_probe first and
    // is served by tike_ptycho_fwd_intensity
    // (256 / 512 never get here: the two streaming kernels above)
    if (det == 128)
      return launch_fwd_pos<128>(psi_, scan, P, far, nullptr, nscan, S, pw, H, W, scale, stream);
  }
  if (det == 128)
    return launch_fwd_v2<128>(psi_, scan, P, far, ntile, S, pw, H, W, scale, stream);
  switch (det) {
    case 32: return launch_fwd<32>(psi_, scan, P, far, ntile, S, pw, H, W, scale, stream);
    case 64: return launch_fwd<64>(psi_, scan, P, far, ntile, S, pw, H, W, scale, stream);
    case 1024: return launch_fwd<1024>(psi_, scan, P, far, ntile, S, pw, H, W, scale, stream);
    default: break;
  }
  // any other detector size: unfused gather*probe, then the generic DFT in place
  int rc = tk_conv_fwd(psi_, scan, P, far, nscan, S, pw, det, H, W, stream);
  if (rc) return rc;
  return tk_fft2(far, far, ntile, det, 0, scale, stream);
}
