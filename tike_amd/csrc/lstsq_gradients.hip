// The two gradients of the least-squares + gradient update loop (lstsq_grad)
// for gfx950, and the probe preconditioner.
//
// Reference: src/tike/ptycho/solvers/lstsq.py (one minibatch):
//   :506-520  object gradient  sum_s conj(P_n,s) chi_n,s             -> tike_lstsq_gradients (scattered by scatter.hip)
//   :524-539  probe gradient   sum_n conj(O_n) chi_n,s               -> tike_lstsq_gradients (tike_probe_grad)
//   :504-539  the same behind the inverse transform's second pass    -> tike_ifft2_pass2_gradients{,_scaled,_eproj,_modes}
//   solvers/_preconditioner.py:116-167 probe preconditioner          -> tike_probe_preconditioner
// where chi is the exit-wave update (IFFT2 of the far-plane gradient cropped
// to the probe window), P_n,s the probe at position n (shared probe plus
// eigen probes synthesised on the fly) and O_n the bilinear object patch.
// probe_chunk is shared with the minibatch tail, lstsq.hip (internal.h).
#include "fft_engine2.h"
#include <type_traits>

#include "internal.h"
#include "tike_amd.h"

// ------------------------------------------------------------ probe gradient
// One thread per probe pixel, a workgroup walks a chunk of positions keeping S
// complex accumulators in registers; one atomic pair per (pixel, mode, chunk).
// Optionally stores the object patches (B, pw, pw) for later passes.
constexpr int TK_MAX_MODES = 16;

// SC = compile-time number of modes (0: runtime S <= TK_MAX_MODES).  With SC
// known the mode loop has no branches, so all S loads of a position are in
// flight together instead of one memory latency per mode.
template <bool WITH_CHI, int SC>
__global__ __launch_bounds__(256) void probe_grad_kernel(
    const cf* __restrict__ chi, const float* __restrict__ scan, const cf* __restrict__ psi,
    cf* __restrict__ patches, float* __restrict__ out, const TkProbe probe,
    cf* __restrict__ objproj, int nscan, int S_rt, int pw, int H, int W, int chunk,
    float* __restrict__ part) {
  constexpr int SM = SC > 0 ? SC : TK_MAX_MODES;
  const int S = SC > 0 ? SC : S_rt;
  const long P = (long)pw * pw;
  const long total = (long)H * W;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b0 = blockIdx.y * chunk;
  const int b1 = min(nscan, b0 + chunk);
  if (p >= P) return;
  const int py = (int)(p / pw), px = (int)(p % pw);
  cf acc[SM];
#pragma unroll
  for (int s = 0; s < SM; ++s) acc[s] = mk(0.f, 0.f);
  // The shared probe value of this pixel is the same for every position of
  // the chunk: keep it in registers instead of re-reading it per position
  // (only the modes that own eigen probes vary beyond a scalar weight).
  const bool hoist = WITH_CHI && objproj != nullptr && probe.pos_stride == 0;
  cf pr[SM];
  if (hoist) {
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (SC > 0 || s < S) pr[s] = probe.probe[s * P + p];
  }
  for (int b = b0; b < b1; ++b) {
    const TkCorner c = tk_corner(scan, b);
    const int y = c.sy + py, x = c.sx + px;
    const bool ok = y >= 0 && y < H && x >= 0 && x < W;
    const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
    const int xc = x < 0 ? 0 : (x >= W ? W - 1 : x);
    cf xs[SM];
    if (WITH_CHI) {
#pragma unroll
      for (int s = 0; s < SM; ++s)
        if (SC > 0 || s < S) xs[s] = tk_ld_stream(chi + ((long)b * S + s) * P + p);
    }
    cf o;
    // interior position (uniform): the two taps of a row are adjacent complex
    // values, one 16-byte load each -- half the L1 requests of four 8-byte taps
    if (!WITH_CHI && c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W &&
        total < (1L << 28)) {
      typedef float tk_v4f __attribute__((ext_vector_type(4)));
      const unsigned off = (unsigned)(y * W + x) * (unsigned)sizeof(cf);
      tk_v4f u, l;
      __builtin_memcpy(&u, reinterpret_cast<const char*>(psi) + off, sizeof(u));
      __builtin_memcpy(&l, reinterpret_cast<const char*>(psi) + off + (unsigned)W * 8u, sizeof(l));
      o = mk(u.x * c.w00, u.y * c.w00);
      o.x += u.z * c.w01;
      o.y += u.w * c.w01;
      o.x += l.x * c.w10;
      o.y += l.y * c.w10;
      o.x += l.z * c.w11;
      o.y += l.w * c.w11;
    } else {
      o = tk_gather(psi, (long)yc * W + xc, W, total, c);
      if (!ok) o = mk(0.f, 0.f);
    }
    if (patches) patches[b * P + p] = o;
    if (WITH_CHI) {
      const cf oc = conjf(o);
      cf proj = mk(0.f, 0.f);
#pragma unroll
      for (int s = 0; s < SM; ++s)
        if (SC > 0 || s < S) {
          if (out) acc[s] = acc[s] + oc * xs[s];
          if (objproj) {
            cf ps;
            // (the first Sm modes vary by more than a weight: eigen probes, or
            // a unique probe passed in their place)
            if (hoist && !(probe.weights != nullptr && s < probe.Sm &&
                           (probe.eigen != nullptr || probe.unique != nullptr))) {
              const float w0 =
                  probe.weights ? probe.weights[b * (long)(probe.C + 1) * probe.S + s] : 1.0f;
              ps = pr[s] * w0;
            } else {
              ps = probe.at(b, s, p);
            }
            proj = proj + conjf(ps) * xs[s];
          }
        }
      if (objproj) objproj[b * P + p] = proj;
    } else {
      acc[0].x += norm2(o);
    }
  }
  // deterministic mode: the chunk's sums go to its own row of `part`, added in
  // a fixed order after the launch (tk_ordered_sum)
  if (WITH_CHI) {
    if (out) {
#pragma unroll
      for (int s = 0; s < SM; ++s)
        if (SC > 0 || s < S) {
          if (part != nullptr) {
            float* o = part + 2 * (((long)blockIdx.y * S + s) * P + p);
            o[0] = acc[s].x;
            o[1] = acc[s].y;
          } else {
            unsafeAtomicAdd(&out[2 * (s * P + p)], acc[s].x);
            unsafeAtomicAdd(&out[2 * (s * P + p) + 1], acc[s].y);
          }
        }
    }
  } else if (part != nullptr) {
    part[(long)blockIdx.y * P + p] = acc[0].x;
  } else {
    unsafeAtomicAdd(&out[2 * p], acc[0].x);
  }
}

template <bool WITH_CHI>
static void launch_probe_grad(dim3 grid, hipStream_t stream, const cf* chi, const float* scan,
                              const cf* psi, cf* patches, float* out, const TkProbe& probe,
                              cf* objproj, int nscan, int S, int pw, int H, int W, int chunk,
                              float* part = nullptr) {
#define TK_PG(SC)                                                                              \
  hipLaunchKernelGGL((probe_grad_kernel<WITH_CHI, SC>), grid, dim3(256), 0, stream, chi, scan, \
                     psi, patches, out, probe, objproj, nscan, S, pw, H, W, chunk, part)
  switch (WITH_CHI ? S : 1) {
    case 1: TK_PG(1); break;
    case 2: TK_PG(2); break;
    case 3: TK_PG(3); break;
    case 4: TK_PG(4); break;
    case 5: TK_PG(5); break;
    case 6: TK_PG(6); break;
    case 8: TK_PG(8); break;
    default: TK_PG(0); break;
  }
#undef TK_PG
}

// Positions per chunk of the sums over positions, and -- deterministic mode --
// where the chunks leave their partial sums (`len` floats each; *part stays
// NULL otherwise).  When the caller's scratch buffer cannot hold them the
// launch falls back to ONE chunk, so that every sum has a single contributor
// per address (its one atomic then only adds to what earlier, stream-ordered
// launches left there).
int probe_chunk(int nscan, long len, float** part) {
  // enough position chunks to fill the chip, at least 8 positions each
  int chunk = (nscan + 31) / 32;
  chunk = chunk < 8 ? 8 : chunk;
  if (!tk_deterministic()) return chunk;
  const int nchunk = (nscan + chunk - 1) / chunk;
  float* p = len > 0 && part ? tk_det_scratch(sizeof(float) * (size_t)len * nchunk) : nullptr;
  if (p != nullptr) {
    *part = p;
    return chunk;
  }
  return nscan > 8 ? nscan : 8;
}

extern "C" int tike_probe_grad(const void* chi, const float* scan, const void* psi,
                               void* patches, void* m_probe_update, int nscan, int S, int pw,
                               int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && S <= TK_MAX_MODES && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(chi && scan && psi && m_probe_update);
  const long P = (long)pw * pw;
  float* part = nullptr;
  const int chunk = probe_chunk(nscan, 2 * S * P, &part);
  dim3 grid((unsigned)((P + 255) / 256), (unsigned)((nscan + chunk - 1) / chunk));
  launch_probe_grad<true>(grid, (hipStream_t)stream, (const cf*)chi, scan, (const cf*)psi,
                          (cf*)patches, (float*)m_probe_update,
                          tk_make_probe(psi, 0, nullptr, nullptr, 0, 0, S, pw), (cf*)nullptr,
                          nscan, S, pw, H, W, chunk, part);
  TK_LAUNCH_CHECK();
  if (part != nullptr)
    return tk_ordered_sum((float*)m_probe_update, part, 2 * S * P, (int)grid.y, true,
                          (hipStream_t)stream);
  return TK_OK;
}

// One pass over chi for BOTH gradients (lstsq.py:506-539):
//   m_probe_update (S,pw,pw) += sum_n conj(O_n) chi_n,s          (may be NULL)
//   objproj (nscan,pw,pw)     = sum_s conj(P_n,s) chi_n,s        (may be NULL)
//   patches (nscan,pw,pw)     = O_n = patch_n(psi)               (may be NULL)
extern "C" int tike_lstsq_gradients(const void* chi, const float* scan, const void* psi,
                                    const void* probe, const void* eigen_probe,
                                    const float* eigen_weights, int num_eigen, int eigen_modes,
                                    const void* unique_probe, void* patches,
                                    void* m_probe_update, void* objproj, int nscan, int S,
                                    int pw, int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && S <= TK_MAX_MODES && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(chi && scan && psi && probe);
  const long P = (long)pw * pw;
  float* part = nullptr;
  const int chunk = probe_chunk(nscan, m_probe_update ? 2 * S * P : 0, &part);
  dim3 grid((unsigned)((P + 255) / 256), (unsigned)((nscan + chunk - 1) / chunk));
  launch_probe_grad<true>(grid, (hipStream_t)stream, (const cf*)chi, scan, (const cf*)psi,
                          (cf*)patches, (float*)m_probe_update,
                          tk_make_probe(probe, 0, eigen_probe, eigen_weights, num_eigen,
                                        eigen_modes, S, pw, unique_probe),
                          (cf*)objproj, nscan, S, pw, H, W, chunk, part);
  TK_LAUNCH_CHECK();
  if (part != nullptr)
    return tk_ordered_sum((float*)m_probe_update, part, 2 * S * P, (int)grid.y, true,
                          (hipStream_t)stream);
  return TK_OK;
}

// ------------------------------------------- inverse pass 2 + both gradients
// The second pass of the inverse 2-D FFT (fft_engine2.h: in-place radix-RB over
// rows {ya + 16 k}) run PIXEL-major and fused with everything that consumes
// the exit-wave update chi (lstsq.py:504-539), so chi is never stored:
//   objproj_n      = sum_s conj(P_n,s) chi_n,s      (one write per position)
//   m_probe_update += sum_n conj(O_n) chi_n,s       (register accumulators over
//                                                    a chunk of positions, one
//                                                    atomic per pixel/mode/chunk)
//   chi0_n         = chi_n,0                        (step sizes, eigen probes,
//                                                    position correction)
// Probe window = detector (pw == N).  A workgroup owns one slice of the tile:
// the RB rows {ya + 16 yb} -- exactly what one radix-RB butterfly per thread
// consumes and produces -- by 64 * (4 / MW) columns, and walks a chunk of
// positions.  Its four waves are MW mode-waves x (4 / MW) column-waves: wave
// (mw, cw) handles modes {mw, mw + MW, ...} (MPW of them) of column block cw,
// lane = column, so every global access is a 512-byte row segment at one of
// the RB offsets off0 + yb * 16 N (the same offsets for the intermediate,
// the patches, the probe and every output).  The per-position sum over modes
// crosses the mode-waves through LDS: every wave leaves its partial sum in a
// slot of its own, one barrier, then mode-wave mw adds the slots of rows
// yb = mw (mod MW) and writes them (slots double buffered where they fit).
struct TkModeProbe {  // probe of one (position, mode): uniform values
  const cf* base;     // shared probe of the mode, or its synthesised varying probe
  float w0;           // scale of `base`
  int nE;             // eigen probes to add on the fly (0 when `base` is final)
};

// EIG: eigen probes are applied on the fly (their loops cost the 512^2
// instantiation 19 spilled registers when compiled in and never taken).
// GRP (round 6: more modes than one launch holds in registers -- 9 .. 16 at
// 256^2): the launch serves S consecutive modes of a problem with Stot modes
// per position (`mid`, `probe`, the weights and `mpu` arrive offset to the
// first of them; tiles and mode_scale are Stot apart) and, `accumulate`, adds
// its projection to what the launch of the group in front left in objproj.
// QN (eigen probes in LDS, N <= 256): the wave of mode 0 also forms
//   q_n = sum_p Re(conj(O_n) chi_n,0 conj(E_0,0))
// over its pixels from the values it holds, one partial per (position,
// column-wave of a slice): qtab[(slice * CW + cw) * nscan + n] (plain stores, N / 4
// partials per position, added up in a fixed order by the launcher).
template <int N, int MW, int MPW, bool HAVE_PROJ, bool EIG = true, bool GRP = false,
          bool QN = false>
__global__ __launch_bounds__(256, 2) void ifft2_pass2_gradients_kernel(
    const cf* __restrict__ mid, const cf* __restrict__ patches, const TkProbe probe,
    cf* __restrict__ objproj, cf* __restrict__ chi0, float* __restrict__ mpu, float mpu_scale,
    int nscan, int S, float inv_scale, int chunk, float* __restrict__ mpu_part,
    const float* __restrict__ mode_scale, int Stot_ = 0, int accumulate_ = 0,
    float* __restrict__ qtab = nullptr) {
  const int Stot = GRP ? Stot_ : S;
  const bool accumulate = GRP && accumulate_ != 0;
  constexpr int RB = N / 16;
  constexpr int CW = 4 / MW;            // column-waves per workgroup
  constexpr int NCB = N / (64 * CW);    // column blocks
  constexpr int NSLICE = 16 * NCB;      // (ya, column block) slices
  constexpr bool REDUCE = HAVE_PROJ && MW > 1;
  // RB = 32 (N = 512): the accumulators and one butterfly already fill the
  // register file, so probe and patch values are re-read (L2) per use
  constexpr bool HOIST = RB <= 16;
  static_assert(NCB >= 1 && NSLICE % 8 == 0, "slice layout");
  static_assert(!QN || (HOIST && EIG && HAVE_PROJ && !GRP && NSLICE * CW == N / 4),
                "q_n partials: eigen slices in LDS, patch values in registers");
  constexpr int NBUF = RB <= 16 ? 2 : 1;  // slot sets (2: one barrier per position)
  __shared__ cf part[REDUCE ? NBUF * 4 * RB * 64 : 1];  // [buf][wave][yb][lane]
  extern __shared__ cf eigl[];  // conj(E_c,s) on this slice: [C][Sm][RB][64 CW]
  constexpr long P = (long)N * N;
  // XCD-aware slice order: workgroup v runs on XCD v % 8 (round-robin
  // dispatch); every XCD keeps NSLICE/8 slices, so its L2 holds 1/8 of the
  // probe and of the patches.  Placement affects speed only.
  const int v = blockIdx.x;
  constexpr int per = NSLICE / 8;
  const int slice = (v & 7) * per + (v >> 3) % per;
  // chunks in DESCENDING order: the inverse pass 1 wrote the intermediate in
  // ascending position order, its tail is still in the Infinity Cache
  const int nchunk_ = (nscan + chunk - 1) / chunk;
  const int b0 = (nchunk_ - 1 - ((v >> 3) / per)) * chunk;
  const int b1 = min(nscan, b0 + chunk);
  const int ya = slice / NCB, cb = slice % NCB;
  // the wave index is uniform: say so, so that everything derived from it
  // (mode, column block, base pointers, weights) lives in scalar registers
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int mw = w % MW, cw = w / MW;
  constexpr long ROW = 16 * N;  // elements between the rows of this slice
  // uniform element offset of the slice's first row and column block, and the
  // per-lane byte offset inside a row segment
  const long slice0 = (long)ya * N + (cb * CW + cw) * 64;
  const unsigned lb = (unsigned)lane * (unsigned)sizeof(cf);
  // the QN partial of this wave's pixels: one value per (position, wave)
  auto q_store = [&](float q, int n) {
    // row sums by DPP (no LDS round trips on the pass's critical
    // wave), then the four rows through readlane
    auto dpp = [](float x, auto ctl) {
      return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x),
                                                     decltype(ctl)::value, 0xf, 0xf,
                                                     false));
    };
    q += dpp(q, std::integral_constant<int, 0xb1>{});   // quad_perm [1,0,3,2]
    q += dpp(q, std::integral_constant<int, 0x4e>{});   // quad_perm [2,3,0,1]
    q += dpp(q, std::integral_constant<int, 0x141>{});  // row_half_mirror
    q += dpp(q, std::integral_constant<int, 0x140>{});  // row_mirror
    auto lane_q = [&](int l) {
      return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q), l));
    };
    q = (lane_q(0) + lane_q(16)) + (lane_q(32) + lane_q(48));
    if (lane == 0) qtab[(long)(slice * CW + cw) * nscan + n] = q;
  };
  if (EIG && HAVE_PROJ && probe.weights != nullptr && probe.eigen != nullptr) {
    const int total = probe.C * probe.Sm * RB * 64 * CW;
    for (int i = threadIdx.x; i < total; i += 256) {
      const int x = i % (64 * CW), yb = (i / (64 * CW)) % RB, cs = i / (64 * CW * RB);
      eigl[i] = conjf(probe.eigen[(long)cs * P + ya * N + yb * ROW + cb * CW * 64 + x]);
    }
  }
  __syncthreads();
  static_assert(MW > 1 || MPW == 1, "a lone mode-wave writes objproj straight from one mode");
  cf acc[MPW][RB];
  // conj(shared probe) at this thread's pixels
  cf Pc[HAVE_PROJ && HOIST ? MPW : 1][HAVE_PROJ && HOIST ? RB : 1];
#pragma unroll
  for (int m = 0; m < MPW; ++m) {
    const int s = mw + MW * m;
    const int sc = s < S ? s : S - 1;  // idle (wave, m): any valid mode, result unused
#pragma unroll
    for (int yb = 0; yb < RB; ++yb) {
      acc[m][yb] = mk(0.f, 0.f);
      if (HAVE_PROJ && HOIST)
        Pc[m][yb] = conjf(*tk_at(probe.probe + (long)sc * P + slice0 + yb * ROW, lb));
    }
  }
  // eigen probes vary the probe of the first Sm modes per position
  // (probe.py:272-303); only the waves that own those modes meet them
  const bool vary = HAVE_PROJ && probe.weights != nullptr;
  const int nE = (EIG && vary && probe.eigen != nullptr) ? probe.C : 0;
  for (int n = b0; n < b1; ++n) {
    // keep the per-lane offset out of the loop's induction variables: bases
    // stay in scalar registers, one 32-bit VGPR offset serves every access
    unsigned lo = lb;
    asm volatile("" : "+v"(lo));
    const cf* __restrict__ On = patches + (long)n * P + slice0;
    // with two modes per wave the patch values are re-read for the second
    // one (an L1/L2 hit) rather than held across both: 32 registers
    constexpr bool O_ONCE = HOIST && MPW == 1;
    cf O[HOIST ? RB : 1];
    if (O_ONCE) {
#pragma unroll
      for (int yb = 0; yb < RB; ++yb) O[yb] = *tk_at(On + yb * ROW, lo);
    }
    // this wave's slot, and slot 0 of its column block, for this position
    cf* slot = part + ((((n - b0) & (NBUF - 1)) * 4 + w) * RB) * 64 + lane;
    const cf* slots = part + ((((n - b0) & (NBUF - 1)) * 4 + cw * MW) * RB) * 64 + lane;
    const float* __restrict__ wn =
        vary ? probe.weights + n * (long)(probe.C + 1) * probe.S : nullptr;
#pragma unroll
    for (int m = 0; m < MPW; ++m) {
      const int s = mw + MW * m;
      if (s < S) {  // wave-uniform
        const cf* __restrict__ src = mid + ((long)n * Stot + s) * P + slice0;
        cf u[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) u[k] = tk_ld_stream(tk_at(src + k * ROW, lo));
        if (HOIST && !O_ONCE) {
#pragma unroll
          for (int yb = 0; yb < RB; ++yb) O[yb] = *tk_at(On + yb * ROW, lo);
        }
        const float w0 = vary ? wn[s] : 1.0f;
        // (poisson step lengths that became known after pass 1 was written:
        // a uniform factor per position and mode)
        const float sc = mode_scale ? inv_scale * mode_scale[(long)n * Stot + s] : inv_scale;
        Dft<RB, true>::run(u);
        if (HOIST) {
#pragma unroll
          for (int yb = 0; yb < RB; ++yb) {
            u[yb] = u[yb] * sc;  // chi of row ya + 16 yb
            acc[m][yb] = acc[m][yb] + conjf(O[yb]) * u[yb];
          }
          if (QN && !REDUCE && s == 0) {  // wave-uniform (with REDUCE: below)
            // eigl holds conj(E_0,0): Re(t conj(E)) = t.x el.x - t.y el.y
            const cf* __restrict__ el = eigl + cw * 64 + lane;
            float q = 0.f;
#pragma unroll
            for (int yb = 0; yb < RB; ++yb) {
              const cf t = conjf(O[yb]) * u[yb];
              const cf e = el[yb * (64 * CW)];
              q += t.x * e.x - t.y * e.y;
            }
            q_store(q, n);
          }
        } else {
#pragma unroll
          for (int g = 0; g < RB; g += 8) {
            cf o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = *tk_at(On + (g + i) * ROW, lo);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              u[g + i] = u[g + i] * sc;
              acc[m][g + i] = acc[m][g + i] + conjf(o[i]) * u[g + i];
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        if (s == 0 && chi0 != nullptr) {
#pragma unroll
          for (int yb = 0; yb < RB; ++yb)
            tk_st_stream(tk_at(chi0 + (long)n * P + slice0 + yb * ROW, lo), u[yb]);
        }
        if (HAVE_PROJ) {
          const cf* __restrict__ Ps = probe.probe + (long)s * P + slice0;
          const bool eig = EIG && nE > 0 && s < probe.Sm;  // wave-uniform, rare
#pragma unroll
          for (int g = 0; g < RB; g += 8) {
            cf pc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
              pc[i] = HOIST ? Pc[m][g + i] : conjf(*tk_at(Ps + (g + i) * ROW, lo));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              cf t = (pc[i] * u[g + i]) * w0;
              if (REDUCE) {
                // first mode of the wave fills its slot, later ones add to it
                // (a wave's LDS operations execute in order)
                slot[(g + i) * 64] = m == 0 ? t : slot[(g + i) * 64] + t;
              } else {
                // a lone mode-wave: the whole projection is this one product
                if (eig) {
#pragma unroll 1
                  for (int c = 0; c < nE; ++c)
                    t = t + (eigl[((c * probe.Sm + s) * RB + g + i) * (64 * CW) + cw * 64 + lane] *
                             u[g + i]) * wn[(c + 1) * probe.S + s];
                }
                tk_st_stream(tk_at(objproj + (long)n * P + slice0 + (g + i) * ROW, lo), t);
              }
            }
            if (!HOIST) __builtin_amdgcn_sched_barrier(0);
          }
          if (REDUCE && eig) {
            // + sum_c w_c conj(E_c,s) chi from the LDS-resident eigen slices
            // (only the waves owning the first Sm modes)
#pragma unroll 1
            for (int c = 0; c < nE; ++c) {
              const float wc = wn[(c + 1) * probe.S + s];
              const cf* __restrict__ el =
                  eigl + ((c * probe.Sm + s) * RB) * (64 * CW) + cw * 64 + lane;
              if (QN && c == 0 && s == 0) {  // wave-uniform: q_n from the same loads
                float q = 0.f;
#pragma unroll
                for (int yb = 0; yb < RB; ++yb) {
                  const cf e = el[yb * (64 * CW)];
                  slot[yb * 64] = slot[yb * 64] + (e * u[yb]) * wc;
                  const cf t = conjf(O[yb]) * u[yb];  // (el holds conj(E))
                  q += t.x * e.x - t.y * e.y;
                }
                q_store(q, n);
                continue;
              }
#pragma unroll
              for (int yb = 0; yb < RB; ++yb)
                slot[yb * 64] = slot[yb * 64] + (el[yb * (64 * CW)] * u[yb]) * wc;
            }
          }
        }
      } else if (REDUCE && m == 0) {
        // idle mode-wave (fewer modes than waves): an empty partial sum
#pragma unroll
        for (int yb = 0; yb < RB; ++yb) slot[yb * 64] = mk(0.f, 0.f);
      }
    }
    if (REDUCE) {
      __syncthreads();
      // mode-wave mw finishes rows yb = mw, mw + MW, ... of its column block
#pragma unroll
      for (int q = 0; q < RB / MW; ++q) {
        const int yb = mw + MW * q;
        cf sum = slots[yb * 64];
#pragma unroll
        for (int k = 1; k < MW; ++k) sum = sum + slots[(k * RB + yb) * 64];
        if (accumulate) sum = sum + *tk_at(objproj + (long)n * P + slice0 + yb * ROW, lo);
        tk_st_stream(tk_at(objproj + (long)n * P + slice0 + yb * ROW, lo), sum);
      }
      if (NBUF == 1) __syncthreads();  // the single slot set is rewritten next
    }
  }
  if (mpu != nullptr) {
#pragma unroll
    for (int m = 0; m < MPW; ++m) {
      const int s = mw + MW * m;
      if (s < S) {
#pragma unroll
        for (int yb = 0; yb < RB; ++yb) {
          if (mpu_part != nullptr) {
            // deterministic mode: this chunk's partial sum, added up in chunk
            // order by tk_ordered_sum after the launch
            const long ci = (nchunk_ - 1) - b0 / chunk;
            float* o = tk_at(mpu_part + 2 * ((ci * S + s) * P + slice0 + yb * ROW), lb);
            o[0] = acc[m][yb].x * mpu_scale;
            o[1] = acc[m][yb].y * mpu_scale;
          } else {
            float* o = tk_at(mpu + 2 * ((long)s * P + slice0 + yb * ROW), lb);
            unsafeAtomicAdd(o, acc[m][yb].x * mpu_scale);
            unsafeAtomicAdd(o + 1, acc[m][yb].y * mpu_scale);
          }
        }
      }
    }
  }
}

// work (nscan,S,det,det): output of tike_grad_ifft2_pass1 / tike_ifft2_pass1_scaled;
// patches (nscan,det,det): O_n from the forward kernel.  Outputs (each may be
// NULL): objproj (nscan,det,det), chi0 (nscan,det,det), m_probe_update
// (S,det,det, accumulated).  Probe window = detector; det in {128, 256, 512};
// S <= 8 (TIKE_ERR_UNSUPPORTED otherwise: use tike_ifft2_crop* +
// tike_lstsq_gradients).
// q_n of every position from the partials of the QN instantiation, in a fixed order
__global__ __launch_bounds__(256) void pass2_q_finish_kernel(const float* __restrict__ qtab,
                                                             int slots, int nscan,
                                                             float* __restrict__ q) {
  // one wave per position, lane k reads slot k (slots <= 64), a fixed tree
  const int n = blockIdx.x * 4 + (int)(threadIdx.x >> 6), k = threadIdx.x & 63;
  if (n >= nscan) return;  // wave-uniform
  float a = k < slots ? qtab[(long)k * nscan + n] : 0.f;
  a = tk_wave_sum(a);
  if (k == 0) q[n] = a;
}

// the QN instantiation of a (det, MW, MPW) launch (probe windows of 128 and
// 256: the patch values stay in registers there); false: not compiled
template <int N, int MW_, int MPW_>
static bool launch_pass2_qn(dim3 grid, size_t lds, hipStream_t stream, const cf* work,
                            const cf* patches, const TkProbe& pr, cf* objproj, cf* chi0,
                            float* mpu, float mpu_scale, int nscan, int S, float inv_scale,
                            int chunk, float* mpu_part, const float* mode_scale, float* qtab) {
  if constexpr (N <= 256) {
    hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, true, true, false, true>),
                       grid, dim3(256), lds, stream, work, patches, pr, objproj, chi0, mpu,
                       mpu_scale, nscan, S, inv_scale, chunk, mpu_part, mode_scale, 0, 0, qtab);
    return true;
  } else {
    return false;
  }
}

static int launch_pass2_gradients(const void* work, const void* patches, const void* probe,
                                  const void* eigen_probe, const float* eigen_weights,
                                  int num_eigen, int eigen_modes, void* objproj, void* chi0,
                                  void* m_probe_update, float mpu_scale, int nscan, int S,
                                  int det, float inv_scale, const float* mode_scale,
                                  hipStream_t stream, int Stot = 0, int accumulate = 0,
                                  float* qtab = nullptr, float* q = nullptr) {
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && det >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(work && patches && (probe || !objproj));
  if (S > 8 || (det != 128 && det != 256 && det != 512)) return TK_ERR_UNSUPPORTED;
  const bool qn = q != nullptr;
  TK_CHECK_ARG(!qn || qtab);
  if (qn && (Stot != 0 || det > 256 || !objproj || !eigen_probe || !eigen_weights ||
             num_eigen < 1 || eigen_modes < 1))
    return TK_ERR_UNSUPPORTED;
  // a group of S modes out of Stot (tike_ifft2_pass2_gradients_modes): the
  // weights are Stot apart, as the tiles
  const bool grp = Stot != 0;
  // (with objproj: through the mode-sum path, which needs two mode-waves)
  if (grp && objproj && S < 2) return TK_ERR_UNSUPPORTED;
  const TkProbe pr = tk_make_probe(probe, 0, eigen_probe, eigen_weights, num_eigen, eigen_modes,
                                   grp ? Stot : S, det);
  // mode-waves x column-waves of a workgroup and modes per wave
  int MW = S >= 3 ? 4 : S;
  if (det == 128 && MW == 1) MW = 2;  // a 128-wide tile has only two 64-column waves
  // eigen probes applied on the fly keep conj(E) of the workgroup's slice in LDS
  // (32 KiB at most: two workgroups per CU): a slice of 4 / MW column-waves --
  // with one or two modes at 512^2 (or several eigen probes) more mode-waves,
  // the spare ones idle, make it narrow enough
  auto eig_bytes = [&](int mw) {
    return sizeof(cf) * (size_t)num_eigen * eigen_modes * (det / 16) * 64 * (4 / mw);
  };
  if (objproj && eigen_weights && eigen_probe)
    while (MW < 4 && eig_bytes(MW) > 32 * 1024) MW *= 2;
  const int MPW = S > 4 ? 2 : 1;
  const int nslice = 16 * (det / (64 * (4 / MW)));
  // enough (slice, chunk) workgroups to fill the chip about twice -- and
  // in WHOLE rounds: the kernel holds two workgroups per CU (512 at a time) and
  // every workgroup walks the same number of positions, so 4.5 rounds cost 5
  int nchunk = (1024 + nslice - 1) / nslice;
  {
    int unit = 512, a = nslice;  // unit = 512 / gcd(512, nslice)
    while (a % 2 == 0 && unit > 1) { a /= 2; unit /= 2; }
    if (nchunk >= unit) nchunk = nchunk / unit * unit;
  }
  int chunk = (nscan + nchunk - 1) / nchunk;
  if (chunk < 8) chunk = 8;
  nchunk = (nscan + chunk - 1) / chunk;
  const dim3 grid((unsigned)(nslice * nchunk)), block(256);
  // deterministic mode: per-chunk partial sums of the probe gradient in the
  // caller's scratch buffer (one chunk when it is too small)
  float* mpu_part = nullptr;
  const long mpu_len = 2L * S * det * det;
  if (m_probe_update && tk_deterministic()) {
    mpu_part = tk_det_scratch(sizeof(float) * (size_t)mpu_len * nchunk);
    if (mpu_part == nullptr) return TK_ERR_ARG;
  }
  // LDS for the eigen-probe slices (only when they are applied on the fly)
  size_t eig_lds = 0;
  if (objproj && eigen_weights && eigen_probe) eig_lds = eig_bytes(MW);
  if (eig_lds > 32 * 1024) return TK_ERR_UNSUPPORTED;
#define TK_P2G(N, MW_, MPW_)                                                                 \
  do {                                                                                       \
    if (qn) {                                                                                \
      if (!launch_pass2_qn<N, MW_, MPW_>(grid, eig_lds, stream, (const cf*)work,             \
                                         (const cf*)patches, pr, (cf*)objproj, (cf*)chi0,    \
                                         (float*)m_probe_update, mpu_scale, nscan, S,        \
                                         inv_scale, chunk, mpu_part, mode_scale, qtab))      \
        return TK_ERR_UNSUPPORTED;                                                           \
    } else if (grp && !objproj)                                                              \
      hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, false, true, true>),    \
                         grid, block, 0,                                                     \
                         stream, (const cf*)work, (const cf*)patches, pr, (cf*)objproj,      \
                         (cf*)chi0, (float*)m_probe_update, mpu_scale, nscan, S, inv_scale,  \
                         chunk, mpu_part, mode_scale, Stot, accumulate);                     \
    else if (grp && eig_lds > 0)                                                             \
      hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, true, true, true>),     \
                         grid, block, eig_lds,                                               \
                         stream, (const cf*)work, (const cf*)patches, pr, (cf*)objproj,      \
                         (cf*)chi0, (float*)m_probe_update, mpu_scale, nscan, S, inv_scale,  \
                         chunk, mpu_part, mode_scale, Stot, accumulate);                     \
    else if (grp)                                                                            \
      hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, true, false, true>),    \
                         grid, block, 0,                                                     \
                         stream, (const cf*)work, (const cf*)patches, pr, (cf*)objproj,      \
                         (cf*)chi0, (float*)m_probe_update, mpu_scale, nscan, S, inv_scale,  \
                         chunk, mpu_part, mode_scale, Stot, accumulate);                     \
    else if (objproj && eig_lds > 0)                                                         \
      hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, true>), grid, block,    \
                         eig_lds,                                                            \
                         stream, (const cf*)work, (const cf*)patches, pr, (cf*)objproj,      \
                         (cf*)chi0, (float*)m_probe_update, mpu_scale, nscan, S, inv_scale,  \
                         chunk, mpu_part, mode_scale);                                       \
    else if (objproj)                                                                        \
      hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, true, false>), grid,    \
                         block, 0,                                                           \
                         stream, (const cf*)work, (const cf*)patches, pr, (cf*)objproj,      \
                         (cf*)chi0, (float*)m_probe_update, mpu_scale, nscan, S, inv_scale,  \
                         chunk, mpu_part, mode_scale);                                       \
    else                                                                                     \
      hipLaunchKernelGGL((ifft2_pass2_gradients_kernel<N, MW_, MPW_, false>), grid, block,   \
                         0, stream, (const cf*)work, (const cf*)patches, pr, (cf*)objproj,   \
                         (cf*)chi0, (float*)m_probe_update, mpu_scale, nscan, S, inv_scale,  \
                         chunk, mpu_part, mode_scale);                                       \
  } while (0)
#define TK_P2G_N(N)                     \
  do {                                  \
    if (MW == 1)                        \
      TK_P2G(N < 256 ? 256 : N, 1, 1);  \
    else if (MW == 2)                   \
      TK_P2G(N, 2, 1);                  \
    else if (MPW == 1)                  \
      TK_P2G(N, 4, 1);                  \
    else                                \
      TK_P2G(N, 4, 2);                  \
  } while (0)
  switch (det) {
    case 128: TK_P2G_N(128); break;
    case 256: TK_P2G_N(256); break;
    default: TK_P2G_N(512); break;
  }
#undef TK_P2G_N
#undef TK_P2G
  TK_LAUNCH_CHECK();
  if (qn) {
    hipLaunchKernelGGL(pass2_q_finish_kernel, dim3((nscan + 3) / 4), dim3(256), 0, stream,
                       qtab, det / 4, nscan, q);
    TK_LAUNCH_CHECK();
  }
  if (mpu_part != nullptr)
    return tk_ordered_sum((float*)m_probe_update, mpu_part, mpu_len, nchunk, true, stream);
  return TK_OK;
}

extern "C" int tike_ifft2_pass2_gradients(const void* work, const void* patches,
                                          const void* probe, const void* eigen_probe,
                                          const float* eigen_weights, int num_eigen,
                                          int eigen_modes, void* objproj, void* chi0,
                                          void* m_probe_update, float mpu_scale, int nscan,
                                          int S, int det, float inv_scale, void* stream) {
  TK_ENTER();
  return launch_pass2_gradients(work, patches, probe, eigen_probe, eigen_weights, num_eigen,
                                eigen_modes, objproj, chi0, m_probe_update, mpu_scale, nscan, S,
                                det, inv_scale, nullptr, (hipStream_t)stream);
}

// ... with chi_n,s also times mode_scale[n][s] (nscan,S): the poisson step
// lengths of tike_poisson_steps_grad_ifft2_pass1, known only after its pass 1
// was written.
extern "C" int tike_ifft2_pass2_gradients_scaled(const void* work, const void* patches,
                                                 const void* probe, const void* eigen_probe,
                                                 const float* eigen_weights, int num_eigen,
                                                 int eigen_modes, void* objproj, void* chi0,
                                                 void* m_probe_update, float mpu_scale,
                                                 int nscan, int S, int det, float inv_scale,
                                                 const float* mode_scale, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan == 0 || mode_scale != nullptr);
  return launch_pass2_gradients(work, patches, probe, eigen_probe, eigen_weights, num_eigen,
                                eigen_modes, objproj, chi0, m_probe_update, mpu_scale, nscan, S,
                                det, inv_scale, mode_scale, (hipStream_t)stream);
}

// tike_ifft2_pass2_gradients, and q[n] = sum_p Re(conj(O_n) chi_n,0 conj(E_0,0))
// from the same registers (the step statistics' eigen projection without the
// probe-update term; tike_eigen_pixel_update1q subtracts it).  qtab: scratch
// of nscan * det / 4 floats.
extern "C" int tike_ifft2_pass2_gradients_eproj(const void* work, const void* patches,
                                                const void* probe, const void* eigen_probe,
                                                const float* eigen_weights, int num_eigen,
                                                int eigen_modes, void* objproj, void* chi0,
                                                void* m_probe_update, float mpu_scale,
                                                int nscan, int S, int det, float inv_scale,
                                                float* qtab, float* q, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan == 0 || (qtab && q));
  return launch_pass2_gradients(work, patches, probe, eigen_probe, eigen_weights, num_eigen,
                                eigen_modes, objproj, chi0, m_probe_update, mpu_scale, nscan, S,
                                det, inv_scale, nullptr, (hipStream_t)stream, 0, 0, qtab, q);
}

// 1 where the eigen probes' LDS slices of tike_ifft2_pass2_gradients fit (32 KiB
// per workgroup at the widest mode-wave split); 0: the caller keeps chi
// (tike_ifft2_crop* + tike_lstsq_gradients).  No device work.
extern "C" int tike_ifft2_pass2_eigen_fits(int det, int num_eigen, int eigen_modes) {
  if (det < 16 || num_eigen < 0 || eigen_modes < 0) return 0;
  return sizeof(cf) * (size_t)num_eigen * eigen_modes * (det / 16) * 64 <= 32 * 1024 ? 1 : 0;
}

// Modes [mode0, mode0 + nmodes) of an S-mode problem (2 <= nmodes <= 8): what
// tike_ifft2_pass2_gradients does for those modes alone -- their probe
// gradients, mode 0 of chi when mode0 == 0 -- with their share of objproj
// stored (accumulate == 0: the first group) or added to what is there.  The
// caller walks the groups in order; eigen probes must all belong to the modes
// of the first group (eigen_modes <= its nmodes).
extern "C" int tike_ifft2_pass2_gradients_modes(const void* work, const void* patches,
                                                const void* probe, const void* eigen_probe,
                                                const float* eigen_weights, int num_eigen,
                                                int eigen_modes, void* objproj, void* chi0,
                                                void* m_probe_update, float mpu_scale,
                                                int nscan, int S, int det, float inv_scale,
                                                int mode0, int nmodes, int accumulate,
                                                void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(S >= 1 && det >= 1 && mode0 >= 0 && nmodes >= 1 && mode0 + nmodes <= S);
  TK_CHECK_ARG(nscan == 0 || (work && (probe || !objproj)));
  const long P = (long)det * det;
  const bool first = mode0 == 0;
  if (first ? eigen_modes > nmodes : false) return TK_ERR_UNSUPPORTED;
  return launch_pass2_gradients(
      (const cf*)work + mode0 * P, patches, probe ? (const cf*)probe + mode0 * P : nullptr,
      first ? eigen_probe : nullptr, eigen_weights ? eigen_weights + mode0 : nullptr,
      first ? num_eigen : (eigen_weights ? num_eigen : 0), first ? eigen_modes : 0, objproj,
      first ? chi0 : nullptr,
      m_probe_update ? (void*)((float*)m_probe_update + 2 * mode0 * P) : nullptr, mpu_scale,
      nscan, nmodes, det, inv_scale, nullptr, (hipStream_t)stream, S, accumulate);
}

// The probe preconditioner with RW vertically adjacent pixels per thread: the
// RW + 1 tap rows of a position are loaded once (1.25 16-byte loads per pixel
// and position instead of 2; the sum is bound by its L1 requests).  Thread
// groups of cols = min(pw, 256) columns, 256 / cols groups stacked over the
// rows; grid.x = row blocks x column blocks, grid.y = position chunks.
template <int RW>
__global__ __launch_bounds__(256) void probe_precond_rows_kernel(
    const float* __restrict__ scan, const cf* __restrict__ psi, float* __restrict__ out,
    int nscan, int pw, int H, int W, int chunk, float* __restrict__ part) {
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const long P = (long)pw * pw;
  const long total = (long)H * W;
  const int cols = pw < 256 ? pw : 256, ncb = pw / cols;
  const int x = ((int)blockIdx.x % ncb) * cols + (int)threadIdx.x % cols;
  const int y0 = (((int)blockIdx.x / ncb) * (256 / cols) + (int)threadIdx.x / cols) * RW;
  const int b0 = blockIdx.y * chunk;
  const int b1 = min(nscan, b0 + chunk);
  float acc[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) acc[r] = 0.f;
  bool inside = true;  // every position of the chunk interior (decided once)
  for (int b = b0; b < b1; ++b) {
    const TkCorner c = tk_corner(scan, b);
    inside = inside && c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W;
  }
  if (inside) {
    const unsigned row_bytes = (unsigned)W * (unsigned)sizeof(cf);
    const unsigned lane_off = (unsigned)y0 * row_bytes + (unsigned)x * (unsigned)sizeof(cf);
#pragma unroll 2
    for (int b = b0; b < b1; ++b) {
      const TkCorner c = tk_corner(scan, b);  // uniform
      const unsigned off = (unsigned)(c.sy * W + c.sx) * (unsigned)sizeof(cf) + lane_off;
      tk_v4f t[RW + 1];
#pragma unroll
      for (int r = 0; r <= RW; ++r)
        __builtin_memcpy(&t[r], reinterpret_cast<const char*>(psi) + off + (unsigned)r * row_bytes,
                         sizeof(tk_v4f));
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        cf o = mk(t[r].x * c.w00, t[r].y * c.w00);  // the order of tk_patch_pixel
        o.x += t[r].z * c.w01;
        o.y += t[r].w * c.w01;
        o.x += t[r + 1].x * c.w10;
        o.y += t[r + 1].y * c.w10;
        o.x += t[r + 1].z * c.w11;
        o.y += t[r + 1].w * c.w11;
        acc[r] += norm2(o);
      }
    }
  } else {
    for (int b = b0; b < b1; ++b) {
      const TkCorner c = tk_corner(scan, b);
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int y = c.sy + y0 + r, xx = c.sx + x;
        const bool ok = y >= 0 && y < H && xx >= 0 && xx < W;
        const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
        const int xc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
        const cf o = tk_gather(psi, (long)yc * W + xc, W, total, c);
        acc[r] += ok ? norm2(o) : 0.f;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const long p = (long)(y0 + r) * pw + x;
    if (part != nullptr)
      part[(long)blockIdx.y * P + p] = acc[r];
    else
      unsafeAtomicAdd(&out[2 * p], acc[r]);
  }
}

// probe preconditioner: out (pw,pw) complex (imaginary part untouched) +=
// sum_n |patch_n(psi)|^2   (_preconditioner.py:136-144)
extern "C" int tike_probe_preconditioner(const float* scan, const void* psi, void* out,
                                         int nscan, int pw, int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(scan && psi && out);
  const long P = (long)pw * pw;
  float* part = nullptr;
  const int chunk = probe_chunk(nscan, P, &part);
  dim3 grid((unsigned)((P + 255) / 256), (unsigned)((nscan + chunk - 1) / chunk));
  constexpr int RW = 4;
  const int cols = pw < 256 ? pw : 256;
  if (g_stats_pairs && (pw % 256 == 0 || 256 % pw == 0) && pw % ((256 / cols) * RW) == 0 &&
      (long)H * W < (1L << 28)) {
    grid.x = (unsigned)(P / (256 * RW));
    hipLaunchKernelGGL(probe_precond_rows_kernel<RW>, grid, dim3(256), 0, (hipStream_t)stream,
                       scan, (const cf*)psi, (float*)out, nscan, pw, H, W, chunk, part);
  } else {
    launch_probe_grad<false>(grid, (hipStream_t)stream, (const cf*)nullptr, scan,
                             (const cf*)psi, (cf*)nullptr, (float*)out,
                             tk_make_probe(psi, 0, nullptr, nullptr, 0, 0, 1, pw),
                             (cf*)nullptr, nscan, 1, pw, H, W, chunk, part);
  }
  TK_LAUNCH_CHECK();
  if (part != nullptr)  // (the real parts of `out`)
    return tk_ordered_sum((float*)out, part, P, (int)grid.y, true, (hipStream_t)stream, 2);
  return TK_OK;
}
