// The backward of the differentiable intensity model (tike_amd/autograd.py)
// with a varying probe (reference probe.py:272-303, get_varying_probe):
//   P[n,s] = w[n,0,s] probe[s] + sum_c w[n,c+1,s] eigen[c,s]   (s < M; the
//            shared term alone for s >= M)
// No reference counterpart: the reference updates eigen probes and weights by
// a heuristic (lstsq.py) and has no gradient with respect to either.
//
//   tike_eigen_probe_gradients, with q[n,s] = conj(patch_n(psi)) chi[n,s]:
//     probe_grad[s]        += sum_n w[n,0,s]   q[n,s]
//     eigen_grad[c,s]      += sum_n w[n,c+1,s] q[n,s]                 s < M
//     weights_grad[n,0,s]   = sum_px Re(conj(probe[s])   q[n,s])
//     weights_grad[n,c+1,s] = sum_px Re(conj(eigen[c,s]) q[n,s])      s < M, else 0
//     objproj[n]            = sum_s conj(P[n,s]) chi[n,s]
//
// Byte model, per position: S * pw^2 * 8 bytes of chi read ONCE for all four
// outputs, pw^2 * 8 bytes of objproj written once, (pw + 1)^2 * 8 bytes of
// object (mostly from cache: neighbouring footprints overlap), (C + 1) * S * 4
// bytes of weights (scalar loads), ntile * (S + C M) * 8 bytes of partial
// weight sums written and read back once (ntile = ceil(pw^2 / 256)).  Per
// chunk of positions: (S + C M) * pw^2 * 8 bytes of probe and eigen probes
// read once and as many bytes of float atomics; the chunk holds at least
// 64 (S + C M) / S positions, so the atomic bytes stay below 1/64 of the
// chunk's chi bytes (the chip-wide float-atomic rate is about a sixth of the
// streaming rate: a tenth of the kernel's time at most).
#include "internal.h"
#include "tike_amd.h"

namespace {

constexpr int EG_MAX_MODES = 16;   // S
constexpr int EG_MAX_PLANES = 16;  // C * M
constexpr int EG_BATCH = 8;        // positions whose wave sums share a trip through LDS

// The bilinear gather of tk_gather (common.h) in two halves, so that the taps
// can be in flight while other work goes on: the same clamped addresses, the
// same weights -- exactly zero for a tap behind the allocation -- and the same
// order of the products; a pixel outside the object counts as zero.
// (What waits with the taps is kept small: the four weights are uniform in a
// workgroup -- scalar registers --, the per-lane part is four flags.)
struct EgTaps {
  cf a, b, d, e;
  float w00, w01, w10, w11;  // uniform: of the position
  bool in1, in2, in3, ok;    // taps inside the allocation; pixel inside the object
};

__device__ __forceinline__ EgTaps eg_taps(const cf* __restrict__ psi,
                                          const float* __restrict__ scan, long n, int py, int px,
                                          int H, int W, long total) {
  const TkCorner c = tk_corner(scan, n);
  const int y = c.sy + py, x = c.sx + px;
  const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
  const int xc = x < 0 ? 0 : (x >= W ? W - 1 : x);
  const long ii = (long)yc * W + xc, last = total - 1;
  const long i1 = ii + 1 <= last ? ii + 1 : last;
  const long i2 = ii + W <= last ? ii + W : last;
  const long i3 = ii + W + 1 <= last ? ii + W + 1 : last;
  EgTaps t;
  t.ok = y >= 0 && y < H && x >= 0 && x < W;
  t.w00 = c.w00, t.w01 = c.w01, t.w10 = c.w10, t.w11 = c.w11;
  t.in1 = ii + 1 <= last, t.in2 = ii + W <= last, t.in3 = ii + W + 1 <= last;
  t.a = psi[ii], t.b = psi[i1], t.d = psi[i2], t.e = psi[i3];
  return t;
}

__device__ __forceinline__ cf eg_patch(const EgTaps& t) {
  const float w1 = t.in1 ? t.w01 : 0.0f, w2 = t.in2 ? t.w10 : 0.0f, w3 = t.in3 ? t.w11 : 0.0f;
  cf r = mk(t.a.x * t.w00, t.a.y * t.w00);
  r.x += t.b.x * w1;
  r.y += t.b.y * w1;
  r.x += t.d.x * w2;
  r.y += t.d.y * w2;
  r.x += t.e.x * w3;
  r.y += t.e.y * w3;
  return t.ok ? r : mk(0.f, 0.f);
}

// The exchanges of the first two steps below without a trip through the LDS
// crossbar and without selects (gfx950): v_permlane32_swap exchanges lanes
// 32-63 of `a` with lanes 0-31 of `b`, v_permlane16_swap the odd rows of 16
// lanes of `a` with the even rows of `b`.  Afterwards a + b is, in the lower
// half (the even rows), the sum of what both partners held in `a`, and in the
// upper half (the odd rows) the sum of what they held in `b`.
__device__ __forceinline__ void eg_swap32(unsigned& a, unsigned& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0], b = r[1];
}
__device__ __forceinline__ void eg_swap16(unsigned& a, unsigned& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  a = r[0], b = r[1];
}

// The sums over the 64 lanes of V values at once (1 <= V <= 32), in float64:
// at every step a lane hands over the half of its values that its partner
// keeps -- of A values the lane with the lower number keeps the first
// H = ceil(A / 2), its partner WIDTH lanes up the other A - H (and a zero for
// an odd A) -- so the steps move ceil(V/2), ceil(V/4), ... 1, 1 ... values
// instead of V values six times.  The first step hands over the float32 terms
// themselves (their conversion to float64 is exact either side of the
// exchange).  The order of the additions is fixed.  eg_holder says which
// value's sum a lane is left with.
// (the steps behind the first: a template recursion, so that every register
// index is a constant)
template <int A, int WIDTH, int VH>
__device__ __forceinline__ double eg_halve(double (&v)[VH], int lane) {
  if constexpr (A > 1) {
    constexpr int H = (A + 1) / 2;
    const bool upper = (lane & WIDTH) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const double a = v[i], b = i + H < A ? v[i + H] : 0.0;
      if constexpr (WIDTH == 16) {
        unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
        unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
        eg_swap16(alo, blo);
        eg_swap16(ahi, bhi);
        v[i] = __hiloint2double((int)ahi, (int)alo) + __hiloint2double((int)bhi, (int)blo);
      } else {
        const double send = upper ? a : b, keep = upper ? b : a;
        v[i] = keep + __shfl_xor(send, WIDTH, 64);
      }
    }
    return eg_halve<H, WIDTH / 2>(v, lane);
  } else if constexpr (WIDTH > 0) {
    v[0] += __shfl_xor(v[0], WIDTH, 64);
    return eg_halve<1, WIDTH / 2>(v, lane);
  } else {
    return v[0];
  }
}

template <int V>
__device__ __forceinline__ double eg_wave_sums(const float (&t)[V], int lane) {
  static_assert(V >= 1 && V <= 32, "at most the halving steps there are");
  constexpr int H = (V + 1) / 2;
  double v[H];
  if constexpr (V == 1) {
    v[0] = (double)t[0];
    return eg_halve<1, 32>(v, lane);
  } else {
#pragma unroll
    for (int i = 0; i < H; ++i) {
      unsigned a = __float_as_uint(t[i]), b = i + H < V ? __float_as_uint(t[i + H]) : 0u;
      eg_swap32(a, b);
      v[i] = (double)__uint_as_float(a) + (double)__uint_as_float(b);
    }
    return eg_halve<H, 16>(v, lane);
  }
}

// The value (0 ... V - 1) whose sum eg_wave_sums<V> leaves in this lane, for
// the one lane that writes it; -1 for every other lane.
template <int V>
__device__ __forceinline__ int eg_holder(int lane) {
  int A = V, n = V, idx = 0, width = 32;  // A: values of a step; n: this lane's real ones
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (A > 1) {
      const int H = (A + 1) / 2;
      if (lane & width) {
        idx += H;
        n = n > H ? n - H : 0;
      } else {
        n = n < H ? n : H;
      }
      A = H;
      width >>= 1;
    }
  return n == 1 && (lane & (2 * width - 1)) == 0 ? idx : -1;
}

// One thread per probe pixel, a workgroup (pixel tile = 256 pixels) walks a
// chunk of positions.  The pixel's probe[s] and eigen[c][s] stay in registers
// over the chunk: they are the left factors of the weight sums, they
// synthesise P[n,s] for objproj, and their plane sums accumulate next to them
// in float32, one atomic pair per (pixel, plane, chunk) -- or, deterministic
// mode, one store to the chunk's row of `ppart` / `epart`, added in chunk
// order after the launch (tk_ordered_sum), as probe_grad_kernel has it.
//
// Eigen plane j = c * M + m belongs to mode m.  SC > 0: S = SC at compile
// time and EC = 0 (no eigen probe) or 1 (C = M = 1: one eigen probe on mode
// 0, which takes chi from the register the mode loop loaded), no branch in
// the plane loops -- the rule of probe_grad_kernel<SC>, S = 1 ... 6 and 8.
// Otherwise the general kernels, SC = 0: S and C M at run time, at most SB
// and EB = 4, 8 or 16 (the loops are unrolled to the bounds and predicated,
// the registers are those of the bounds); a plane
// loads chi of its mode again -- the line the same lane loaded a few
// instructions earlier, served from cache -- because a register cannot be
// indexed by m.
//
// Weight sums: a term Re(conj(B) q) is float32; it is summed in float64 over
// the 64 lanes (shuffles: all values of a position in one halving butterfly,
// eg_wave_sums -- S + C M values when the counts are known at compile time,
// SB + EB slots with zeros in the unused ones while SB + EB <= 12; value by
// value above, where there are no registers to spare), the four
// waves (LDS, EG_BATCH positions per barrier pair) and left in
// work[tile][n][v], v < S the shared planes, S + j eigen plane j;
// eigen_weights_finish_kernel adds the tiles in ascending order.  No atomics:
// the same bits on every run.
//
// The patch: the gather of probe_grad_kernel (clamped address, selected
// value; a pixel outside the object counts as zero).  Lanes behind the last
// pixel of the last tile run along on pixel P - 1 with zero left factors (they
// take part in the barriers and the shuffles) and write nothing.
template <int SC, int EC, int SB, int EB>
__global__ __launch_bounds__(256, SC > 0 ? 3 : 1) void eigen_grad_kernel(
    const cf* __restrict__ chi, const float* __restrict__ scan, const cf* __restrict__ psi,
    const cf* __restrict__ probe, const cf* __restrict__ eigen,
    const float* __restrict__ weights, float* __restrict__ pgrad, float* __restrict__ egrad,
    double* __restrict__ work, cf* __restrict__ objproj, long nscan, int S_rt, int C, int M_rt,
    int pw, int H, int W, int chunk, float* __restrict__ ppart, float* __restrict__ epart) {
  static_assert(SC > 0 || (SB >= 1 && SB <= EG_MAX_MODES && EB >= 1 && EB <= EG_MAX_PLANES),
                "general: S <= SB, C M <= EB");
  constexpr int SM = SC > 0 ? SC : SB;
  constexpr int EM = SC > 0 ? EC : EB;
  constexpr int EA = EM > 0 ? EM : 1;
  // one butterfly over the slots [0, SM) of the modes and [SM, SM + EM) of the
  // eigen planes; the look-ahead of a position goes with it
  constexpr bool BUTTERFLY = SC > 0 || SB + EB <= 12;
  constexpr int VC = BUTTERFLY ? SM + EM : 1;
  const int S = SC > 0 ? SC : S_rt;
  static_assert(SC == 0 || EC <= 1, "specialised: at most one eigen plane, on mode 0");
  const int M = SC > 0 ? EC : M_rt;
  const int E = SC > 0 ? EC : C * M_rt;
  const int V = S + E;
  const long R = C + 1;
  const long P = (long)pw * pw;
  const long total = (long)H * W;
  __shared__ double red[4][EG_BATCH][SM + EA];
  const long p_raw = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = p_raw < P;
  const long p = live ? p_raw : P - 1;
  const int py = (int)(p / pw), px = (int)(p % pw);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long b0 = (long)blockIdx.y * chunk;
  const long b1 = b0 + chunk < nscan ? b0 + chunk : nscan;
  const bool sums = work != nullptr;
  // the sum this lane writes: slot -> v (S + j for eigen plane j), -1: none
  int mine = -1;
  if (BUTTERFLY) {
    const int slot_mine = eg_holder<VC>(lane);
    if (slot_mine >= 0 && slot_mine < SM)
      mine = slot_mine < S ? slot_mine : -1;
    else if (slot_mine >= SM)
      mine = slot_mine - SM < E ? S + slot_mine - SM : -1;
  }

  cf pr[SM], acc[SM], ei[EA], eacc[EA];
#pragma unroll
  for (int s = 0; s < SM; ++s) {
    acc[s] = mk(0.f, 0.f);
    pr[s] = mk(0.f, 0.f);
    if (SC > 0 || s < S) {
      const cf v = probe[s * P + p];
      pr[s] = live ? v : mk(0.f, 0.f);
    }
  }
#pragma unroll
  for (int j = 0; j < EA; ++j) {
    eacc[j] = mk(0.f, 0.f);
    ei[j] = mk(0.f, 0.f);
    if (EM > 0 && (SC > 0 || j < E)) {
      const cf v = eigen[j * P + p];
      ei[j] = live ? v : mk(0.f, 0.f);
    }
  }

  // The loads of position b + 1 (chi and the four taps of the patch) are
  // issued before the arithmetic and the cross-lane sums of position b, which
  // are a long dependent chain with nothing else to hide a memory latency
  // behind.  (The larger general kernels have no registers for a second set.)
  constexpr bool AHEAD = BUTTERFLY;
  EgTaps taps;
  cf xs[SM];
  if (AHEAD) {
    taps = eg_taps(psi, scan, b0, py, px, H, W, total);
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (SC > 0 || s < S) xs[s] = tk_ld_stream(chi + b0 * S * P + p + s * P);
  }
  for (long b = b0; b < b1; ++b) {
    const int slot = (int)((b - b0) % EG_BATCH);
    const cf* __restrict__ X = chi + b * S * P + p;
    EgTaps taps_next;
    cf xn[SM];
    if (AHEAD) {
      const long bn = b + 1 < b1 ? b + 1 : b;  // (the last position: itself again, from cache)
      taps_next = eg_taps(psi, scan, bn, py, px, H, W, total);
#pragma unroll
      for (int s = 0; s < SM; ++s)
        if (SC > 0 || s < S) xn[s] = tk_ld_stream(chi + bn * S * P + p + s * P);
    } else {
      taps = eg_taps(psi, scan, b, py, px, H, W, total);
#pragma unroll
      for (int s = 0; s < SM; ++s)
        if (s < S) xs[s] = tk_ld_stream(X + s * P);
    }
    const cf oc = conjf(eg_patch(taps));
    const float* __restrict__ w = weights + b * R * S;  // uniform: scalar loads
    cf proj = mk(0.f, 0.f);
    float tt[VC];  // the terms of the weight sums, by slot
#pragma unroll
    for (int v = 0; v < VC; ++v) tt[v] = 0.f;
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (SC > 0 || s < S) {
        const cf q = oc * xs[s];
        const float w0 = w[s];
        acc[s].x += w0 * q.x;
        acc[s].y += w0 * q.y;
        proj = proj + conjf(pr[s] * w0) * xs[s];
        const float t = pr[s].x * q.x + pr[s].y * q.y;  // Re(conj(probe) q)
        if constexpr (BUTTERFLY) {
          tt[s] = t;
        } else if (sums) {
          const double ts = tk_wave_sum((double)t);
          if (lane == 0) red[wave][slot][s] = ts;
        }
      }
    if (EM > 0) {
      int m = 0, r = 1;  // mode and weight row of plane j (general kernel)
#pragma unroll
      for (int j = 0; j < EA; ++j)
        if (SC > 0 || j < E) {
          cf xm;
          int mj, rj;
          if (SC > 0) {  // the one plane: eigen probe 0 on mode 0
            mj = 0, rj = 1;
            xm = xs[0];
          } else {
            mj = m, rj = r;
            xm = X[m * P];
            if (++m == M) m = 0, ++r;
          }
          const cf q = oc * xm;
          const float wj = w[rj * S + mj];
          eacc[j].x += wj * q.x;
          eacc[j].y += wj * q.y;
          proj = proj + conjf(ei[j] * wj) * xm;
          const float t = ei[j].x * q.x + ei[j].y * q.y;  // Re(conj(eigen) q)
          if constexpr (BUTTERFLY) {
            tt[SM + j] = t;
          } else if (sums) {
            const double ts = tk_wave_sum((double)t);
            if (lane == 0) red[wave][slot][S + j] = ts;
          }
        }
    }
    if (BUTTERFLY && sums) {
      const double ts = eg_wave_sums<VC>(tt, lane);
      if (mine >= 0) red[wave][slot][mine] = ts;
    }
    if (objproj != nullptr && live) tk_st_stream(objproj + b * P + p, proj);
    if (sums && (slot == EG_BATCH - 1 || b == b1 - 1)) {  // uniform
      __syncthreads();
      const int i = threadIdx.x;
      if (i < (slot + 1) * V) {
        const int k = i / V, v = i % V;
        const double t = (red[0][k][v] + red[1][k][v]) + (red[2][k][v] + red[3][k][v]);
        work[((long)blockIdx.x * nscan + (b - slot + k)) * V + v] = t;
      }
      __syncthreads();
    }
    if (AHEAD) {
      taps = taps_next;
#pragma unroll
      for (int s = 0; s < SM; ++s)
        if (SC > 0 || s < S) xs[s] = xn[s];
    }
  }

  if (!live) return;
  if (pgrad != nullptr) {
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (SC > 0 || s < S) {
        if (ppart != nullptr) {
          float* o = ppart + 2 * (((long)blockIdx.y * S + s) * P + p);
          o[0] = acc[s].x;
          o[1] = acc[s].y;
        } else {
          unsafeAtomicAdd(&pgrad[2 * (s * P + p)], acc[s].x);
          unsafeAtomicAdd(&pgrad[2 * (s * P + p) + 1], acc[s].y);
        }
      }
  }
  if (EM > 0 && egrad != nullptr) {
#pragma unroll
    for (int j = 0; j < EA; ++j)
      if (SC > 0 || j < E) {
        if (epart != nullptr) {
          float* o = epart + 2 * (((long)blockIdx.y * E + j) * P + p);
          o[0] = eacc[j].x;
          o[1] = eacc[j].y;
        } else {
          unsafeAtomicAdd(&egrad[2 * (j * P + p)], eacc[j].x);
          unsafeAtomicAdd(&egrad[2 * (j * P + p) + 1], eacc[j].y);
        }
      }
  }
}

// weights_grad[n][r][s] = sum_tile work[tile][n][v(r, s)], tiles ascending,
// rounded to float32 once; exactly 0 where mode s has no eigen probe.
__global__ __launch_bounds__(256) void eigen_weights_finish_kernel(
    const double* __restrict__ work, float* __restrict__ wgrad, long nscan, int S, int C, int M,
    long ntile) {
  const long R = C + 1, V = S + (long)C * M;
  const long count = nscan * R * S;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += gridDim.x * 256L) {
    const long n = i / (R * S);
    const int r = (int)(i / S % R), s = (int)(i % S);
    double t = 0.;
    if (r == 0 || s < M) {
      const long v = r == 0 ? s : S + (long)(r - 1) * M + s;
      const double* __restrict__ at = work + n * V + v;
      const long step = nscan * V;
      long tile = 0;
      for (; tile + 8 <= ntile; tile += 8) {  // eight loads in flight, added in order
        double x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = at[(tile + k) * step];
#pragma unroll
        for (int k = 0; k < 8; ++k) t += x[k];
      }
      for (; tile < ntile; ++tile) t += at[tile * step];
    }
    wgrad[i] = (float)t;
  }
}

}  // namespace

extern "C" int tike_eigen_probe_gradients(const void* chi, const float* scan, const void* psi,
                                          const void* probe, const void* eigen_probe,
                                          const float* eigen_weights, int num_eigen,
                                          int eigen_modes, void* probe_grad, void* eigen_grad,
                                          float* weights_grad, void* objproj, void* work,
                                          long nscan, int S, int pw, int H, int W,
                                          void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && H >= 1 && W >= 1);
  TK_CHECK_ARG(num_eigen >= 0 && eigen_modes >= 0);
  const int C = num_eigen, M = num_eigen > 0 ? eigen_modes : 0;
  if (S > EG_MAX_MODES || (long)C * M > EG_MAX_PLANES) return TK_ERR_UNSUPPORTED;
  TK_CHECK_ARG(C == 0 || (M >= 1 && M <= S && eigen_probe != nullptr));
  const int E = C * M;
  if (E == 0) eigen_grad = nullptr;  // no plane to add to
  if (nscan == 0 || (!probe_grad && !eigen_grad && !weights_grad && !objproj)) return TK_OK;
  TK_CHECK_ARG(chi && scan && psi && probe && eigen_weights);
  TK_CHECK_ARG(!weights_grad || work);
  const long P = (long)pw * pw;
  const long ntile = (P + 255) / 256;
  TK_CHECK_ARG(ntile <= 0x7fffffffL);  TK_GRID_Y_LIMIT(max_y);

  // Positions per chunk: at least 64 (S + E) / S, so that the atomics stay
  // below 1/64 of the chunk's chi bytes, and no fewer than leave about eight
  // workgroups per CU; whole batches of the weight sums.
  const long per_bytes = (64L * (S + E) + S - 1) / S;
  const long columns = ntile < 2048 ? 2048 / ntile : 1;  // chunks at 8 workgroups per CU
  long chunk = (nscan + columns - 1) / columns;
  chunk = chunk < per_bytes ? per_bytes : chunk;
  chunk = (chunk + EG_BATCH - 1) / EG_BATCH * EG_BATCH;
  long nchunk = (nscan + chunk - 1) / chunk;
  float *ppart = nullptr, *epart = nullptr;
  if (tk_deterministic() && (probe_grad || eigen_grad)) {
    const long plen = probe_grad ? 2 * S * P : 0, elen = eigen_grad ? 2 * E * P : 0;
    float* part = tk_det_scratch(sizeof(float) * (size_t)(plen + elen) * nchunk);
    if (part == nullptr) {
      // the scratch buffer cannot hold the chunks' rows: ONE chunk, whose single
      // atomic per address only adds to what earlier launches left there
      chunk = (nscan + EG_BATCH - 1) / EG_BATCH * EG_BATCH;
      nchunk = 1;
    } else {
      if (probe_grad) ppart = part;
      if (eigen_grad) epart = part + plen * nchunk;
    }
  }
  TK_CHECK_ARG(nchunk <= max_y && chunk <= 0x7fffffffL);

  dim3 grid((unsigned)ntile, (unsigned)nchunk);
  double* wk = weights_grad ? (double*)work : nullptr;
#define TK_EG(SC, EC, SB, EB)                                                                  \
  hipLaunchKernelGGL((eigen_grad_kernel<SC, EC, SB, EB>), grid, dim3(256), 0, stream,          \
                     (const cf*)chi, scan, (const cf*)psi, (const cf*)probe,                   \
                     (const cf*)eigen_probe, eigen_weights, (float*)probe_grad,                \
                     (float*)eigen_grad, wk, (cf*)objproj, nscan, S, C, M, pw, H, W,           \
                     (int)chunk, ppart, epart)
#define TK_EG_S(SC)        \
  do {                     \
    if (E == 0)            \
      TK_EG(SC, 0, 0, 0);  \
    else                   \
      TK_EG(SC, 1, 0, 0);  \
  } while (0)
#define TK_EG_B(SB)        \
  do {                     \
    if (E <= 4)            \
      TK_EG(0, 0, SB, 4);  \
    else if (E <= 8)       \
      TK_EG(0, 0, SB, 8);  \
    else                   \
      TK_EG(0, 0, SB, 16); \
  } while (0)
  // The mode counts of probe_grad_kernel<SC>, without an eigen probe or with
  // ONE on mode 0 (C = M = 1); everything else: the general kernel of the
  // smallest bounds (4, 8, 16) that hold S and C M.
  switch (E == 0 || (C == 1 && M == 1) ? S : 0) {
    case 1: TK_EG_S(1); break;
    case 2: TK_EG_S(2); break;
    case 3: TK_EG_S(3); break;
    case 4: TK_EG_S(4); break;
    case 5: TK_EG_S(5); break;
    case 6: TK_EG_S(6); break;
    case 8: TK_EG_S(8); break;
    default:
      if (S <= 4)
        TK_EG_B(4);
      else if (S <= 8)
        TK_EG_B(8);
      else
        TK_EG_B(16);
      break;
  }
#undef TK_EG_B
#undef TK_EG_S
#undef TK_EG
  TK_LAUNCH_CHECK();
  if (weights_grad) {
    const long count = nscan * (C + 1) * S;
    hipLaunchKernelGGL(eigen_weights_finish_kernel, dim3(tk_grid((count + 255) / 256, 8)),
                       dim3(256), 0, stream, (const double*)work, weights_grad, nscan, S, C, M,
                       ntile);
    TK_LAUNCH_CHECK();
  }
  if (ppart != nullptr) {
    int rc = tk_ordered_sum((float*)probe_grad, ppart, 2 * S * P, (int)nchunk, true, stream);
    if (rc != TK_OK) return rc;
  }
  if (epart != nullptr)
    return tk_ordered_sum((float*)eigen_grad, epart, 2 * E * P, (int)nchunk, true, stream);
  return TK_OK;
}
