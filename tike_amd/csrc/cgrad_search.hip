// The conjugate-gradient solver's search on the device (solvers/cgrad.py),
// for gfx950: no host round trip per trial.
//   tike_cgrad_direction the Dai-Yuan direction (reference opt.py:281-301);
//   tike_cgrad_line_search{,_masked}
//                        backtracking line search (opt.py:216-278), a cost-only
//                        forward pass per trial, enqueued ahead of the decisions;
//   tike_cgrad_line_search_linear{,_masked}
//                        the same search, every step length from ONE column
//                        pass over two hand-offs.
#include "fft_engine2.h"
#include "internal.h"
#include "tike_amd.h"
#include "ptycho_shared.h"

// ------------------------------------------- line search decided on the device
// Backtracking line search of the conjugate-gradient solver (reference
// opt.py:216-278 line_search, as composed by solvers/cgrad.py): try
// x + step d, x + step/2 d, ... until the gaussian cost of the minibatch is no
// larger than at x.  Every trial is a cost-only forward pass; its launches are
// enqueued for `nslots` step lengths AHEAD of the decisions, and a trial whose
// predecessor was accepted returns at once (the `skip` word the kernels read):
// no host round trip per trial.
// state (device, double[5]): { fx = mean cost at x, step, done, trials, failures }.
//   in : fx, step (first step length to try)
//   out: accepted -> fx = mean cost there, step = that step length, done = 1
//        otherwise  step = the next step length to try (step / 2^nslots), done = 0,
//        failures += 1 (a caller that chains searches reads it once at the end)
// xs receives x + step d of the LAST trial made (accepted: the new iterate).
__global__ __launch_bounds__(256) void ls_trial_kernel(const cf* __restrict__ x,
                                                       const cf* __restrict__ d,
                                                       cf* __restrict__ xs, long n,
                                                       const double* __restrict__ state,
                                                       float shrink,
                                                       const int* __restrict__ skip) {
  if (*skip != 0) return;
  const float a = (float)state[1] * shrink;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const cf v = d[i];
    xs[i] = mk(x[i].x + a * v.x, x[i].y + a * v.y);
  }
}

// One workgroup: mean cost of the trial; accept if it is no larger than fx.
__global__ __launch_bounds__(256) void ls_decide_kernel(const float* __restrict__ costs, int n,
                                                        double inv_count, float shrink,
                                                        int last, double* __restrict__ state,
                                                        int* __restrict__ skip) {
  if (*skip != 0) return;
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)costs[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double f = red[0] * inv_count;
    state[3] += 1.0;
    if (f <= state[0]) {
      state[0] = f;
      state[1] = (double)((float)state[1] * shrink);
      state[2] = 1.0;
      *skip = 1;
    } else if (last) {
      state[1] = (double)((float)state[1] * shrink * 0.5f);
      state[4] += 1.0;
    }
  }
}

// ------------------------------------------- conjugate direction on the device
// Dai-Yuan direction of the conjugate-gradient solver (reference opt.py:281-301
// direction_dy as solvers/cgrad.py composes it) in two kernels instead of a
// dozen element-wise launches:
//   g1 = -(accumulated update)            (object: planar (2, n) float32;
//                                          probe: interleaved complex (n))
//   first:  d = -g1
//   else:   d = -g1 + d |g1|^2 / (sum conj(d) (g1 - g0) + 1e-32)
//   g0 <- g1;  first: state[0] = sum(costs) / count   (the cost at x)
// sums[0..3] (double, zeroed here): |g1|^2, Re / Im of the denominator, sum(costs)
__global__ __launch_bounds__(256) void cg_sums_kernel(const float* __restrict__ planar,
                                                      const cf* __restrict__ inter,
                                                      const cf* __restrict__ g0,
                                                      const cf* __restrict__ d, long n, int first,
                                                      const float* __restrict__ costs, int ncost,
                                                      double* __restrict__ sums) {
  __shared__ float red[4];
  __shared__ double redd[256];
  float nn = 0.f, dr = 0.f, di = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const cf a = planar ? mk(planar[i], planar[n + i]) : inter[i];
    const cf g1 = mk(-a.x, -a.y);
    nn += norm2(g1);
    if (!first) {
      const cf y = mk(g1.x - g0[i].x, g1.y - g0[i].y);
      const cf t = conjf(d[i]) * y;
      dr += t.x;
      di += t.y;
    }
  }
  nn = tk_block_sum256(nn, red);
  dr = tk_block_sum256(dr, red);
  di = tk_block_sum256(di, red);
  if (threadIdx.x == 0) {
    unsafeAtomicAdd(&sums[0], (double)nn);
    if (!first) {
      unsafeAtomicAdd(&sums[1], (double)dr);
      unsafeAtomicAdd(&sums[2], (double)di);
    }
  }
  if (first && costs != nullptr) {  // uniform: the mean cost, summed in double
    double cs = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ncost; i += gridDim.x * 256L)
      cs += (double)costs[i];
    redd[threadIdx.x] = cs;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) redd[threadIdx.x] += redd[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0 && redd[0] != 0.0) unsafeAtomicAdd(&sums[3], redd[0]);
  }
}

__global__ __launch_bounds__(256) void cg_direction_kernel(const float* __restrict__ planar,
                                                           const cf* __restrict__ inter,
                                                           cf* __restrict__ g0, cf* __restrict__ d,
                                                           long n, int first, int have_costs,
                                                           double inv_count,
                                                           const double* __restrict__ sums,
                                                           double* __restrict__ state) {
  cf beta = mk(0.f, 0.f);
  if (!first) {
    // |g1|^2 / (den + 1e-32), complex
    const float nr = (float)sums[0];
    const float er = (float)sums[1] + 1e-32f, ei = (float)sums[2];
    const float m = er * er + ei * ei;
    beta = mk(nr * er / m, -nr * ei / m);
  }
  if (first && have_costs && blockIdx.x == 0 && threadIdx.x == 0) state[0] = sums[3] * inv_count;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const cf a = planar ? mk(planar[i], planar[n + i]) : inter[i];
    const cf g1 = mk(-a.x, -a.y);
    cf nd = mk(-g1.x, -g1.y);
    if (!first) {
      const cf t = d[i] * beta;
      nd = mk(t.x - g1.x, t.y - g1.y);
    }
    d[i] = nd;
    g0[i] = g1;
  }
}

extern "C" int tike_cgrad_direction(const float* update_planar, const void* update_complex,
                                    void* gradient, void* direction, long n, int first,
                                    const float* costs, int ncost, double count, double* state,
                                    double* sums, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(n >= 1 && gradient && direction && sums);
  TK_CHECK_ARG((update_planar != nullptr) != (update_complex != nullptr));
  TK_CHECK_ARG(!(first && costs != nullptr) || (ncost >= 1 && count > 0 && state != nullptr));
  hipError_t e = hipMemsetAsync(sums, 0, 4 * sizeof(double), stream);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(tk_grid((n + 255) / 256, 4)), block(256);
  // deterministic mode: ONE summing workgroup (its tree is fixed; the double
  // atomics of several workgroups arrive in any order)
  hipLaunchKernelGGL(cg_sums_kernel, tk_deterministic() ? dim3(1) : grid, block, 0, stream,
                     update_planar,
                     (const cf*)update_complex, (const cf*)gradient, (const cf*)direction, n,
                     first, first ? costs : nullptr, ncost, sums);
  hipLaunchKernelGGL(cg_direction_kernel, grid, block, 0, stream, update_planar,
                     (const cf*)update_complex, (cf*)gradient, (cf*)direction, n, first,
                     (int)(first && costs != nullptr), count > 0 ? 1.0 / count : 0.0, sums, state);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

static int tk_cgrad_line_search(int variable, const void* x, const void* d, void* xs,
                                const void* other, const float* scan, const void* data,
                                int data_u16, void* scratch, float* costs, int nscan, int chunk,
                                int S, int det, int H, int W, float fwd_scale, double count,
                                double* state, int* skip, int nslots,
                                const unsigned char* measured, int model, long num_measured,
                                hipStream_t stream) {
  TK_CHECK_ARG(nscan >= 1 && chunk >= 1 && S >= 1 && H >= 1 && W >= 1 && nslots >= 1 &&
               nslots <= 30 && count > 0 && (variable == 0 || variable == 1));
  TK_CHECK_ARG((model == 0 || model == 1) && num_measured > 0 &&
               num_measured <= (long)det * det);
  TK_CHECK_ARG(x && d && xs && other && scan && data && scratch && costs && state && skip);
  if (det != 128 && det != 256 && det != 512) return TK_ERR_UNSUPPORTED;
  if (det == 128 && data_u16) return TK_ERR_UNSUPPORTED;  // the 128^2 cost kernel reads float32
  const long n = variable == 0 ? (long)H * W : (long)S * det * det;
  hipError_t e = hipMemsetAsync(skip, 0, sizeof(int), stream);
  if (e == hipSuccess) e = hipMemsetAsync(state + 2, 0, sizeof(double), stream);  // done = 0
  if (e != hipSuccess) return (int)e;
  const size_t dsz = data_u16 ? 2 : 4;
  float shrink = 1.0f;
  for (int k = 0; k < nslots; ++k, shrink *= 0.5f) {
    hipLaunchKernelGGL(ls_trial_kernel, dim3(tk_grid((n + 255) / 256, 8)), dim3(256), 0, stream,
                       (const cf*)x, (const cf*)d, (cf*)xs, n, state, shrink, skip);
    const void* psi = variable == 0 ? xs : other;
    const void* probe = variable == 0 ? other : xs;
    for (int lo = 0; lo < nscan; lo += chunk) {
      const int m = nscan - lo < chunk ? nscan - lo : chunk;
      if (det == 128) {
        // whole-tile forward (far plane stored) + the cost of that far plane:
        // the two launches of a host-side trial at this size
        const TkProbe P = tk_make_probe(probe, 0, nullptr, nullptr, 0, 0, S, det);
        int rc = launch_fwd128_lds((const cf*)psi, scan + 2L * lo, P, (cf*)scratch, nullptr, m, S,
                                   H, W, fwd_scale, stream, nullptr, skip);
        if (rc) return rc;
        rc = tk_farplane_gradient(scratch, (const float*)data + (size_t)lo * det * det, measured,
                                  nullptr, costs + lo, m, S, det, model, 0, 1.0f, num_measured,
                                  stream, skip);
        if (rc) return rc;
        continue;
      }
      int rc = tk_fwd_pass1(psi, scan + 2L * lo, probe, 0, nullptr, nullptr, nullptr, 0, 0,
                            scratch, nullptr, m, S, det, det, H, W, stream, skip);
      if (rc) return rc;
      rc = tk_fwd_gradient_scale(scratch, (const char*)data + dsz * (size_t)lo * det * det,
                                 data_u16, measured, nullptr, nullptr, costs + lo, nullptr, m, S,
                                 det, fwd_scale, model, 1.0f, num_measured, stream, skip);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(ls_decide_kernel, dim3(1), dim3(256), 0, stream, costs, nscan,
                       1.0 / count, shrink, k + 1 == nslots, state, skip);
  }
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_cgrad_line_search(int variable, const void* x, const void* d, void* xs,
                                      const void* other, const float* scan, const void* data,
                                      int data_u16, void* scratch, float* costs, int nscan,
                                      int chunk, int S, int det, int H, int W, float fwd_scale,
                                      double count, double* state, int* skip, int nslots,
                                      void* stream_) {
  TK_ENTER();
  return tk_cgrad_line_search(variable, x, d, xs, other, scan, data, data_u16, scratch, costs,
                              nscan, chunk, S, det, H, W, fwd_scale, count, state, skip, nslots,
                              nullptr, 0, (long)det * det, (hipStream_t)stream_);
}

extern "C" int tike_cgrad_line_search_masked(
    int variable, const void* x, const void* d, void* xs, const void* other, const float* scan,
    const void* data, int data_u16, void* scratch, float* costs, int nscan, int chunk, int S,
    int det, int H, int W, float fwd_scale, double count, double* state, int* skip, int nslots,
    const unsigned char* measured, int model, long num_measured, void* stream_) {
  TK_ENTER();
  return tk_cgrad_line_search(variable, x, d, xs, other, scan, data, data_u16, scratch, costs,
                              nscan, chunk, S, det, H, W, fwd_scale, count, state, skip, nslots,
                              measured, model, num_measured, (hipStream_t)stream_);
}

// ------------------------------------------- the same line search, all steps at once
// The far plane is LINEAR in the variable a line search moves along: with
// A = F(x) and B = F(d) (the forward model applied to the direction in place
// of the object, or of the probe), F(x + s d) = A + s B for every step length
// s.  A is the hand-off the gradient pass at x has just left behind; B costs
// ONE forward pass 1; the intensity of a trial is the quadratic
//   I(s) = sum_m |A_m|^2 + 2 s sum_m Re(conj(A_m) B_m) + s^2 sum_m |B_m|^2
// in s per pixel, so one column pass over the TWO hand-offs gives the costs of
// x and of x + step d, x + step/2 d, ... (TK_LS_STEPS of them) together, and
// one small kernel takes the decision of the backtracking search
// (opt.py:216-278): the first of those step lengths whose cost is no larger
// than the cost at x.  Same candidates, same rule, same result as
// tike_cgrad_line_search up to float32 rounding -- for one forward pass and
// one two-stream column pass instead of a forward pass per trial.
constexpr int TK_LS_STEPS = 8;   // step lengths per pass over the hand-offs
constexpr int TK_LS_PASSES = 2;  // passes enqueued (the second returns at once if the first accepted)
constexpr int TK_LS_ROWS = TK_LS_STEPS * TK_LS_PASSES + 1;  // cost rows: x, then every step

// cost terms of RB pixels at step0 / 2^k, k < K (rows 1..K) and, FIRST, at
// step 0 (row 0); MK: only the measured pixels of `bits` (selected, never
// multiplied: unmeasured counts may be NaN).
// Gaussian: v_sqrt_f32 (1 ulp) instead of the correctly rounded sqrtf (a dozen
// instructions each): K x RB square roots per thread are what this kernel
// issues most, and the cost at x it is compared with is formed the same way.
// Poisson: the rows of the step lengths hold the DIFFERENCE from x per pixel,
//   (I(s) - I0) - d log1p((I(s) - I0) / (I0 + 1e-9)),
// so that the decision does not rest on two float32 totals that carry the large
// offset sum(d - d log d); row 0 is the plain term I0 - d log(I0 + 1e-9).
// log1p(r) = log(u) + (r - (u - 1)) / u with u = (I(s) + 1e-9) / (I0 + 1e-9)
// the rounded 1 + r (never 0); 1 / u ~ max(2 - u, 0) is exact enough for a
// correction of the size of u's rounding.
template <int K, int RB, bool FIRST, int MODEL, bool MK, class DT>
__device__ __forceinline__ void tk_ksteps_costs(const float (&I0)[RB], const float (&C)[RB],
                                                const float (&I1)[RB], const DT (&raw)[RB],
                                                unsigned bits, float step0,
                                                float (&acc)[K + 1]) {
#pragma unroll
  for (int p = 0; p < RB; ++p) {
    const bool meas = !MK || ((bits >> p) & 1u);
    const float c2 = 2.0f * C[p];
    if (MODEL == 0) {
      const float sd = __builtin_amdgcn_sqrtf((float)raw[p]);
      if (FIRST) {
        const float t0 = __builtin_amdgcn_sqrtf(I0[p]) - sd;
        const float a0 = fmaf(t0, t0, acc[0]);
        acc[0] = meas ? a0 : acc[0];
      }
      float s = step0;
#pragma unroll
      for (int k = 0; k < K; ++k, s *= 0.5f) {
        const float I = fmaxf(fmaf(s, fmaf(s, I1[p], c2), I0[p]), 0.0f);
        const float t = __builtin_amdgcn_sqrtf(I) - sd;
        const float a = fmaf(t, t, acc[k + 1]);
        acc[k + 1] = meas ? a : acc[k + 1];
      }
    } else {
      const float dv = (float)raw[p];
      const float e0 = I0[p] + 1e-9f;
      if (FIRST) {
        const float a0 = acc[0] + fmaf(-dv, __logf(e0), I0[p]);
        acc[0] = meas ? a0 : acc[0];
      }
      const float inv0 = __builtin_amdgcn_rcpf(e0);
      float s = step0;
#pragma unroll
      for (int k = 0; k < K; ++k, s *= 0.5f) {
        // (dI from s (s I1 + 2 C) itself: I(s) - I0 of the rounded I(s)
        // would be a multiple of ulp(I0), far coarser than the short steps)
        const float dI = fmaxf(s * fmaf(s, I1[p], c2), -I0[p]);
        const float I = I0[p] + dI;
        const float r = dI * inv0;
        const float u = (I + 1e-9f) * inv0;
        const float lp = fmaf(r - (u - 1.0f), fmaxf(2.0f - u, 0.0f), __logf(u));
        const float a = acc[k + 1] + fmaf(-dv, lp, dI);
        acc[k + 1] = meas ? a : acc[k + 1];
      }
    }
  }
}

// per-thread sums -> one atomic each into costs_k[row * stride + n]; acc[0] is
// row 0 (FIRST only), acc[1..K] are rows row1 .. row1 + K - 1
// (deterministic mode: `part` != nullptr receives the contribution of slot
// `slot` of `nslots` per (row, pattern) -- part[(slot * TK_LS_ROWS + row) *
// stride + n] -- and ls_costs_finish_kernel adds the slots in order)
template <int K, bool FIRST>
__device__ __forceinline__ void tk_ksteps_emit(float (&acc)[K + 1], float (*red)[K + 1],
                                               float* __restrict__ costs_k, long stride, long n,
                                               int row1, float inv_nmeasured,
                                               float* __restrict__ part = nullptr,
                                               int slot = 0) {
#pragma unroll
  for (int k = FIRST ? 0 : 1; k <= K; ++k) acc[k] = tk_wave_sum(acc[k]);
  __syncthreads();  // the previous item's sums have been read
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k <= K; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k <= K && (FIRST || k > 0)) {
    const int row = k == 0 ? 0 : row1 + k - 1;
    const float v = (red[0][k] + red[1][k] + red[2][k] + red[3][k]) * inv_nmeasured;
    if (part != nullptr)
      part[((long)slot * TK_LS_ROWS + row) * stride + n] = v;
    else
      unsafeAtomicAdd(&costs_k[row * stride + n], v);
  }
}

// 256^2 / 512^2: the column pass of fwd_gradient_scale_kernel over the
// hand-offs of x (col_a) and of the direction (col_b)
template <int N, class DT, bool FIRST, int MODEL, bool MK>
__global__ __launch_bounds__(256, 2) void ls_ksteps_colpass_kernel(
    const cf* __restrict__ col_a, const cf* __restrict__ col_b, const DT* __restrict__ data,
    const unsigned char* __restrict__ mask, float* __restrict__ costs_k, long stride, long nitem, int S, float scale,
    float inv_nmeasured, int row1, const double* __restrict__ state,
    float* __restrict__ part) {
  constexpr int RB = N / 16, NH = N / 256, K = TK_LS_STEPS;
  __shared__ float red[4][K + 1];
  if (!FIRST && state[2] != 0.0) return;  // an earlier pass has accepted a step
  const float s2 = scale * scale;
  const float step0 = (float)state[1];
  for (long v = blockIdx.x; v < nitem; v += gridDim.x) {
    const int hb = (int)(v % NH);
    const int k1 = (int)((v / NH) & 15);
    const long n = nitem / (16 * NH) - 1 - v / (16 * NH);  // descending, as its siblings
    const int t = hb * 256 + threadIdx.x;
    float I0[RB], C[RB], I1[RB];
#pragma unroll
    for (int k2 = 0; k2 < RB; ++k2) I0[k2] = C[k2] = I1[k2] = 0.f;
    for (int s = 0; s < S; ++s) {
      const long off = (n * S + s) * (long)N * N + k1 * N + t;
      cf a[RB], b[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) a[r] = tk_ld_stream(col_a + off + (long)(16 * r) * N);
#pragma unroll
      for (int r = 0; r < RB; ++r) b[r] = tk_ld_stream(col_b + off + (long)(16 * r) * N);
      Dft<RB, false>::run(a);
      Dft<RB, false>::run(b);
#pragma unroll
      for (int k2 = 0; k2 < RB; ++k2) {
        I0[k2] += norm2(a[k2]) * s2;
        C[k2] += (a[k2].x * b[k2].x + a[k2].y * b[k2].y) * s2;
        I1[k2] += norm2(b[k2]) * s2;
      }
    }
    DT raw[RB];
    unsigned bits;
    tk_request_data<N, RB>(data, !MK ? (const unsigned char*)nullptr : mask, n, k1, t, raw, bits);
    float acc[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) acc[k] = 0.f;
    tk_ksteps_costs<K, RB, FIRST, MODEL, MK>(I0, C, I1, raw, bits, step0, acc);
    tk_ksteps_emit<K, FIRST>(acc, red, costs_k, stride, n, row1, inv_nmeasured, part,
                             k1 * NH + hb);
  }
}

// deterministic mode: costs_k[row][n] = sum over the slots, in slot order
__global__ __launch_bounds__(256) void ls_costs_finish_kernel(float* __restrict__ costs_k,
                                                              const float* __restrict__ part,
                                                              long stride, int n0, int n1,
                                                              int row_first, int row1,
                                                              int nslots) {
  constexpr int K = TK_LS_STEPS;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < (long)(K + 1) * (n1 - n0);
       i += gridDim.x * 256L) {
    const int k = (int)(i / (n1 - n0));
    const long n = n0 + i % (n1 - n0);
    if (k == 0 && !row_first) continue;
    const int row = k == 0 ? 0 : row1 + k - 1;
    float s = 0.f;
    for (int c = 0; c < nslots; ++c) s += part[((long)c * TK_LS_ROWS + row) * stride + n];
    costs_k[row * stride + n] = s;
  }
}

// stored far planes (128^2): a workgroup covers TK_FG_PIX pixels of one position
template <bool FIRST, int MODEL, bool MK>
__global__ __launch_bounds__(256) void ls_ksteps_farplane_kernel(
    const cf* __restrict__ far_a, const cf* __restrict__ far_b, const float* __restrict__ data,
    const unsigned char* __restrict__ mask, float* __restrict__ costs_k, long stride, int S, long npix, float inv_nmeasured, int row1,
    const double* __restrict__ state, float* __restrict__ part) {
  constexpr int K = TK_LS_STEPS;
  __shared__ float red[4][K + 1];
  if (!FIRST && state[2] != 0.0) return;
  const float step0 = (float)state[1];
  const long n = blockIdx.y;
  const cf* __restrict__ FA = far_a + n * S * npix;
  const cf* __restrict__ FB = far_b + n * S * npix;
  const long p0 = (long)blockIdx.x * TK_FG_PIX;
  const long p1 = p0 + TK_FG_PIX < npix ? p0 + TK_FG_PIX : npix;
  float acc[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) acc[k] = 0.f;
  for (long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    float I0[1] = {0.f}, C[1] = {0.f}, I1[1] = {0.f};
    const float raw[1] = {data[n * npix + p]};
    const unsigned bits = MK ? (mask[p] ? 1u : 0u) : 1u;
    for (int s = 0; s < S; ++s) {
      const cf a = FA[s * npix + p], b = FB[s * npix + p];
      I0[0] += norm2(a);
      C[0] += a.x * b.x + a.y * b.y;
      I1[0] += norm2(b);
    }
    tk_ksteps_costs<K, 1, FIRST, MODEL, MK>(I0, C, I1, raw, bits, step0, acc);
  }
  tk_ksteps_emit<K, FIRST>(acc, red, costs_k, stride, n, row1, inv_nmeasured, part,
                           (int)blockIdx.x);
}

// One workgroup: the means of a pass's cost rows, then the backtracking
// decision.  state { fx, step, done, trials, failures } as in ls_decide_kernel.
// First pass: fx on entry is ignored -- the cost at x is row 0, formed with the
// same arithmetic as the trials it is compared with -- and kept in state[0] for
// the passes behind it.  A pass that accepts nothing leaves step = the next
// length to try; the last one also counts a failure.  relative (poisson): the
// rows of the step lengths hold cost(s) - cost(x); a step is accepted when that
// is no larger than 0, and state[0] = cost(x) + the difference.
__global__ __launch_bounds__(256) void ls_pick_kernel(const float* __restrict__ costs_k,
                                                      long stride, int n, double inv_count,
                                                      int row1, int first, int last,
                                                      int relative, double* __restrict__ state,
                                                      int* __restrict__ accepted) {
  constexpr int K = TK_LS_STEPS;
  __shared__ double red[256];
  __shared__ double mean[K + 1];
  if (!first && state[2] != 0.0) return;
  for (int k = first ? 0 : 1; k <= K; ++k) {
    const float* __restrict__ row = costs_k + (k == 0 ? 0 : row1 + k - 1) * stride;
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += (double)row[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) mean[k] = red[0] * inv_count;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double fx = first ? mean[0] : state[0];
    const double bar = relative ? 0.0 : fx;
    float s = (float)state[1];
    int pick = -1;
    for (int k = 0; k < K; ++k, s *= 0.5f) {
      if (mean[k + 1] <= bar) {
        pick = k;
        break;
      }
    }
    if (pick >= 0) {
      state[0] = relative ? fx + mean[pick + 1] : mean[pick + 1];
      state[1] = (double)s;
      state[2] = 1.0;
      state[3] += (double)(pick + 1);
      *accepted = 1;
    } else {
      state[0] = fx;
      state[1] = (double)s;  // step / 2^K: the next length to try
      state[2] = 0.0;
      state[3] += (double)K;
      if (last) state[4] += 1.0;
    }
  }
}

// Several ranks: the sums of a pass's cost rows over THIS rank's positions,
// to be all-reduced between the cost pass and the decision (row 0 only for
// the first pass).  One workgroup; sums (TK_LS_ROWS doubles).
__global__ __launch_bounds__(256) void ls_rowsum_kernel(const float* __restrict__ costs_k,
                                                        long stride, int n, int row1, int first,
                                                        const double* __restrict__ state,
                                                        double* __restrict__ sums) {
  constexpr int K = TK_LS_STEPS;
  __shared__ double red[256];
  const bool skip = !first && state[2] != 0.0;  // accepted already: leave zeros
  for (int k = first ? 0 : 1; k <= K; ++k) {
    const int rowi = k == 0 ? 0 : row1 + k - 1;
    double a = 0.0;
    if (!skip)
      for (int i = threadIdx.x; i < n; i += 256) a += (double)costs_k[rowi * stride + i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[rowi] = red[0];
    __syncthreads();
  }
}

// The decision of ls_pick_kernel from (all-reduced) row sums.
__global__ void ls_pick_sums_kernel(const double* __restrict__ sums, double inv_count, int row1,
                                    int first, int last, int relative,
                                    double* __restrict__ state, int* __restrict__ accepted) {
  constexpr int K = TK_LS_STEPS;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!first && state[2] != 0.0) return;
  const double fx = first ? sums[0] * inv_count : state[0];
  const double bar = relative ? 0.0 : fx;
  float s = (float)state[1];
  int pick = -1;
  for (int k = 0; k < K; ++k, s *= 0.5f) {
    if (sums[row1 + k] * inv_count <= bar) {
      pick = k;
      break;
    }
  }
  if (pick >= 0) {
    state[0] = relative ? fx + sums[row1 + pick] * inv_count : sums[row1 + pick] * inv_count;
    state[1] = (double)s;
    state[2] = 1.0;
    state[3] += (double)(pick + 1);
    *accepted = 1;
  } else {
    state[0] = fx;
    state[1] = (double)s;
    state[2] = 0.0;
    state[3] += (double)K;
    if (last) state[4] += 1.0;
  }
}

// xs = x + step d with the accepted step (x itself when none was)
__global__ __launch_bounds__(256) void ls_apply_kernel(const cf* __restrict__ x,
                                                       const cf* __restrict__ d,
                                                       cf* __restrict__ xs, long n,
                                                       const double* __restrict__ state) {
  const float a = state[2] != 0.0 ? (float)state[1] : 0.0f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const cf v = d[i];
    xs[i] = mk(x[i].x + a * v.x, x[i].y + a * v.y);
  }
}

static int tk_cgrad_line_search_linear(int variable, const void* x, const void* d, void* xs,
                                       const void* other, const float* scan, const void* data,
                                       int data_u16, void* far_a, int a_valid, void* far_b,
                                       float* costs_k, int nscan, int chunk, int S, int det,
                                       int H, int W, float fwd_scale, double count,
                                       double* state, int stage, double* sums,
                                       const unsigned char* measured, int model,
                                       long num_measured, hipStream_t stream) {
  TK_CHECK_ARG(nscan >= 1 && chunk >= 1 && S >= 1 && H >= 1 && W >= 1 && count > 0 &&
               (variable == 0 || variable == 1));
  TK_CHECK_ARG((model == 0 || model == 1) && num_measured > 0 &&
               num_measured <= (long)det * det);
  TK_CHECK_ARG(x && d && xs && other && scan && data && far_a && far_b && far_a != far_b &&
               costs_k && state);
  // stage 0: the whole search (one rank).  Several ranks, whose cost sums
  // must be all-reduced between a cost pass and its decision: 1 = first cost
  // pass -> sums; 2 = first decision from sums; 3 = second cost pass -> sums;
  // 4 = second decision from sums, then xs.
  TK_CHECK_ARG(stage >= 0 && stage <= 4 && (stage == 0 || sums != nullptr));
  if (det != 128 && det != 256 && det != 512) return TK_ERR_UNSUPPORTED;
  if (det == 128 && data_u16) return TK_ERR_UNSUPPORTED;  // the 128^2 cost kernel reads float32
  const long n = variable == 0 ? (long)H * W : (long)S * det * det;
  // (+ one word behind the rows: raised once a step is accepted -- the forward
  // passes of a later pass over a several-chunk minibatch read it and return)
  int* accepted = reinterpret_cast<int*>(costs_k + (size_t)TK_LS_ROWS * nscan);
  if (stage <= 1) {
    hipError_t e = hipMemsetAsync(
        costs_k, 0, sizeof(float) * ((size_t)TK_LS_ROWS * nscan + 1), stream);
    if (e != hipSuccess) return (int)e;
  }
  // deterministic mode: every (row, pattern) cost has `nslots` contributors --
  // their values go to the caller's scratch buffer and are added in slot order
  const int nslots = det == 128 ? (int)(((long)det * det + TK_FG_PIX - 1) / TK_FG_PIX)
                                : 16 * (det / 256);
  float* part = nullptr;
  if (tk_deterministic()) {
    part = tk_det_scratch(sizeof(float) * (size_t)nslots * TK_LS_ROWS * nscan);
    if (part == nullptr) return TK_ERR_ARG;  // scratch buffer too small
  }
  const bool reuse = a_valid && nscan <= chunk;  // the gradient pass left F(x) in far_a
  const bool resident = nscan <= chunk;          // one chunk: both hand-offs stay put
  const size_t dsz = data_u16 ? 2 : 4;
  const float inv = 1.0f / (float)num_measured;
  const bool mk = measured != nullptr;
  // forward model of the direction: d in place of the variable
  const void* psi_b = variable == 0 ? d : other;
  const void* probe_b = variable == 0 ? other : d;
  const void* psi_a = variable == 0 ? x : other;
  const void* probe_a = variable == 0 ? other : x;
  static_assert(TK_LS_PASSES == 2, "stages 1-4 name two passes");
  for (int pass = 0; pass < TK_LS_PASSES; ++pass) {
    const int row1 = 1 + pass * TK_LS_STEPS;
    const bool costs_now = stage == 0 || stage == 1 + 2 * pass;
    const bool decide_now = stage == 0 || stage == 2 + 2 * pass;
    if (!costs_now && !decide_now) continue;
    for (int lo = 0; costs_now && lo < nscan; lo += chunk) {
      const int m = nscan - lo < chunk ? nscan - lo : chunk;
      const float* sc = scan + 2L * lo;
      // the hand-offs of a chunk: formed in the first pass; a later pass (rare:
      // the first one accepted nothing) finds them in place unless the
      // minibatch has several chunks, which share the two buffers
      const bool form = pass == 0 || !resident;
      if (det == 128) {
        if (form && !(reuse && pass == 0)) {
          const TkProbe PA = tk_make_probe(probe_a, 0, nullptr, nullptr, 0, 0, S, det);
          int rc = launch_fwd128_lds((const cf*)psi_a, sc, PA, (cf*)far_a, nullptr, m, S, H, W,
                                     fwd_scale, stream, nullptr, pass ? accepted : nullptr);
          if (rc) return rc;
        }
        if (form) {
          const TkProbe PB = tk_make_probe(probe_b, 0, nullptr, nullptr, 0, 0, S, det);
          int rc = launch_fwd128_lds((const cf*)psi_b, sc, PB, (cf*)far_b, nullptr, m, S, H, W,
                                     fwd_scale, stream, nullptr, pass ? accepted : nullptr);
          if (rc) return rc;
        }
        const long npix = (long)det * det;
        // the chunk's positions in gridDim.y, in slices of at most the device's
        // limit (`at`: first position of the slice within the chunk)
        TK_GRID_Y_LIMIT(ymax);
        const unsigned gx = (unsigned)((npix + TK_FG_PIX - 1) / TK_FG_PIX);
        const float* dchunk = (const float*)data + (size_t)lo * npix;
#define TK_LSF(FIRST, M, MK)                                                                  \
  hipLaunchKernelGGL((ls_ksteps_farplane_kernel<FIRST, M, MK>), grid, dim3(256), 0, stream,      \
                     (const cf*)far_a + at * S * npix, (const cf*)far_b + at * S * npix,          \
                     dchunk + at * npix, measured, costs_k + lo + at, (long)nscan, S, npix, inv,  \
                     row1, state, part ? part + lo + at : part)
#define TK_LSF_M(FIRST)          \
  do {                           \
    if (model == 0 && !mk)       \
      TK_LSF(FIRST, 0, false);   \
    else if (model == 0)         \
      TK_LSF(FIRST, 0, true);    \
    else if (!mk)                \
      TK_LSF(FIRST, 1, false);   \
    else                         \
      TK_LSF(FIRST, 1, true);    \
  } while (0)
        for (long at = 0; at < m; at += ymax) {
          const dim3 grid(gx, (unsigned)(m - at < ymax ? m - at : ymax));
          if (pass == 0)
            TK_LSF_M(true);
          else
            TK_LSF_M(false);
        }
#undef TK_LSF_M
#undef TK_LSF
        if (part)
          hipLaunchKernelGGL(ls_costs_finish_kernel, dim3(tk_grid((long)(m * 9 + 255) / 256, 8)),
                             dim3(256), 0, stream, costs_k, part, (long)nscan, lo, lo + m,
                             (int)(pass == 0), row1, nslots);
        continue;
      }
      if (form && !(reuse && pass == 0)) {
        int rc = tk_fwd_pass1(psi_a, sc, probe_a, 0, nullptr, nullptr, nullptr, 0, 0, far_a,
                              nullptr, m, S, det, det, H, W, stream, pass ? accepted : nullptr);
        if (rc) return rc;
      }
      if (form) {
        int rc = tk_fwd_pass1(psi_b, sc, probe_b, 0, nullptr, nullptr, nullptr, 0, 0, far_b,
                              nullptr, m, S, det, det, H, W, stream, pass ? accepted : nullptr);
        if (rc) return rc;
      }
      const long nitem = (long)m * 16 * (det / 256);
      const dim3 grid(tk_grid(nitem, 32)), block(256);
      const char* dchunk = (const char*)data + dsz * (size_t)lo * det * det;
#define TK_LSK(N, DT, FIRST, M, MK)                                                           \
  hipLaunchKernelGGL((ls_ksteps_colpass_kernel<N, DT, FIRST, M, MK>), grid, block, 0, stream,    \
                     (const cf*)far_a, (const cf*)far_b, (const DT*)dchunk, measured,            \
                     costs_k + lo, (long)nscan, nitem, S, fwd_scale, inv, row1, state,           \
                     part ? part + lo : part)
#define TK_LSK_M(N, DT, FIRST)           \
  do {                                   \
    if (model == 0 && !mk)               \
      TK_LSK(N, DT, FIRST, 0, false);    \
    else if (model == 0)                 \
      TK_LSK(N, DT, FIRST, 0, true);     \
    else if (!mk)                        \
      TK_LSK(N, DT, FIRST, 1, false);    \
    else                                 \
      TK_LSK(N, DT, FIRST, 1, true);     \
  } while (0)
#define TK_LSK_N(N, DT)        \
  do {                         \
    if (pass == 0)             \
      TK_LSK_M(N, DT, true);   \
    else                       \
      TK_LSK_M(N, DT, false);  \
  } while (0)
      if (det == 256 && data_u16)
        TK_LSK_N(256, unsigned short);
      else if (det == 256)
        TK_LSK_N(256, float);
      else if (data_u16)
        TK_LSK_N(512, unsigned short);
      else
        TK_LSK_N(512, float);
#undef TK_LSK_N
#undef TK_LSK_M
#undef TK_LSK
      if (part)
        hipLaunchKernelGGL(ls_costs_finish_kernel, dim3(tk_grid((long)(m * 9 + 255) / 256, 8)),
                           dim3(256), 0, stream, costs_k, part, (long)nscan, lo, lo + m,
                           (int)(pass == 0), row1, nslots);
    }
    if (stage == 0)
      hipLaunchKernelGGL(ls_pick_kernel, dim3(1), dim3(256), 0, stream, costs_k, (long)nscan,
                         nscan, 1.0 / count, row1, (int)(pass == 0),
                         (int)(pass + 1 == TK_LS_PASSES), model, state, accepted);
    else if (costs_now)
      hipLaunchKernelGGL(ls_rowsum_kernel, dim3(1), dim3(256), 0, stream, costs_k, (long)nscan,
                         nscan, row1, (int)(pass == 0), state, sums);
    else
      hipLaunchKernelGGL(ls_pick_sums_kernel, dim3(1), dim3(64), 0, stream, sums, 1.0 / count,
                         row1, (int)(pass == 0), (int)(pass + 1 == TK_LS_PASSES), model, state,
                         accepted);
  }
  if (stage != 0 && stage != 4) {
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  hipLaunchKernelGGL(ls_apply_kernel, dim3(tk_grid((n + 255) / 256, 8)), dim3(256), 0, stream,
                     (const cf*)x, (const cf*)d, (cf*)xs, n, state);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_cgrad_line_search_linear(int variable, const void* x, const void* d, void* xs,
                                             const void* other, const float* scan,
                                             const void* data, int data_u16, void* far_a,
                                             int a_valid, void* far_b, float* costs_k,
                                             int nscan, int chunk, int S, int det, int H, int W,
                                             float fwd_scale, double count, double* state,
                                             int stage, double* sums, void* stream_) {
  TK_ENTER();
  return tk_cgrad_line_search_linear(variable, x, d, xs, other, scan, data, data_u16, far_a,
                                     a_valid, far_b, costs_k, nscan, chunk, S, det, H, W,
                                     fwd_scale, count, state, stage, sums, nullptr, 0,
                                     (long)det * det, (hipStream_t)stream_);
}

extern "C" int tike_cgrad_line_search_linear_masked(
    int variable, const void* x, const void* d, void* xs, const void* other, const float* scan,
    const void* data, int data_u16, void* far_a, int a_valid, void* far_b, float* costs_k,
    int nscan, int chunk, int S, int det, int H, int W, float fwd_scale, double count,
    double* state, int stage, double* sums, const unsigned char* measured, int model,
    long num_measured, void* stream_) {
  TK_ENTER();
  return tk_cgrad_line_search_linear(variable, x, d, xs, other, scan, data, data_u16, far_a,
                                     a_valid, far_b, costs_k, nscan, chunk, S, det, H, W,
                                     fwd_scale, count, state, stage, sums, measured, model,
                                     num_measured, (hipStream_t)stream_);
}
