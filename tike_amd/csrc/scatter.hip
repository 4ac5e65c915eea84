// The footprint scatter for gfx950: the adjoint of the bilinear patch gather,
// for the least-squares + gradient update loop (lstsq_grad), the adjoint
// operator (adjoint.hip) and the preconditioners.
//
// Reference:
//   operators/cupy/convolution.cu:35-165 (adj_patch), as called by
//   ptycho/solvers/lstsq.py:510-520  object gradient  sum_s conj(P_n,s) chi_n,s scattered
//                                                                    -> tike_scatter_patches
//   solvers/_preconditioner.py:48-104 psi preconditioner             -> tike_psi_preconditioner
//   solvers/_preconditioner.py:82-95  the same, multislice object    -> tike_scatter_amplitudes
// Direct, grouped and ordered (deterministic mode) scatter-add of a patch's
// (pw+1)^2 footprint with one atomic per object pixel and position.
#include <type_traits>

#include "internal.h"
#include "tike_amd.h"

// ------------------------------------------------- footprint scatter-add
// Adjoint of the bilinear patch gather with ONE atomic per object pixel and
// position instead of four per patch pixel: the patch value v[y][x] reaches
// the (pw+1)^2 object pixels (sy+y', sx+x') with
//   f[y'][x'] = (1-fy) u[y'][x'] + fy u[y'-1][x'],
//   u[y'][x'] = (1-fx) v[y'][x'] + fx v[y'][x'-1]          (v = 0 outside)
// which expands to the reference's four products w00..w11 (convolution.cu:
// 130-135).  A workgroup owns a strip of rows of one position; a thread owns
// a column, walks down the strip keeping u[y'-1] in registers and takes its
// left neighbour's v by wave shuffle.  Requires positions that keep the patch
// inside the image (check_allowed_positions, position.py:600-628); pixels
// falling outside are dropped.
constexpr int TK_STRIP = 32;
#define TK_ATOMIC_ADD(p, v) unsafeAtomicAdd(p, v)

// The accumulation image is PLANAR (all real parts, then all imaginary parts):
// one atomic wave-instruction then covers 256 contiguous bytes, the shape that
// runs at the full atomic rate (interleaved complex halves it).
// `sink(yp, xp, re, im)` receives the footprint value of row y' = yp, column
// x' = xp (0 <= yp, xp <= pw); rows y' in [r0, r1) are produced.
template <bool REAL_ONLY, class ValueFn, class Sink>
__device__ __forceinline__ void scatter_footprint_rows(ValueFn&& value, float fx, float fy,
                                                       int pw, int r0, int r1, Sink&& sink) {
  for (int x0 = 0; x0 < pw; x0 += blockDim.x) {
    const int xp = x0 + threadIdx.x;  // column x' (also the patch column)
    const bool active = xp < pw;
    cf uprev = mk(0.f, 0.f), uprev_last = mk(0.f, 0.f);
    constexpr int RG = 4;  // rows whose loads are issued together
    // Software pipeline: the loads of row group g+1 are issued BEFORE the
    // atomics of group g.  vmcnt retires in issue order, so a load issued
    // after an atomic would wait for that atomic's full round trip.
    cf vv[RG], ll[RG], nv[RG], nl[RG];
    auto load_group = [&](int yb, cf (&a)[RG], cf (&b)[RG]) {
      const int xpc = active ? xp : pw - 1;
#pragma unroll
      for (int k = 0; k < RG; ++k) {
        const int ypc = yb + k < pw ? yb + k : pw - 1;  // clamped, unconditional
        a[k] = value(ypc, xpc);
      }
      // left neighbour for lane 0 of each wave (the others take it by shuffle)
      if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < RG; ++k) {
          const int ypc = yb + k < pw ? yb + k : pw - 1;
          b[k] = value(ypc, xpc > 0 ? xpc - 1 : 0);
        }
      }
    };
    const int ystart = max(r0 - 1, 0);
    load_group(ystart, vv, ll);
    for (int yb = ystart; yb < r1; yb += RG) {
      if (yb + RG < r1) load_group(yb + RG, nv, nl);
#pragma unroll
      for (int k = 0; k < RG; ++k) {
        const int yp = yb + k;
        if (yp >= r1) break;
        cf v = (active && yp < pw) ? vv[k] : mk(0.f, 0.f);
        cf left = mk(__shfl_up(v.x, 1, 64), __shfl_up(v.y, 1, 64));
        if ((threadIdx.x & 63) == 0)
          left = (active && xp > 0 && yp < pw) ? ll[k] : mk(0.f, 0.f);
        const cf u = mk((1.0f - fx) * v.x + fx * left.x, (1.0f - fx) * v.y + fx * left.y);
        // the thread owning the last patch column also produces column x' = pw
        const cf ulast = mk(fx * v.x, fx * v.y);
        if (yp >= r0 && active) {
          sink(yp, xp, (1.0f - fy) * u.x + fy * uprev.x,
               REAL_ONLY ? 0.f : (1.0f - fy) * u.y + fy * uprev.y);
          if (xp == pw - 1)
            sink(yp, pw, (1.0f - fy) * ulast.x + fy * uprev_last.x,
                 REAL_ONLY ? 0.f : (1.0f - fy) * ulast.y + fy * uprev_last.y);
        }
        uprev = u;
        uprev_last = ulast;
      }
#pragma unroll
      for (int k = 0; k < RG; ++k) {
        vv[k] = nv[k];
        ll[k] = nl[k];
      }
    }
  }
}

// One position, one strip of TK_STRIP rows, straight to the image by atomics.
template <bool REAL_ONLY, class ValueFn>
__device__ __forceinline__ void scatter_footprint(ValueFn&& value, const TkCorner& c,
                                                  float fx, float fy, float* __restrict__ re,
                                                  float* __restrict__ im, int pw, int H, int W,
                                                  int strip) {
  const int r0 = strip * TK_STRIP;
  const int r1 = min(pw + 1, r0 + TK_STRIP);  // rows y' in [r0, r1)
  scatter_footprint_rows<REAL_ONLY>(value, fx, fy, pw, r0, r1,
                                    [&](int yp, int xp, float vr, float vi) {
                                      const int Y = c.sy + yp, X = c.sx + xp;
                                      if (Y >= 0 && Y < H && X >= 0 && X < W) {
                                        const long ii = (long)Y * W + X;
                                        TK_ATOMIC_ADD(&re[ii], vr);
                                        if (!REAL_ONLY) TK_ATOMIC_ADD(&im[ii], vi);
                                      }
                                    });
}

// ------------------------------------------- grouped footprint scatter-add
// Footprints of neighbouring scan positions overlap almost entirely (pw =
// 256 against a pitch of tens of pixels), so TK_GROUP CONSECUTIVE positions
// are summed on chip first -- over the bounding box of their footprints, one
// strip of TK_GROWS image rows per workgroup, one thread per box column with
// the row sums in registers (rounds 2-4: in LDS, a barrier per position) --
// and the image then takes ONE atomic per box pixel instead of one per
// position and pixel.  The caller orders positions so that consecutive ones
// are neighbours (the solver sorts every minibatch spatially); a group whose
// box is wider than TK_GSPREAD allows falls back to the per-position
// atomics, so any order gives the same sums.
constexpr int TK_GROUP = 8;
constexpr int TK_GROWS = 8;     // image rows per workgroup
constexpr int TK_GSPREAD = 112;  // extra box width and height beyond one footprint

struct TkGroupBox {
  int ymin, ymax, xmin, xmax;  // inclusive image bounds of the union footprint
};

__device__ __forceinline__ TkGroupBox tk_group_box(const float* __restrict__ scan, long n0,
                                                   long n1, int pw) {
  TkGroupBox b = {1 << 30, -(1 << 30), 1 << 30, -(1 << 30)};
  for (long n = n0; n < n1; ++n) {
    const int sy = (int)floorf(scan[2 * n]), sx = (int)floorf(scan[2 * n + 1]);
    b.ymin = min(b.ymin, sy);
    b.ymax = max(b.ymax, sy + pw);
    b.xmin = min(b.xmin, sx);
    b.xmax = max(b.xmax, sx + pw);
  }
  return b;
}

// lane i receives lane i - 1 (wave_shr:1); lane 0 receives 0
__device__ __forceinline__ float tk_lane_down(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}

// value(n, y, x): patch value of position n.  Round 5: a thread owns a COLUMN
// of the box and keeps its TK_GROWS row sums in registers -- no LDS, no
// barrier, and (inside a group) a fixed summation order.  For position n the
// thread's column is patch column x' = X - sx_n; it needs v[y'][x'] of the
// TK_GROWS + 1 patch rows that reach the strip and, for the tap to the left,
// its left neighbour's values: lane - 1 holds x' - 1 of the same position (DPP
// wave shift).  Lane 0 of every wave is a HALO lane: it repeats the last
// column of the wave before it, feeds lane 1 and writes nothing -- a wave
// covers 63 box columns and no lane ever needs a value from another wave
// (loading those at a wave-uniform address made scalar loads of them, each
// waited for on its own: 9 serial latencies per position).  Every load is
// unconditional (clamped address, value selected): the rows of the next
// position are requested before the sums of this one.
constexpr int TK_GCOLS = 63;  // box columns per wave

// rowptr(n, y): (uniform) pointer to row y of the patch of position n -- cf, or
// float when REAL_ONLY.  Columns outside the patch take weight 0 instead of a
// select per row (their clamped loads return finite values of the same row).
template <bool REAL_ONLY, class RowFn>
__device__ __forceinline__ void scatter_group(RowFn&& rowptr, const float* __restrict__ scan,
                                              long n0, long n1, int strip, int wmax,
                                              float* __restrict__ re, float* __restrict__ im,
                                              int pw, int H, int W) {
  using T = std::conditional_t<REAL_ONLY, float, cf>;
  auto ld = [](const T* p) {
    if constexpr (REAL_ONLY) return mk(*p, 0.f);
    else return *p;
  };
  const TkGroupBox b = tk_group_box(scan, n0, n1, pw);
  const int wb = b.xmax - b.xmin + 1;
  const int hb = b.ymax - b.ymin + 1;
  const int nstrip_direct = (pw + 1 + TK_STRIP - 1) / TK_STRIP;
  if (wb > wmax || hb > pw + 1 + TK_GSPREAD) {
    // positions too far apart for one box: per-position atomics; the
    // first workgroups of the group share the (position, strip) items
    const int nwg = (pw + 1 + TK_GSPREAD + TK_GROWS - 1) / TK_GROWS;
    for (long w = strip; w < (n1 - n0) * nstrip_direct; w += nwg) {
      const long n = n0 + w / nstrip_direct;
      const TkCorner c = tk_corner(scan, n);
      const float fy = scan[2 * n] - floorf(scan[2 * n]);
      const float fx = scan[2 * n + 1] - floorf(scan[2 * n + 1]);
      scatter_footprint<REAL_ONLY>([&](int y, int x) { return ld(rowptr(n, y) + x); }, c, fx,
                                   fy, re, im, pw, H, W, (int)(w % nstrip_direct));
    }
    return;
  }
  const int Y0 = b.ymin + strip * TK_GROWS;
  if (Y0 > b.ymax) return;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int nwave = (int)blockDim.x >> 6;
  const int lane = threadIdx.x & 63;
  constexpr int R = TK_GROWS + 1;  // patch rows y'_0 - 1 .. y'_0 + TK_GROWS - 1
  for (int c0 = wave * TK_GCOLS; c0 < wb; c0 += nwave * TK_GCOLS) {  // uniform
    const int X = b.xmin + c0 + lane - 1;  // lane 0: the column left of the wave's first
    // rows of position n at this thread's column; (wv, wl) = weights of the
    // thread's own value and of its left neighbour's in u = (1-fx) v + fx v_left
    auto load = [&](long n, cf (&v)[R], float& wv, float& wl) {
      const float py = scan[2 * n], px = scan[2 * n + 1];
      const int sy = (int)floorf(py), sx = (int)floorf(px);
      const float fx = px - floorf(px);
      const int xq = X - sx;
      const bool okx = (unsigned)xq < (unsigned)pw;
      wv = okx ? 1.0f - fx : 0.f;
      wl = (unsigned)(xq - 1) < (unsigned)pw ? fx : 0.f;
      const unsigned off = (unsigned)(okx ? xq : 0) * (unsigned)sizeof(T);
      const int y0 = Y0 - sy - 1;
      if (y0 >= 0 && y0 + R <= pw) {  // uniform: every row inside the patch
        const T* __restrict__ base = rowptr(n, y0);
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = ld(tk_at(base + (long)j * pw, off));
      } else {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int y = y0 + j;
          const bool oky = y >= 0 && y < pw;
          const cf a = ld(tk_at(rowptr(n, oky ? y : 0), off));
          v[j] = oky ? a : mk(0.f, 0.f);
        }
      }
    };
    float ar[TK_GROWS], ai[TK_GROWS];
#pragma unroll
    for (int k = 0; k < TK_GROWS; ++k) ar[k] = ai[k] = 0.f;
    cf v[R], nv[R];
    float wv, wl, nwv = 0.f, nwl = 0.f;
    load(n0, v, wv, wl);
    for (long n = n0; n < n1; ++n) {
      if (n + 1 < n1) load(n + 1, nv, nwv, nwl);
      const float py = scan[2 * n];
      const float fy = py - floorf(py);
      cf u[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const cf left = mk(tk_lane_down(v[j].x), REAL_ONLY ? 0.f : tk_lane_down(v[j].y));
        u[j] = mk(wv * v[j].x + wl * left.x, REAL_ONLY ? 0.f : wv * v[j].y + wl * left.y);
      }
#pragma unroll
      for (int k = 0; k < TK_GROWS; ++k) {
        ar[k] += (1.0f - fy) * u[k + 1].x + fy * u[k].x;
        if (!REAL_ONLY) ai[k] += (1.0f - fy) * u[k + 1].y + fy * u[k].y;
      }
#pragma unroll
      for (int j = 0; j < R; ++j) v[j] = nv[j];
      wv = nwv;
      wl = nwl;
    }
    if (lane > 0 && X <= b.xmax && X >= 0 && X < W) {
#pragma unroll
      for (int k = 0; k < TK_GROWS; ++k) {
        const int Y = Y0 + k;
        if (Y > b.ymax || Y < 0 || Y >= H) continue;
        const long ii = (long)Y * W + X;
        if (REAL_ONLY) {
          if (ar[k] != 0.f) TK_ATOMIC_ADD(&re[ii], ar[k]);
        } else if (ar[k] != 0.f || ai[k] != 0.f) {
          TK_ATOMIC_ADD(&re[ii], ar[k]);
          TK_ATOMIC_ADD(&im[ii], ai[k]);
        }
      }
    }
  }
}

// Deterministic form of the same sum (tike_set_deterministic): a wave OWNS 63
// image columns of a strip of TK_GROWS rows and walks ALL positions in index
// order, adding the footprint values of those that reach its pixels in
// registers; the image is then updated by plain read-modify-writes -- every
// pixel has one owner, every sum one order.  Same arithmetic per position as
// scatter_group; no group boxes, so any position order costs the same.
template <bool REAL_ONLY, class RowFn>
__device__ __forceinline__ void scatter_ordered(RowFn&& rowptr, const float* __restrict__ scan,
                                                long nscan, float* __restrict__ re,
                                                float* __restrict__ im, int pw, int H, int W) {
  using T = std::conditional_t<REAL_ONLY, float, cf>;
  auto ld = [](const T* p) {
    if constexpr (REAL_ONLY) return mk(*p, 0.f);
    else return *p;
  };
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int nwave = (int)blockDim.x >> 6;
  const int lane = threadIdx.x & 63;
  constexpr int R = TK_GROWS + 1;
  const int Y0 = blockIdx.x * TK_GROWS;
  const int Xw = ((int)blockIdx.y * nwave + wave) * TK_GCOLS;  // first owned column (uniform)
  if (Y0 >= H || Xw >= W) return;
  const int X = Xw + lane - 1;  // lane 0: the halo column left of the first owned one
  float ar[TK_GROWS], ai[TK_GROWS];
#pragma unroll
  for (int k = 0; k < TK_GROWS; ++k) ar[k] = ai[k] = 0.f;
  for (long n = 0; n < nscan; ++n) {
    const float py = scan[2 * n], px = scan[2 * n + 1];
    const int sy = (int)floorf(py), sx = (int)floorf(px);
    // footprint rows [sy, sy + pw], columns [sx, sx + pw]: does it reach this
    // wave's pixels?  (uniform)
    if (sy > Y0 + TK_GROWS - 1 || sy + pw < Y0 || sx > Xw + TK_GCOLS - 1 || sx + pw < Xw) continue;
    const float fy = py - floorf(py), fx = px - floorf(px);
    const int xq = X - sx;
    const bool okx = (unsigned)xq < (unsigned)pw;
    const float wv = okx ? 1.0f - fx : 0.f;
    const float wl = (unsigned)(xq - 1) < (unsigned)pw ? fx : 0.f;
    const unsigned off = (unsigned)(okx ? xq : 0) * (unsigned)sizeof(T);
    const int y0 = Y0 - sy - 1;
    cf v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int y = y0 + j;
      const bool oky = y >= 0 && y < pw;
      const cf a = ld(tk_at(rowptr(n, oky ? y : 0), off));
      v[j] = oky ? a : mk(0.f, 0.f);
    }
    cf u[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const cf left = mk(tk_lane_down(v[j].x), REAL_ONLY ? 0.f : tk_lane_down(v[j].y));
      u[j] = mk(wv * v[j].x + wl * left.x, REAL_ONLY ? 0.f : wv * v[j].y + wl * left.y);
    }
#pragma unroll
    for (int k = 0; k < TK_GROWS; ++k) {
      ar[k] += (1.0f - fy) * u[k + 1].x + fy * u[k].x;
      if (!REAL_ONLY) ai[k] += (1.0f - fy) * u[k + 1].y + fy * u[k].y;
    }
  }
  if (lane > 0 && X < W) {
#pragma unroll
    for (int k = 0; k < TK_GROWS; ++k) {
      const int Y = Y0 + k;
      if (Y >= H) continue;
      const long ii = (long)Y * W + X;
      re[ii] += ar[k];
      if (!REAL_ONLY) im[ii] += ai[k];
    }
  }
}

// grid of the ordered form: (strips of the image, blocks of 4 x 63 columns)
static inline dim3 tk_ordered_grid(int H, int W) {
  return dim3((unsigned)((H + TK_GROWS - 1) / TK_GROWS),
              (unsigned)((W + 4 * TK_GCOLS - 1) / (4 * TK_GCOLS)));
}

__global__ __launch_bounds__(256) void scatter_patches_ordered_kernel(
    const cf* __restrict__ proj, const float* __restrict__ scan, float* __restrict__ acc,
    int nscan, int pw, int H, int W) {
  const long P = (long)pw * pw;
  scatter_ordered<false>([&](long n, int y) { return proj + n * P + (long)y * pw; }, scan, nscan,
                         acc, acc + (long)H * W, pw, H, W);
}

__global__ __launch_bounds__(256) void psi_precond_ordered_kernel(const float* __restrict__ amp,
                                                                  const float* __restrict__ scan,
                                                                  float* __restrict__ out,
                                                                  int nscan, int pw, int H, int W,
                                                                  long amp_stride) {
  scatter_ordered<true>([&](long n, int y) { return amp + n * amp_stride + (long)y * pw; }, scan,
                        nscan, out, out, pw, H, W);
}

// ----------------------------------------------------------- object gradient
// acc (2,H,W) planar f32 += scatter_n( objproj_n ),  objproj (nscan,pw,pw) c64 =
// sum_s conj(P_n,s) chi_n,s  computed by tike_lstsq_gradients
// (lstsq.py:510-520 = conj multiply + Patch.adj with nrepeat = S).
__global__ __launch_bounds__(1024) void scatter_patches_kernel(const cf* __restrict__ proj,
                                                               const float* __restrict__ scan,
                                                               float* __restrict__ acc, int nscan,
                                                               int pw, int H, int W, int wmax) {
  const long P = (long)pw * pw;
  float* __restrict__ re = acc;
  float* __restrict__ im = acc + (long)H * W;
  const long g = blockIdx.y;
  const long n0 = g * TK_GROUP, n1 = min((long)nscan, n0 + TK_GROUP);
  scatter_group<false>([&](long n, int y) { return proj + n * P + (long)y * pw; }, scan, n0, n1,
                       blockIdx.x, wmax, re, im, pw, H, W);
}

// (strips per group, widest box, threads per workgroup) of the grouped scatter
// for a probe width: one thread per box column, whole waves
static inline void tk_group_geometry(int pw, int* nstrip, int* wmax, int* threads) {
  *wmax = pw + 1 + TK_GSPREAD;
  *nstrip = (pw + 1 + TK_GSPREAD + TK_GROWS - 1) / TK_GROWS;
  const int t = (*wmax + TK_GCOLS - 1) / TK_GCOLS * 64;  // a wave covers TK_GCOLS columns
  *threads = t > 1024 ? 1024 : t;
}

extern "C" int tike_scatter_patches(const void* objproj, const float* scan, float* acc,
                                    int nscan, int pw, int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(objproj && scan && acc);
  if (tk_deterministic()) {
    hipLaunchKernelGGL(scatter_patches_ordered_kernel, tk_ordered_grid(H, W), dim3(256), 0,
                       (hipStream_t)stream, (const cf*)objproj, scan, acc, nscan, pw, H, W);
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  int nstrip, wmax, threads;
  tk_group_geometry(pw, &nstrip, &wmax, &threads);
  // groups of positions in gridDim.y, in slices of at most the device's limit
  TK_GRID_Y_LIMIT(ymax);
  const long span = ymax * TK_GROUP, P = (long)pw * pw;
  for (long lo = 0; lo < nscan; lo += span) {
    const int m = (int)(nscan - lo < span ? nscan - lo : span);
    const dim3 grid(nstrip, (m + TK_GROUP - 1) / TK_GROUP);
    hipLaunchKernelGGL(scatter_patches_kernel, grid, dim3(threads), 0, (hipStream_t)stream,
                       (const cf*)objproj + lo * P, scan + 2 * lo, acc, m, pw, H, W, wmax);
  }
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ------------------------------------------------------ psi preconditioner
// out (H,W) float32 += scatter_n( probe_amp ),  probe_amp = sum_s |probe_s|^2 (pw,pw) f32
// (solvers/_preconditioner.py:48-104: Patch.adj of one broadcast patch).
__global__ __launch_bounds__(1024) void psi_precond_kernel(const float* __restrict__ amp,
                                                           const float* __restrict__ scan,
                                                           float* __restrict__ out, int nscan,
                                                           int pw, int H, int W, int wmax) {
  const long g = blockIdx.y;
  const long n0 = g * TK_GROUP, n1 = min((long)nscan, n0 + TK_GROUP);
  scatter_group<true>([&](long, int y) { return amp + (long)y * pw; }, scan, n0, n1,
                      blockIdx.x, wmax, out, out, pw, H, W);
}

extern "C" int tike_psi_preconditioner(const float* probe_amp, const float* scan, void* out,
                                       int nscan, int pw, int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(probe_amp && scan && out);
  if (tk_deterministic()) {
    hipLaunchKernelGGL(psi_precond_ordered_kernel, tk_ordered_grid(H, W), dim3(256), 0,
                       (hipStream_t)stream, probe_amp, scan, (float*)out, nscan, pw, H, W, 0L);
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  int nstrip, wmax, threads;
  tk_group_geometry(pw, &nstrip, &wmax, &threads);
  TK_GRID_Y_LIMIT(ymax);  // groups in gridDim.y, in slices of at most the limit
  const long span = ymax * TK_GROUP;
  for (long lo = 0; lo < nscan; lo += span) {
    const int m = (int)(nscan - lo < span ? nscan - lo : span);
    const dim3 grid(nstrip, (m + TK_GROUP - 1) / TK_GROUP);
    hipLaunchKernelGGL(psi_precond_kernel, grid, dim3(threads), 0, (hipStream_t)stream,
                       probe_amp, scan + 2 * lo, (float*)out, m, pw, H, W, wmax);
  }
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// out (H,W) float32 += scatter_n( amp_n ), amp (nscan,pw,pw) f32: one real
// patch PER POSITION (the illumination of a slice behind the first of a
// multislice object, _preconditioner.py:82-95).
__global__ __launch_bounds__(1024) void scatter_amplitudes_kernel(const float* __restrict__ amp,
                                                                  const float* __restrict__ scan,
                                                                  float* __restrict__ out,
                                                                  int nscan, int pw, int H, int W,
                                                                  int wmax) {
  const long P = (long)pw * pw;
  const long g = blockIdx.y;
  const long n0 = g * TK_GROUP, n1 = min((long)nscan, n0 + TK_GROUP);
  scatter_group<true>([&](long n, int y) { return amp + n * P + (long)y * pw; }, scan, n0, n1,
                      blockIdx.x, wmax, out, out, pw, H, W);
}

extern "C" int tike_scatter_amplitudes(const float* amp, const float* scan, float* out,
                                       int nscan, int pw, int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(amp && scan && out);
  if (tk_deterministic()) {
    hipLaunchKernelGGL(psi_precond_ordered_kernel, tk_ordered_grid(H, W), dim3(256), 0,
                       (hipStream_t)stream, amp, scan, out, nscan, pw, H, W, (long)pw * pw);
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  int nstrip, wmax, threads;
  tk_group_geometry(pw, &nstrip, &wmax, &threads);
  TK_GRID_Y_LIMIT(ymax);  // groups in gridDim.y, in slices of at most the limit
  const long span = ymax * TK_GROUP, P = (long)pw * pw;
  for (long lo = 0; lo < nscan; lo += span) {
    const int m = (int)(nscan - lo < span ? nscan - lo : span);
    const dim3 grid(nstrip, (m + TK_GROUP - 1) / TK_GROUP);
    hipLaunchKernelGGL(scatter_amplitudes_kernel, grid, dim3(threads), 0, (hipStream_t)stream,
                       amp + lo * P, scan + 2 * lo, out, m, pw, H, W, wmax);
  }
  TK_LAUNCH_CHECK();
  return TK_OK;
}
