// The two ends of the exit-wave step of the difference map
// (tike_amd/ptycho/solvers/dm.py; Thibault et al. 2008 / 2009; no reference
// counterpart).  The solver keeps one exit wave per position and mode,
// waves (nscan, S, pw, pw); with O_n the bilinear patch of the object at
// position n, P_s the shared probe and a the relaxation:
//
//   tike_dm_reflect  nearplane[n][s] = pad( (1 + a) P_s O_n - a waves[n][s] )
//                    (waves == NULL: the waves ARE P O, so pad(P_s O_n))
//   tike_dm_update   waves[n][s] <- (1 - a) waves[n][s] + a P_s O_n
//                                   + crop(chi[n][s])
//                    change[n] = sum_{s, pixels} |new - old|^2   (optional)
//
// Between the two: forward transform, modulus projection
// (tike_farplane_gradient) and inverse transform of the padded planes.
//
// Both are streaming kernels of the halo-COLUMN scheme of patch_taps.h with
// TWO columns per lane: an item is DM_ROWS rows x 128 columns, one per wave;
// a lane owns the columns x, x + 1 of its item, so that every access along a
// row is 16 bytes (two cf), and its strip of DM_ROWS + 1 object rows serves
// every mode.  The tap to the right of column x + 1 is column x of the next
// lane (wave shuffle); lane 63 takes it from the halo column.
//
// Byte models, per position.  tike_dm_reflect: S det^2 8 bytes written once
// (the window and the zeros around it), S pw^2 8 bytes of waves read once
// (none with waves == NULL), (pw + 1)^2 8 bytes of object taps (mostly from
// cache: the footprints of neighbouring positions overlap), S pw^2 8 bytes
// of probe (from cache: every position reads the same planes), 8 bytes of
// scan.  tike_dm_update: S pw^2 8 bytes of waves read and as many written,
// the S pw det 8 bytes of the window's rows of chi read (whole cache lines),
// object taps, probe and scan as above; 8 bytes of change.
#include <cmath>

#include "../../include/tike_amd.h"
#include "frame_lanes.h"
#include "patch_taps.h"

namespace {

constexpr int DM_LANE_COLS = 2;                // columns of a lane: one 16-byte access
constexpr int DM_COLS = 64 * DM_LANE_COLS;     // columns of an item
// Rows of a strip.  Measured at 256^2 x 8 modes and 128^2 x 4 modes
// (profiles/dm.md): 16 / 8 / 4 / 2 / 1 rows put tike_dm_update at 0.25 / 0.40
// / 0.57 / 0.61 / 0.61 of the roofline and tike_dm_reflect at 0.36 / 0.47 /
// 0.66 / 0.62 / 0.63 -- the rows a lane holds for all three streams cost
// registers (254 VGPRs at 8 rows, 78 at 2), and these kernels live on the
// number of waves in flight; the object rows a short strip loads again come
// from cache.
constexpr int DM_ROWS = 2;

// Elements x and x + 1 of a row of n elements: ONE 16-byte load whose address
// is clamped into the row (pair base in [0, n - 2]) and whose halves are
// selected; an element outside the row counts as zero.  Unconditional: no
// load leaves the row, whatever x.  (n == 1, uniform: the row's only element.)
__device__ __forceinline__ void dm_ld2(const cf* row, long x, int n, cf& v0, cf& v1) {
  const cf zero = mk(0.f, 0.f);
  if (n < 2) {
    const cf a = row[0];
    v0 = x == 0 ? a : zero;
    v1 = x + 1 == 0 ? a : zero;
    return;
  }
  const long xb = x < 0 ? 0 : (x < n - 1 ? x : n - 2);
  const tk_f4a8 q = *reinterpret_cast<const tk_f4a8*>(row + xb);
  const cf lo = mk(q[0], q[1]), hi = mk(q[2], q[3]);
  v0 = x == xb ? lo : (x == xb + 1 ? hi : zero);
  v1 = x + 1 == xb ? lo : (x == xb ? hi : zero);
}

// Elements x >= 0 and x + 1 of a row of n elements written: 16 bytes where
// both lie in the row, 8 for the last element of a row of odd length.
__device__ __forceinline__ void dm_st2(cf* row, int x, int n, cf v0, cf v1) {
  if (x + 1 < n) {
    tk_f4a8 q;
    q[0] = v0.x, q[1] = v0.y, q[2] = v1.x, q[3] = v1.y;
    *reinterpret_cast<tk_f4a8*>(row + x) = q;
  } else if (x < n) {
    row[x] = v0;
  }
}

// The patch pixels (py0 + j, px) and (py0 + j, px + 1), j < DM_ROWS, of
// position corner c: the strip of DM_ROWS + 1 object rows, two columns per
// lane in one load, the halo column behind the item (row min(lane, DM_ROWS)
// per lane).  pxh: the patch column behind the item.  A tap outside the
// object counts as zero.
__device__ __forceinline__ void dm_patch_pairs(const cf* __restrict__ psi, const TkCorner& c,
                                               int px, int pxh, int py0, int lane, int H, int W,
                                               cf (&pat0)[DM_ROWS], cf (&pat1)[DM_ROWS]) {
  const cf zero = mk(0.f, 0.f);
  const long X = (long)c.sx + px;
  cf a[DM_ROWS + 1], b[DM_ROWS + 1];
#pragma unroll
  for (int j = 0; j <= DM_ROWS; ++j) {
    const long Y = (long)c.sy + py0 + j;
    const bool ok = Y >= 0 && Y < H;
    const long Yc = Y < 0 ? 0 : (Y < H ? Y : H - 1);
    cf v0, v1;
    dm_ld2(psi + Yc * W, X, W, v0, v1);
    a[j] = ok ? v0 : zero;
    b[j] = ok ? v1 : zero;
  }
  cf halo;
  {
    const long XH = (long)c.sx + pxh;
    const long Y = (long)c.sy + py0 + (lane < DM_ROWS ? lane : DM_ROWS);
    const bool ok = XH >= 0 && XH < W && Y >= 0 && Y < H;
    const long XHc = XH < 0 ? 0 : (XH < W ? XH : W - 1);
    const long Yc = Y < 0 ? 0 : (Y < H ? Y : H - 1);
    const cf v = psi[Yc * W + XHc];
    halo = ok ? v : zero;
  }
  cf right = tk_right_tap<64>(a[0], halo, 0, lane);
#pragma unroll
  for (int j = 0; j < DM_ROWS; ++j) {
    const cf below = tk_right_tap<64>(a[j + 1], halo, j + 1, lane);
    pat0[j] = tk_bilinear(a[j], b[j], a[j + 1], b[j + 1], c);
    pat1[j] = tk_bilinear(b[j], right, b[j + 1], below, c);
    right = below;
  }
}

// grid (position, group of four items) over the (det, det) plane.  A pixel
// outside the centred pw window is written as exactly 0.0; an item that lies
// in the padding altogether only writes its zeros.  Every output element has
// one owner and is written once: no atomics, no memset.  All offsets `long`.
__global__ __launch_bounds__(256) void dm_reflect_kernel(
    const cf* __restrict__ psi, const float* __restrict__ scan, const cf* __restrict__ probe,
    const cf* __restrict__ waves, cf* __restrict__ nearplane, float relaxation, int S, int pw,
    int det, int H, int W) {
  // waves == NULL must give the bits of waves = P O: the product is rounded
  // before the wave is taken from it, so that P O - waves is exactly zero
  // there.  With contraction the difference would come from a fused
  // multiply-add on the unrounded product.
#pragma clang fp contract(off)
  const long n = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (det + DM_COLS - 1) / DM_COLS;
  const int nstrip = (det + DM_ROWS - 1) / DM_ROWS;
  const int item = (int)blockIdx.y * 4 + wave;  // uniform in a wave
  if (item >= nseg * nstrip) return;
  const int pad = (det - pw) / 2;
  const int dx0 = (item % nseg) * DM_COLS;
  const int dy0 = (item / nseg) * DM_ROWS;
  const int dx = dx0 + DM_LANE_COLS * lane;
  const int px = dx - pad, px0 = dx0 - pad, py0 = dy0 - pad;
  const long plane = (long)det * det;
  const long pp = (long)pw * pw;
  const cf zero = mk(0.f, 0.f);
  cf* __restrict__ dst = nearplane + n * S * plane;
  if (py0 + DM_ROWS <= 0 || py0 >= pw || px0 + DM_COLS <= 0 || px0 >= pw) {
    // padding only (uniform in a wave)
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < DM_ROWS; ++j)
        if (dy0 + j < det) dm_st2(dst + s * plane + (long)(dy0 + j) * det, dx, det, zero, zero);
    return;
  }
  const TkCorner c = tk_corner(scan, n);
  cf pat0[DM_ROWS], pat1[DM_ROWS];
  dm_patch_pairs(psi, c, px, px0 + DM_COLS, py0, lane, H, W, pat0, pat1);
  const bool in0 = px >= 0 && px < pw, in1 = px + 1 >= 0 && px + 1 < pw;
  const cf* wsrc = waves != nullptr ? waves + n * S * pp : nullptr;
  for (int s = 0; s < S; ++s) {
    cf r0[DM_ROWS], r1[DM_ROWS];
#pragma unroll
    for (int j = 0; j < DM_ROWS; ++j) {
      const int py = py0 + j;
      const long row = s * pp + (long)(py < 0 ? 0 : (py < pw ? py : pw - 1)) * pw;
      cf p0, p1;
      dm_ld2(probe + row, px, pw, p0, p1);
      r0[j] = pat0[j] * p0;
      r1[j] = pat1[j] * p1;
      if (wsrc != nullptr) {  // uniform
        cf w0, w1;
        dm_ld2(wsrc + row, px, pw, w0, w1);
        // P O + a (P O - waves): exactly P O where the waves are P O
        r0[j] = r0[j] + (r0[j] - w0) * relaxation;
        r1[j] = r1[j] + (r1[j] - w1) * relaxation;
      }
    }
#pragma unroll
    for (int j = 0; j < DM_ROWS; ++j) {
      const int py = py0 + j;
      const bool rowin = py >= 0 && py < pw;
      if (dy0 + j < det)
        dm_st2(dst + s * plane + (long)(dy0 + j) * det, dx, det, rowin && in0 ? r0[j] : zero,
               rowin && in1 ? r1[j] : zero);
    }
  }
}

// grid (position, groups) over the (pw, pw) plane of the waves; a wave walks
// the items blockIdx.y * 4 + wave, + 4 gridDim.y, ...  With CHANGE the grid
// has ONE workgroup per position, so that the sum of a position has one owner
// and a fixed order: a lane sums its float32 products |new - old|^2 in
// float64 over its items, modes, rows and two columns in that order, the 64
// lanes by the xor tree of tk_wave_sum, the four waves in order.  The
// elements of a mode that a lane owns are loaded before the first of them is
// stored, and what a clamped address makes a lane load beside them is never
// used: every element of waves is read by its one owner before that owner
// writes it.
template <bool CHANGE>
__global__ __launch_bounds__(256) void dm_update_kernel(
    cf* waves, const cf* __restrict__ chi, const cf* __restrict__ psi,
    const float* __restrict__ scan, const cf* __restrict__ probe, float relaxation,
    double* __restrict__ change, int S, int pw, int det, int H, int W) {
  const long n = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (pw + DM_COLS - 1) / DM_COLS;
  const int nstrip = (pw + DM_ROWS - 1) / DM_ROWS;
  const int pad = (det - pw) / 2;
  const long plane = (long)det * det;
  const long pp = (long)pw * pw;
  const TkCorner c = tk_corner(scan, n);
  cf* dst = waves + n * S * pp;
  const cf* __restrict__ csrc = chi + n * S * plane;
  double total = 0.0;
  for (int item = (int)blockIdx.y * 4 + wave; item < nseg * nstrip;
       item += 4 * (int)gridDim.y) {  // uniform in a wave
    const int px0 = (item % nseg) * DM_COLS;
    const int py0 = (item / nseg) * DM_ROWS;
    const int px = px0 + DM_LANE_COLS * lane;
    cf pat0[DM_ROWS], pat1[DM_ROWS];
    dm_patch_pairs(psi, c, px, px0 + DM_COLS, py0, lane, H, W, pat0, pat1);
    for (int s = 0; s < S; ++s) {
      cf n0[DM_ROWS], n1[DM_ROWS];
#pragma unroll
      for (int j = 0; j < DM_ROWS; ++j) {
        const int py = py0 + j;
        const int pyc = py < pw ? py : pw - 1;
        const long row = s * pp + (long)pyc * pw;
        cf p0, p1, w0, w1, x0, x1;
        dm_ld2(probe + row, px, pw, p0, p1);
        dm_ld2(dst + row, px, pw, w0, w1);
        dm_ld2(csrc + s * plane + (long)(pyc + pad) * det, (long)px + pad, det, x0, x1);
        // the step a (P O - waves) + chi, then waves + step
        const cf d0 = (pat0[j] * p0 - w0) * relaxation + x0;
        const cf d1 = (pat1[j] * p1 - w1) * relaxation + x1;
        n0[j] = w0 + d0;
        n1[j] = w1 + d1;
        if (CHANGE) {
          if (py < pw && px < pw) total += (double)(d0.x * d0.x + d0.y * d0.y);
          if (py < pw && px + 1 < pw) total += (double)(d1.x * d1.x + d1.y * d1.y);
        }
      }
#pragma unroll
      for (int j = 0; j < DM_ROWS; ++j)
        if (py0 + j < pw) dm_st2(dst + s * pp + (long)(py0 + j) * pw, px, pw, n0[j], n1[j]);
    }
  }
  if (CHANGE) {
    __shared__ double red[4];
    total = tk_wave_sum(total);
    if (lane == 0) red[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) change[n] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

bool dm_args_ok(const void* a, const void* b, const void* c, const void* d, float relaxation,
                long nscan, int S, int pw, int det, int H, int W) {
  return a && b && c && d && std::isfinite(relaxation) && nscan >= 0 && S >= 1 && pw >= 1 &&
         det >= pw && H >= 1 && W >= 2;
}

}  // namespace

extern "C" int tike_dm_reflect(const void* psi, const float* scan, const void* probe,
                               const void* waves, void* nearplane, float relaxation, long nscan,
                               int S, int pw, int det, int H, int W, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(dm_args_ok(psi, scan, probe, nearplane, relaxation, nscan, S, pw, det, H, W));
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one grid column per position: grid.x
  const long groups = tk_item_groups(det, DM_COLS, DM_ROWS);
  TK_CHECK_ARG(groups > 0);
  hipLaunchKernelGGL(dm_reflect_kernel, dim3((unsigned)nscan, (unsigned)groups), dim3(256), 0,
                     stream, (const cf*)psi, scan, (const cf*)probe, (const cf*)waves,
                     (cf*)nearplane, relaxation, S, pw, det, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_dm_update(void* waves, const void* chi, const void* psi, const float* scan,
                              const void* probe, float relaxation, double* change, long nscan,
                              int S, int pw, int det, int H, int W, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(waves && dm_args_ok(chi, psi, scan, probe, relaxation, nscan, S, pw, det, H, W));
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one grid column per position: grid.x
  const long groups = tk_item_groups(pw, DM_COLS, DM_ROWS);
  TK_CHECK_ARG(groups > 0);
  if (change != nullptr)
    hipLaunchKernelGGL(dm_update_kernel<true>, dim3((unsigned)nscan, 1u), dim3(256), 0, stream,
                       (cf*)waves, (const cf*)chi, (const cf*)psi, scan, (const cf*)probe,
                       relaxation, change, S, pw, det, H, W);
  else
    hipLaunchKernelGGL(dm_update_kernel<false>, dim3((unsigned)nscan, (unsigned)groups),
                       dim3(256), 0, stream, (cf*)waves, (const cf*)chi, (const cf*)psi, scan,
                       (const cf*)probe, relaxation, change, S, pw, det, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
