// The kernels the differentiable intensity models (tike_amd/autograd.py) add
// to the operators: the upstream gradient applied to a far plane, and the
// EXACT gradient of the bilinear patch gather with respect to the scan
// positions, for one slice and summed over the slices of a multislice object.
// No reference counterpart: the reference takes its derivatives from
// hand-written adjoints and has no d/d scan.
//
//   tike_farplane_scale        farplane[f][j][p] *= scale * table[f][p]
//   tike_scan_gradient         grad[n] = sum_px Re( (Dy_n, Dx_n) conj(objproj_n) )
//   tike_scan_gradient_slices  grad[n] = sum_d sum_px Re( (Dy_n,d, Dx_n,d) conj(objproj_d,n) )
//
// Byte models.  tike_farplane_scale, per frame of P planes of npix pixels:
// P * npix * 8 bytes of far plane read once and written once, npix * 4 bytes
// of table.  tike_scan_gradient, per position: pw^2 * 8 bytes of objproj read
// once and (pw + 1)^2 * 8 bytes of object (mostly served from cache: the
// footprints of neighbouring positions overlap), 8 bytes written;
// tike_scan_gradient_slices reads that much per slice and writes 8 bytes.
#include "../../include/tike_amd.h"
#include "frame_lanes.h"
#include "patch_taps.h"

namespace {

constexpr int AG_PX = 4;  // pixels of a lane: two 16-byte far-plane accesses per plane

// A lane owns AG_PX consecutive pixels of one frame: their factors are loaded
// once and stay in registers over the P planes.  The last npix % AG_PX pixels
// of a frame are taken one per lane by the lanes behind the last vector.
// `bpf` workgroups serve a frame.
__global__ __launch_bounds__(256) void farplane_scale_kernel(cf* __restrict__ farplane,
                                                             const float* __restrict__ table,
                                                             int P, long npix, float scale,
                                                             long bpf) {
  const long f = (long)blockIdx.x / bpf;
  const long v = ((long)blockIdx.x % bpf) * blockDim.x + threadIdx.x;
  cf* __restrict__ F = farplane + f * P * npix;
  const float* __restrict__ T = table + f * npix;
  const long nvec = npix / AG_PX;
  if (v < nvec) {
    const long p = v * AG_PX;
    tk_f4a4 t = *reinterpret_cast<const tk_f4a4*>(T + p);
    t *= scale;
#pragma unroll 4
    for (int j = 0; j < P; ++j) {
      cf* at = F + j * npix + p;
      tk_f4a8 a = *reinterpret_cast<const tk_f4a8*>(at);
      tk_f4a8 b = *reinterpret_cast<const tk_f4a8*>(at + 2);
      a.x *= t.x, a.y *= t.x, a.z *= t.y, a.w *= t.y;
      b.x *= t.z, b.y *= t.z, b.z *= t.w, b.w *= t.w;
      *reinterpret_cast<tk_f4a8*>(at) = a;
      *reinterpret_cast<tk_f4a8*>(at + 2) = b;
    }
    return;
  }
  // scalar tail: fewer than AG_PX pixels, one per lane
  const long p = nvec * AG_PX + (v - nvec);
  if (p >= npix) return;
  const float t = T[p] * scale;
  for (int j = 0; j < P; ++j) F[j * npix + p] = F[j * npix + p] * t;
}

constexpr int AG_COLS = 63;  // patch columns of a wave: lane 63 is the halo lane
constexpr int AG_ROWS = 8;   // patch rows of a strip

// The lanes' float64 sums of a position into out[0 ... 1], in a fixed order: wave
// shuffles, then the four waves through LDS.
__device__ __forceinline__ void ag_store_sums(double gy, double gx, int wave, int lane,
                                              double (&red)[4][2], float* out) {
  gy = tk_wave_sum(gy);
  gx = tk_wave_sum(gx);
  if (lane == 0) {
    red[wave][0] = gy;
    red[wave][1] = gx;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int i = threadIdx.x;
    out[i] = (float)((red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
  }
}

// One workgroup per position.  The halo-LANE scheme of patch_taps.h over the
// (pw, pw) patch, its items dealt to the four waves in turn; a row of a strip
// serves Dy and Dx alike.
//
// The products are float32; the sums are float64 in a fixed order (lane, wave
// shuffles, the four waves through LDS).  The terms cancel over the patch down
// to a thousandth of their absolute sum, so float32 rounding of a running sum,
// harmless against the terms, is not harmless against the result
// (position_pd.hip has the same reason).
__global__ __launch_bounds__(256) void scan_gradient_kernel(const cf* __restrict__ objproj,
                                                            const float* __restrict__ scan,
                                                            const cf* __restrict__ psi,
                                                            float* __restrict__ grad, int pw,
                                                            int H, int W) {
  __shared__ double red[4][2];
  const long n = blockIdx.x;
  const cf* __restrict__ q = objproj + n * pw * pw;
  const float py = scan[2 * n], px = scan[2 * n + 1];
  const float fy0 = floorf(py), fx0 = floorf(px);
  const float fy = py - fy0, fx = px - fx0;
  const long sy = (long)fy0, sx = (long)fx0;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (pw + AG_COLS - 1) / AG_COLS;
  const int nstrip = (pw + AG_ROWS - 1) / AG_ROWS;
  double gy = 0., gx = 0.;
  for (int item = wave; item < nseg * nstrip; item += 4) {  // uniform in a wave
    const int x = (item % nseg) * AG_COLS + lane;  // patch column; x == pw: the last right tap
    const int y0 = (item / nseg) * AG_ROWS;
    const long X = sx + x;
    const bool okx = X >= 0 && X < W;
    const long Xc = X < 0 ? 0 : (X < W ? X : W - 1);
    const bool pixel = lane < AG_COLS && x < pw;
    const int xq = x < pw ? x : pw - 1;
    cf o[AG_ROWS + 1], qq[AG_ROWS];
#pragma unroll
    for (int j = 0; j <= AG_ROWS; ++j) {
      const long Y = sy + y0 + j;
      const bool ok = okx && Y >= 0 && Y < H;
      const long Yc = Y < 0 ? 0 : (Y < H ? Y : H - 1);
      const cf v = psi[Yc * W + Xc];
      o[j] = ok ? v : mk(0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < AG_ROWS; ++j) {
      const int yq = y0 + j < pw ? y0 + j : pw - 1;
      qq[j] = tk_ld_stream(q + (long)yq * pw + xq);
    }
    cf right = tk_cf_lane_up(o[0]);
#pragma unroll
    for (int j = 0; j < AG_ROWS; ++j) {
      const cf o00 = o[j], o01 = right, o10 = o[j + 1];
      const cf o11 = tk_cf_lane_up(o10);
      right = o11;
      const float dyr = tk_slope(fx, o00.x, o10.x, o01.x, o11.x);
      const float dyi = tk_slope(fx, o00.y, o10.y, o01.y, o11.y);
      const float dxr = tk_slope(fy, o00.x, o01.x, o10.x, o11.x);
      const float dxi = tk_slope(fy, o00.y, o01.y, o10.y, o11.y);
      const float ty = dyr * qq[j].x + dyi * qq[j].y;  // Re(Dy conj(objproj))
      const float tx = dxr * qq[j].x + dxi * qq[j].y;
      const bool live = pixel && y0 + j < pw;
      gy += live ? (double)ty : 0.;
      gx += live ? (double)tx : 0.;
    }
  }
  ag_store_sums(gy, gx, wave, lane, red, grad + 2 * n);
}

// The same sum over the D slices of a multislice object, slice d with its own
// objproj plane (`slice_stride` elements apart) and its own object (H, W): one
// workgroup per position walks the slices OUTERMOST with the items of
// scan_gradient_kernel, every lane keeping ONE float64 running sum per
// coordinate over all slices and pixels, reduced once at the end -- so D == 1
// gives the bits of scan_gradient_kernel, and there is no float32 rounding
// between two slices.  All offsets are `long`: d * slice_stride + n * pw * pw
// passes 2^31.
__global__ __launch_bounds__(256) void scan_gradient_slices_kernel(
    const cf* __restrict__ objproj, long slice_stride, const float* __restrict__ scan,
    const cf* __restrict__ psi, float* __restrict__ grad, int D, int pw, int H, int W) {
  __shared__ double red[4][2];
  const long n = blockIdx.x;
  const float py = scan[2 * n], px = scan[2 * n + 1];
  const float fy0 = floorf(py), fx0 = floorf(px);
  const float fy = py - fy0, fx = px - fx0;
  const long sy = (long)fy0, sx = (long)fx0;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (pw + AG_COLS - 1) / AG_COLS;
  const int nstrip = (pw + AG_ROWS - 1) / AG_ROWS;
  double gy = 0., gx = 0.;
  for (int d = 0; d < D; ++d) {
    const cf* __restrict__ q = objproj + (long)d * slice_stride + n * pw * pw;
    const cf* __restrict__ img = psi + (long)d * H * W;
    for (int item = wave; item < nseg * nstrip; item += 4) {  // uniform in a wave
      const int x = (item % nseg) * AG_COLS + lane;  // patch column; x == pw: the last right tap
      const int y0 = (item / nseg) * AG_ROWS;
      const long X = sx + x;
      const bool okx = X >= 0 && X < W;
        const long Xc = X < 0 ? 0 : (X < W ? X : W - 1);
      const bool pixel = lane < AG_COLS && x < pw;
      const int xq = x < pw ? x : pw - 1;
      cf o[AG_ROWS + 1], qq[AG_ROWS];
#pragma unroll
      for (int j = 0; j <= AG_ROWS; ++j) {
        const long Y = sy + y0 + j;
        const bool ok = okx && Y >= 0 && Y < H;
        const long Yc = Y < 0 ? 0 : (Y < H ? Y : H - 1);
        const cf v = img[Yc * W + Xc];
        o[j] = ok ? v : mk(0.f, 0.f);
      }
#pragma unroll
      for (int j = 0; j < AG_ROWS; ++j) {
        const int yq = y0 + j < pw ? y0 + j : pw - 1;
        qq[j] = tk_ld_stream(q + (long)yq * pw + xq);
      }
      cf right = tk_cf_lane_up(o[0]);
#pragma unroll
      for (int j = 0; j < AG_ROWS; ++j) {
        const cf o00 = o[j], o01 = right, o10 = o[j + 1];
        const cf o11 = tk_cf_lane_up(o10);
        right = o11;
        const float dyr = tk_slope(fx, o00.x, o10.x, o01.x, o11.x);
        const float dyi = tk_slope(fx, o00.y, o10.y, o01.y, o11.y);
        const float dxr = tk_slope(fy, o00.x, o01.x, o10.x, o11.x);
        const float dxi = tk_slope(fy, o00.y, o01.y, o10.y, o11.y);
        const float ty = dyr * qq[j].x + dyi * qq[j].y;  // Re(Dy conj(objproj))
        const float tx = dxr * qq[j].x + dxi * qq[j].y;
        const bool live = pixel && y0 + j < pw;
        gy += live ? (double)ty : 0.;
        gx += live ? (double)tx : 0.;
      }
    }
  }
  ag_store_sums(gy, gx, wave, lane, red, grad + 2 * n);
}

}  // namespace

extern "C" int tike_farplane_scale(void* farplane, const float* table, long nframe, int P,
                                   long npix, float scale, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && table);
  TK_CHECK_ARG(nframe >= 0 && P >= 1 && npix >= 1);
  if (nframe == 0) return TK_OK;
  // lanes of a frame: one per vector of AG_PX pixels, one per pixel of the tail
  const long lanes = npix / AG_PX + npix % AG_PX;
  const long bpf = (lanes + 255) / 256;
  TK_CHECK_ARG(bpf <= 0x7fffffffL / nframe);  // the workgroups of all frames: grid.x
  hipLaunchKernelGGL(farplane_scale_kernel, dim3((unsigned)(nframe * bpf)), dim3(256), 0, stream,
                     (cf*)farplane, table, P, npix, scale, bpf);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_scan_gradient(const void* objproj, const float* scan, const void* psi,
                                  float* grad, long nscan, int pw, int H, int W,
                                  void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(objproj && scan && psi && grad);
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one workgroup per position: grid.x
  hipLaunchKernelGGL(scan_gradient_kernel, dim3((unsigned)nscan), dim3(256), 0, stream,
                     (const cf*)objproj, scan, (const cf*)psi, grad, pw, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_scan_gradient_slices(const void* objproj, long slice_stride,
                                         const float* scan, const void* psi, float* grad,
                                         long nscan, int D, int pw, int H, int W,
                                         void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(objproj && scan && psi && grad);
  TK_CHECK_ARG(nscan >= 0 && D >= 1 && pw >= 1 && H >= 1 && W >= 1);
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one workgroup per position: grid.x
  TK_CHECK_ARG(slice_stride >= nscan * pw * pw);  // the planes do not overlap
  if (nscan == 0) return TK_OK;
  hipLaunchKernelGGL(scan_gradient_slices_kernel, dim3((unsigned)nscan), dim3(256), 0, stream,
                     (const cf*)objproj, slice_stride, scan, (const cf*)psi, grad, D, pw, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
