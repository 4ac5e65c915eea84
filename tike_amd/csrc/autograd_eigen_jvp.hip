// The kernel of the FORWARD-mode derivative of the differentiable intensity
// model with a varying probe (tike_amd/autograd.py: eigen_intensity_jvp): the
// tangent of the exit waves for tangents of the object, the positions, the
// shared probe, the eigen probes and their weights.  It does for the varying
// probe of tike_eigen_probe_gradients (autograd_eigen.hip; reference
// probe.py:272-303, get_varying_probe) what tike_conv_fwd_tangent
// (autograd_jvp.hip) does for the shared probe; the tangent far plane comes
// from tike_fft2 and the tangent intensity from tike_intensity_tangent.  No
// reference counterpart: the reference differentiates neither the eigen
// probes nor their weights.
//
//   tike_eigen_wave_tangent, with C = num_eigen, M = eigen_modes:
//     P[n][s]  = w[n][0][s] probe[s] + sum_c w[n][c+1][s] E[c][s]         (s < M; else the first term)
//     dP[n][s] = w[n][0][s] dprobe[s] + dw[n][0][s] probe[s]
//              + sum_c ( w[n][c+1][s] dE[c][s] + dw[n][c+1][s] E[c][s] )  (sum only for s < M)
//     dpatch_n = patch_n(dpsi) + dscan[n][0] Dy_n(psi) + dscan[n][1] Dx_n(psi)
//     nearplane[n][s] = pad( dpatch_n P[n][s] + patch_n(psi) dP[n][s] )
//
// Byte model, per position: S * det^2 * 8 bytes written once (the window and
// the zeros around it) -- what bounds the kernel; (pw + 1)^2 * 8 bytes of
// object read, twice that with dpsi (mostly from cache: the footprints of
// neighbouring positions overlap); (S + C M) * pw^2 * 8 bytes of probe and
// eigen probes, twice that with dprobe and deigen_probe (from cache: every
// position reads the same planes); (C + 1) * S * 4 bytes of weights and as
// many of their tangent (scalar loads, S + C M of them used); 8 bytes of scan
// and 8 of dscan.  P and dP are never in memory: a per-position P would add
// two more trips of the size of the writes.
#include "../../include/tike_amd.h"
#include "patch_taps.h"

namespace {

constexpr int EW_MAX_MODES = 16;   // S: TK_MAX_MODES of the gradient kernels
constexpr int EW_MAX_PLANES = 16;  // C * M, as tike_eigen_probe_gradients
constexpr int EW_COLS = 64;        // detector columns of an item: every lane owns one
constexpr int EW_ROWS = 8;         // detector rows of a strip

// grid (position, group of four items): the halo-COLUMN scheme of
// patch_taps.h laid over the (det, det) DETECTOR plane, one item per wave: all
// 64 lanes own a column.  The strips of psi and of dpsi serve the patch, Dy, Dx
// and every mode.  The modes are the outer loop: w[n][:][s] and dw[n][:][s] are
// uniform in a workgroup (scalar loads), and P and dP of a pixel are built in
// registers from probe, E, dprobe and dE, which come from cache.  Rows c + 1
// of w and dw are not read for s >= M.  A NULL tangent is a zero tangent: its
// loads are skipped (uniform) and its terms are left out or computed on
// zeros; with all five NULL the plane is written as exactly 0.0 and nothing
// is loaded.  A pixel outside the centred pw window is written as exactly 0.0;
// an item that lies in the padding altogether only writes its zeros.  Every
// output element has one owner: no atomics.  All offsets are `long`.
__global__ __launch_bounds__(256) void eigen_wave_tangent_kernel(
    const cf* __restrict__ psi, const cf* __restrict__ dpsi, const float* __restrict__ scan,
    const float* __restrict__ dscan, const cf* __restrict__ probe, const cf* __restrict__ dprobe,
    const cf* __restrict__ eigen, const cf* __restrict__ deigen, const float* __restrict__ weights,
    const float* __restrict__ dweights, int C, int M, cf* __restrict__ nearplane, int S, int pw,
    int det, int H, int W) {
  const long n = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (det + EW_COLS - 1) / EW_COLS;
  const int nstrip = (det + EW_ROWS - 1) / EW_ROWS;
  const int item = (int)blockIdx.y * 4 + wave;  // uniform in a wave
  if (item >= nseg * nstrip) return;
  const int pad = (det - pw) / 2;
  const int dx0 = (item % nseg) * EW_COLS;
  const int dy0 = (item / nseg) * EW_ROWS;
  const int dx = dx0 + lane;  // detector column
  const int px = dx - pad, px0 = dx0 - pad, py0 = dy0 - pad;
  const bool owner = dx < det;
  const long plane = (long)det * det;
  cf* __restrict__ dst = nearplane + n * S * plane + (long)dx;
  const bool none = dpsi == nullptr && dscan == nullptr && dprobe == nullptr &&
                    dweights == nullptr && (deigen == nullptr || C == 0);
  if (none || py0 + EW_ROWS <= 0 || py0 >= pw || px0 + EW_COLS <= 0 || px0 >= pw) {
    // no tangent, or padding only (uniform in a wave): zeros, and no load
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < EW_ROWS; ++j)
        if (owner && dy0 + j < det) dst[s * plane + (long)(dy0 + j) * det] = mk(0.f, 0.f);
    return;
  }
  const TkCorner c = tk_corner(scan, n);
  const float py_ = scan[2 * n], px_ = scan[2 * n + 1];
  const float fy = py_ - floorf(py_), fx = px_ - floorf(px_);
  const float dsy = dscan != nullptr ? dscan[2 * n] : 0.f;
  const float dsx = dscan != nullptr ? dscan[2 * n + 1] : 0.f;
  const long X = (long)c.sx + px;
  const bool okx = X >= 0 && X < W;
  const long Xc = X < 0 ? 0 : (X < W ? X : W - 1);
  cf o[EW_ROWS + 1], d[EW_ROWS + 1];
#pragma unroll
  for (int j = 0; j <= EW_ROWS; ++j) {
    const long Y = (long)c.sy + py0 + j;
    const bool ok = okx && Y >= 0 && Y < H;
    const long Yc = Y < 0 ? 0 : (Y < H ? Y : H - 1);
    const cf v = psi[Yc * W + Xc];
    o[j] = ok ? v : mk(0.f, 0.f);
    d[j] = mk(0.f, 0.f);
    if (dpsi != nullptr) {  // uniform
      const cf t = dpsi[Yc * W + Xc];
      d[j] = ok ? t : mk(0.f, 0.f);
    }
  }
  // the halo column: row min(lane, EW_ROWS) of the column behind the item
  cf ho, hd = mk(0.f, 0.f);
  {
    const long XH = (long)c.sx + px0 + EW_COLS;
    const long Y = (long)c.sy + py0 + (lane < EW_ROWS ? lane : EW_ROWS);
    const bool ok = XH >= 0 && XH < W && Y >= 0 && Y < H;
    const long XHc = XH < 0 ? 0 : (XH < W ? XH : W - 1);
    const long Yc = Y < 0 ? 0 : (Y < H ? Y : H - 1);
    const cf v = psi[Yc * W + XHc];
    ho = ok ? v : mk(0.f, 0.f);
    if (dpsi != nullptr) {  // uniform
      const cf t = dpsi[Yc * W + XHc];
      hd = ok ? t : mk(0.f, 0.f);
    }
  }
  cf pat[EW_ROWS], dpat[EW_ROWS];
  cf right = tk_right_tap<EW_COLS>(o[0], ho, 0, lane);
#pragma unroll
  for (int j = 0; j < EW_ROWS; ++j) {
    const cf o00 = o[j], o01 = right, o10 = o[j + 1];
    const cf o11 = tk_right_tap<EW_COLS>(o10, ho, j + 1, lane);
    right = o11;
    const float dyr = tk_slope(fx, o00.x, o10.x, o01.x, o11.x);
    const float dyi = tk_slope(fx, o00.y, o10.y, o01.y, o11.y);
    const float dxr = tk_slope(fy, o00.x, o01.x, o10.x, o11.x);
    const float dxi = tk_slope(fy, o00.y, o01.y, o10.y, o11.y);
    pat[j] = tk_bilinear(o00, o01, o10, o11, c);
    cf t = mk(0.f, 0.f);
    if (dpsi != nullptr)  // uniform
      t = tk_bilinear(d[j], tk_right_tap<EW_COLS>(d[j], hd, j, lane), d[j + 1],
                      tk_right_tap<EW_COLS>(d[j + 1], hd, j + 1, lane), c);
    dpat[j] = tk_patch_tangent(t, dsy, dyr, dyi, dsx, dxr, dxi);
  }
  const bool colin = px >= 0 && px < pw;
  const int pxc = px < 0 ? 0 : (px < pw ? px : pw - 1);
  // the pixel in a (pw, pw) plane, clamped into the window: the row part is
  // uniform in a wave
  const int pyl = pw - 1;
#define EW_AT(j) ((long)(py0 + (j) < 0 ? 0 : (py0 + (j) < pw ? py0 + (j) : pyl)) * pw + pxc)
  const long pp = (long)pw * pw;
  const float* __restrict__ wn = weights + n * (C + 1) * S;  // uniform
  const float* __restrict__ dwn = dweights != nullptr ? dweights + n * (C + 1) * S : nullptr;
  for (int s = 0; s < S; ++s) {
    // P and dP of the lane's EW_ROWS pixels of mode s
    cf P[EW_ROWS], dP[EW_ROWS];
    {
      const float w0 = wn[s];
      const float dw0 = dwn != nullptr ? dwn[s] : 0.f;
#pragma unroll
      for (int j = 0; j < EW_ROWS; ++j) {
        const cf b = probe[s * pp + EW_AT(j)];
        P[j] = mk(w0 * b.x, w0 * b.y);
        dP[j] = mk(dw0 * b.x, dw0 * b.y);
      }
      if (dprobe != nullptr) {  // uniform
#pragma unroll
        for (int j = 0; j < EW_ROWS; ++j) {
          const cf t = dprobe[s * pp + EW_AT(j)];
          dP[j].x += w0 * t.x;
          dP[j].y += w0 * t.y;
        }
      }
    }
    if (s < M) {  // uniform; M is 0 without an eigen probe
      for (int k = 0; k < C; ++k) {
        const float wk = wn[(long)(k + 1) * S + s];
        const float dwk = dwn != nullptr ? dwn[(long)(k + 1) * S + s] : 0.f;
        const long base = ((long)k * M + s) * pp;
#pragma unroll
        for (int j = 0; j < EW_ROWS; ++j) {
          const cf e = eigen[base + EW_AT(j)];
          P[j].x += wk * e.x;
          P[j].y += wk * e.y;
          dP[j].x += dwk * e.x;
          dP[j].y += dwk * e.y;
        }
        if (deigen != nullptr) {  // uniform
#pragma unroll
          for (int j = 0; j < EW_ROWS; ++j) {
            const cf t = deigen[base + EW_AT(j)];
            dP[j].x += wk * t.x;
            dP[j].y += wk * t.y;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < EW_ROWS; ++j) {
      const cf v = dpat[j] * P[j] + pat[j] * dP[j];
      if (owner && dy0 + j < det)
        dst[s * plane + (long)(dy0 + j) * det] =
            colin && py0 + j >= 0 && py0 + j < pw ? v : mk(0.f, 0.f);
    }
  }
#undef EW_AT
}

}  // namespace

extern "C" int tike_eigen_wave_tangent(const void* psi, const void* dpsi, const float* scan,
                                       const float* dscan, const void* probe, const void* dprobe,
                                       const void* eigen_probe, const void* deigen_probe,
                                       const float* eigen_weights, const float* deigen_weights,
                                       int num_eigen, int eigen_modes, void* nearplane,
                                       long nscan, int S, int pw, int det, int H, int W,
                                       void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(psi && scan && probe && eigen_weights && nearplane);
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  TK_CHECK_ARG(num_eigen >= 0 && eigen_modes >= 0);
  const int C = num_eigen, M = num_eigen > 0 ? eigen_modes : 0;
  if (S > EW_MAX_MODES || (long)C * M > EW_MAX_PLANES) return TK_ERR_UNSUPPORTED;
  TK_CHECK_ARG(C == 0 || (M >= 1 && M <= S && eigen_probe != nullptr));
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one grid column per position: grid.x
  const long groups = tk_item_groups(det, EW_COLS, EW_ROWS);
  TK_CHECK_ARG(groups > 0);
  if (C == 0) deigen_probe = nullptr;  // no plane it could be the tangent of
  hipLaunchKernelGGL(eigen_wave_tangent_kernel, dim3((unsigned)nscan, (unsigned)groups),
                     dim3(256), 0, stream, (const cf*)psi, (const cf*)dpsi, scan, dscan,
                     (const cf*)probe, (const cf*)dprobe, (const cf*)eigen_probe,
                     (const cf*)deigen_probe, eigen_weights, deigen_weights, C, M,
                     (cf*)nearplane, S, pw, det, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
