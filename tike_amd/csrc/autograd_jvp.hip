// The kernels of the FORWARD-mode derivative of the differentiable intensity
// model (tike_amd/autograd.py: intensity_jvp, _Intensity.jvp): the tangent of
// the exit waves, and the tangent of the intensity from a far plane and its
// tangent.  Between the two, the tangent far plane comes from tike_fft2.  The
// multislice model (multislice_intensity_jvp) walks its tangent through the
// slices with tike_slice_wave_tangent, the Fresnel step between two slices
// being linear.  No reference counterpart: the reference has no derivative of
// its forward model in any direction but its hand-written adjoints.
//
//   tike_conv_fwd_tangent   dwave[n][s] = pad( dpatch_n probe[s] + patch_n(psi) dprobe[s] )
//                           dpatch_n = patch_n(dpsi) + dscan[n][0] Dy_n(psi) + dscan[n][1] Dx_n(psi)
//   tike_slice_wave_tangent dwave[n][s] = dpatch_n beam[n|0][s] + patch_n(psi) dbeam[n|0][s]
//                           (one slice, probe window = detector: no padding; dwave may be dbeam)
//   tike_intensity_tangent  dI[f][p] = 2 sum_j Re( conj(far[f][j][p]) dfar[f][j][p] )
//                           I[f][p]  = sum_j |far[f][j][p]|^2             (optional)
//
// Byte models.  tike_conv_fwd_tangent, per position: S * det^2 * 8 bytes
// written once (the window and the zeros around it); (pw + 1)^2 * 8 bytes of
// object read, twice that with dpsi (mostly served from cache: the footprints
// of neighbouring positions overlap), S * pw^2 * 8 bytes of probe, twice that
// with dprobe (from cache: every position reads the same planes), 8 bytes of
// scan and 8 of dscan.  tike_slice_wave_tangent, per position: S * pw^2 * 8
// bytes written once; S * pw^2 * 8 bytes of beam read once when it is per
// position, and as many of dbeam (a shared beam or dbeam comes from cache, as
// the probe above); (pw + 1)^2 * 8 bytes of object taps, twice that with dpsi
// (mostly from cache); 8 bytes of scan and 8 of dscan.
// tike_intensity_tangent, per frame of P planes of npix pixels:
// 2 * P * npix * 8 bytes of far plane and tangent read once, npix * 4 bytes of
// dI written, npix * 4 more with I.
#include "../../include/tike_amd.h"
#include "frame_lanes.h"
#include "patch_taps.h"

namespace {

constexpr int JV_MAX_MODES = 16;  // TK_MAX_MODES of the gradient kernels
constexpr int JV_COLS = 63;       // detector columns of a wave: lane 63 is the halo lane
constexpr int JV_ROWS = 8;        // detector rows of a strip

// grid (position, group of four items): the halo-LANE scheme of patch_taps.h
// laid over the (det, det) DETECTOR plane, one item per wave; lane 63 owns no
// output.  The strips of psi and of dpsi serve the patch, Dy, Dx and every
// mode.  A NULL tangent is a zero tangent: its loads are skipped (uniform)
// and its terms are computed on zeros.  A pixel outside the centred pw window
// is written as exactly 0.0; an item that lies in the padding altogether only
// writes its zeros.  Every output element has one owner: no atomics.  All
// offsets are `long`.
__global__ __launch_bounds__(256) void conv_fwd_tangent_kernel(
    const cf* __restrict__ psi, const cf* __restrict__ dpsi, const float* __restrict__ scan,
    const float* __restrict__ dscan, const cf* __restrict__ probe, const cf* __restrict__ dprobe,
    cf* __restrict__ nearplane, int S, int pw, int det, int H, int W) {
  const long n = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (det + JV_COLS - 1) / JV_COLS;
  const int nstrip = (det + JV_ROWS - 1) / JV_ROWS;
  const int item = (int)blockIdx.y * 4 + wave;  // uniform in a wave
  if (item >= nseg * nstrip) return;
  const int pad = (det - pw) / 2;
  const int dx0 = (item % nseg) * JV_COLS;
  const int dy0 = (item / nseg) * JV_ROWS;
  const int dx = dx0 + lane;  // detector column; lane 63: the right tap of lane 62
  const int px = dx - pad, px0 = dx0 - pad, py0 = dy0 - pad;
  const bool owner = lane < JV_COLS && dx < det;
  const long plane = (long)det * det;
  cf* __restrict__ dst = nearplane + n * S * plane + (long)dx;
  if (py0 + JV_ROWS <= 0 || py0 >= pw || px0 + JV_COLS <= 0 || px0 >= pw) {
    // padding only (uniform in a wave)
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < JV_ROWS; ++j)
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
  cf o[JV_ROWS + 1], d[JV_ROWS + 1];
#pragma unroll
  for (int j = 0; j <= JV_ROWS; ++j) {
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
  const bool colin = px >= 0 && px < pw;
  const int pxc = px < 0 ? 0 : (px < pw ? px : pw - 1);
  cf pat[JV_ROWS], dpat[JV_ROWS];
  cf right = tk_cf_lane_up(o[0]), dright = tk_cf_lane_up(d[0]);
#pragma unroll
  for (int j = 0; j < JV_ROWS; ++j) {
    const cf o00 = o[j], o01 = right, o10 = o[j + 1];
    const cf o11 = tk_cf_lane_up(o10);
    right = o11;
    const cf d00 = d[j], d01 = dright, d10 = d[j + 1];
    const cf d11 = tk_cf_lane_up(d10);
    dright = d11;
    const float dyr = tk_slope(fx, o00.x, o10.x, o01.x, o11.x);
    const float dyi = tk_slope(fx, o00.y, o10.y, o01.y, o11.y);
    const float dxr = tk_slope(fy, o00.x, o01.x, o10.x, o11.x);
    const float dxi = tk_slope(fy, o00.y, o01.y, o10.y, o11.y);
    pat[j] = tk_bilinear(o00, o01, o10, o11, c);
    cf t = tk_bilinear(d00, d01, d10, d11, c);
    dpat[j] = tk_patch_tangent(t, dsy, dyr, dyi, dsx, dxr, dxi);
  }
  const long pp = (long)pw * pw;
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int j = 0; j < JV_ROWS; ++j) {
      const int py = py0 + j;
      const bool in = colin && py >= 0 && py < pw;
      const int pyc = py < 0 ? 0 : (py < pw ? py : pw - 1);
      const long at = s * pp + (long)pyc * pw + pxc;
      cf v = dpat[j] * probe[at];
      if (dprobe != nullptr) v = v + pat[j] * dprobe[at];  // uniform
      if (owner && dy0 + j < det)
        dst[s * plane + (long)(dy0 + j) * det] = in ? v : mk(0.f, 0.f);
    }
  }
}

constexpr int SW_COLS = 64;  // columns of an item: every lane owns one
constexpr int SW_ROWS = 8;   // rows of a strip

// grid (position, group of four items): conv_fwd_tangent_kernel for ONE slice
// of a multislice object, whose (pw, pw) plane has no padding (probe window =
// detector), with a beam and a tangent beam that may differ from position to
// position (stride 0: shared).  The halo-COLUMN scheme of patch_taps.h, one
// item per wave: all 64 lanes own a column.  A NULL tangent is a zero tangent
// whose loads are skipped (uniform); with all three NULL the plane is written
// as exactly 0.0 and nothing is loaded.
//
// dwave may be dbeam itself (stride S * pw * pw): the SW_ROWS elements of a
// mode that a lane owns are loaded into registers before the first of them is
// stored, a lane that owns no element stores nothing, and what a clamped
// address makes it load is never used -- so every element is read by its one
// owner before that owner writes it.  Hence neither is `__restrict__`.  Every
// output element has one owner: no atomics.  All offsets are `long`.
__global__ __launch_bounds__(256) void slice_wave_tangent_kernel(
    const cf* __restrict__ psi, const cf* __restrict__ dpsi, const float* __restrict__ scan,
    const float* __restrict__ dscan, const cf* __restrict__ beam, long beam_stride,
    const cf* dbeam, long dbeam_stride, cf* dwave, int S, int pw, int H, int W) {
  const long n = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nseg = (pw + SW_COLS - 1) / SW_COLS;
  const int nstrip = (pw + SW_ROWS - 1) / SW_ROWS;
  const int item = (int)blockIdx.y * 4 + wave;  // uniform in a wave
  if (item >= nseg * nstrip) return;
  const int px0 = (item % nseg) * SW_COLS;
  const int py0 = (item / nseg) * SW_ROWS;
  const int px = px0 + lane;
  const bool owner = px < pw;
  const int pxc = owner ? px : pw - 1;
  const long pp = (long)pw * pw;
  cf* dst = dwave + n * S * pp + px;
  if (dpsi == nullptr && dscan == nullptr && dbeam == nullptr) {
    // no tangent (uniform): zeros, and no load
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < SW_ROWS; ++j)
        if (owner && py0 + j < pw) dst[s * pp + (long)(py0 + j) * pw] = mk(0.f, 0.f);
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
  cf o[SW_ROWS + 1], d[SW_ROWS + 1];
#pragma unroll
  for (int j = 0; j <= SW_ROWS; ++j) {
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
  // the halo column: row min(lane, SW_ROWS) of the column behind the item
  cf ho, hd = mk(0.f, 0.f);
  {
    const long XH = (long)c.sx + px0 + SW_COLS;
    const long Y = (long)c.sy + py0 + (lane < SW_ROWS ? lane : SW_ROWS);
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
  cf pat[SW_ROWS], dpat[SW_ROWS];
  cf right = tk_right_tap<SW_COLS>(o[0], ho, 0, lane);
#pragma unroll
  for (int j = 0; j < SW_ROWS; ++j) {
    const cf o00 = o[j], o01 = right, o10 = o[j + 1];
    const cf o11 = tk_right_tap<SW_COLS>(o10, ho, j + 1, lane);
    right = o11;
    const float dyr = tk_slope(fx, o00.x, o10.x, o01.x, o11.x);
    const float dyi = tk_slope(fx, o00.y, o10.y, o01.y, o11.y);
    const float dxr = tk_slope(fy, o00.x, o01.x, o10.x, o11.x);
    const float dxi = tk_slope(fy, o00.y, o01.y, o10.y, o11.y);
    pat[j] = tk_bilinear(o00, o01, o10, o11, c);
    cf t = mk(0.f, 0.f);
    if (dpsi != nullptr)  // uniform
      t = tk_bilinear(d[j], tk_right_tap<SW_COLS>(d[j], hd, j, lane), d[j + 1],
                      tk_right_tap<SW_COLS>(d[j + 1], hd, j + 1, lane), c);
    dpat[j] = tk_patch_tangent(t, dsy, dyr, dyi, dsx, dxr, dxi);
  }
  const cf* __restrict__ bsrc = beam + n * beam_stride;
  const cf* dbsrc = dbeam != nullptr ? dbeam + n * dbeam_stride : nullptr;
  for (int s = 0; s < S; ++s) {
    cf b[SW_ROWS], t[SW_ROWS];
#pragma unroll
    for (int j = 0; j < SW_ROWS; ++j) {
      const int py = py0 + j;
      const long at = s * pp + (long)(py < pw ? py : pw - 1) * pw + pxc;
      b[j] = bsrc[at];
      t[j] = mk(0.f, 0.f);
      if (dbsrc != nullptr) t[j] = dbsrc[at];  // uniform
    }
#pragma unroll
    for (int j = 0; j < SW_ROWS; ++j) {
      cf v = dpat[j] * b[j];
      if (dbsrc != nullptr) v = v + pat[j] * t[j];  // uniform
      if (owner && py0 + j < pw) dst[s * pp + (long)(py0 + j) * pw] = v;
    }
  }
}

constexpr int JV_PX = 4;  // pixels of a lane: two 16-byte accesses per plane and far plane

// The layout of farplane_scale_kernel: a lane owns JV_PX consecutive pixels of
// one frame and walks the P planes, both far planes read once; the last
// npix % JV_PX pixels of a frame are taken one per lane by the lanes behind
// the last vector.  `bpf` workgroups serve a frame.  The intensity is summed
// as tike_intensity and tike_fly_farplane_gradient sum it (planes ascending,
// a float32 running sum of re^2 + im^2, each product and each sum rounded:
// those kernels compile to packed multiplies and adds).  The same bits must
// not hang on what the compiler chooses to fuse here, so contraction is off
// in this kernel: no fused multiply-add in either sum.
__global__ __launch_bounds__(256) void intensity_tangent_kernel(
    const cf* __restrict__ farplane, const cf* __restrict__ dfarplane,
    float* __restrict__ intensity, float* __restrict__ dintensity, int P, long npix, long bpf) {
#pragma clang fp contract(off)
  const long f = (long)blockIdx.x / bpf;
  const long v = ((long)blockIdx.x % bpf) * blockDim.x + threadIdx.x;
  const cf* __restrict__ F = farplane + f * P * npix;
  const cf* __restrict__ D = dfarplane + f * P * npix;
  const long nvec = npix / JV_PX;
  if (v < nvec) {
    const long p = v * JV_PX;
    float I[JV_PX] = {0.f, 0.f, 0.f, 0.f};
    float T[JV_PX] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < P; ++j) {
      const cf* at = F + j * npix + p;
      const cf* dt = D + j * npix + p;
      const tk_f4a8 a = *reinterpret_cast<const tk_f4a8*>(at);
      const tk_f4a8 b = *reinterpret_cast<const tk_f4a8*>(at + 2);
      const tk_f4a8 da = *reinterpret_cast<const tk_f4a8*>(dt);
      const tk_f4a8 db = *reinterpret_cast<const tk_f4a8*>(dt + 2);
      I[0] += a.x * a.x + a.y * a.y;
      I[1] += a.z * a.z + a.w * a.w;
      I[2] += b.x * b.x + b.y * b.y;
      I[3] += b.z * b.z + b.w * b.w;
      T[0] += a.x * da.x + a.y * da.y;
      T[1] += a.z * da.z + a.w * da.w;
      T[2] += b.x * db.x + b.y * db.y;
      T[3] += b.z * db.z + b.w * db.w;
    }
    tk_f4a4 t;
#pragma unroll
    for (int k = 0; k < JV_PX; ++k) t[k] = 2.0f * T[k];
    *reinterpret_cast<tk_f4a4*>(dintensity + f * npix + p) = t;
    if (intensity != nullptr) {
      tk_f4a4 o;
#pragma unroll
      for (int k = 0; k < JV_PX; ++k) o[k] = I[k];
      *reinterpret_cast<tk_f4a4*>(intensity + f * npix + p) = o;
    }
    return;
  }
  // scalar tail: fewer than JV_PX pixels, one per lane
  const long p = nvec * JV_PX + (v - nvec);
  if (p >= npix) return;
  float I = 0.f, T = 0.f;
  for (int j = 0; j < P; ++j) {
    const cf a = F[j * npix + p], da = D[j * npix + p];
    I += a.x * a.x + a.y * a.y;  // (written here: the pragma does not reach into norm2)
    T += a.x * da.x + a.y * da.y;
  }
  dintensity[f * npix + p] = 2.0f * T;
  if (intensity != nullptr) intensity[f * npix + p] = I;
}

}  // namespace

extern "C" int tike_conv_fwd_tangent(const void* psi, const void* dpsi, const float* scan,
                                     const float* dscan, const void* probe, const void* dprobe,
                                     void* nearplane, long nscan, int S, int pw, int det, int H,
                                     int W, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(psi && scan && probe && nearplane);
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && det >= pw && H >= 1 && W >= 1);
  if (S > JV_MAX_MODES) return TK_ERR_UNSUPPORTED;
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one grid column per position: grid.x
  const long groups = tk_item_groups(det, JV_COLS, JV_ROWS);
  TK_CHECK_ARG(groups > 0);
  hipLaunchKernelGGL(conv_fwd_tangent_kernel, dim3((unsigned)nscan, (unsigned)groups), dim3(256),
                     0, stream, (const cf*)psi, (const cf*)dpsi, scan, dscan, (const cf*)probe,
                     (const cf*)dprobe, (cf*)nearplane, S, pw, det, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_slice_wave_tangent(const void* psi, const void* dpsi, const float* scan,
                                       const float* dscan, const void* beam, int beam_per_scan,
                                       const void* dbeam, int dbeam_per_scan, void* dwave,
                                       long nscan, int S, int pw, int H, int W, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(psi && scan && beam && dwave);
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && H >= 1 && W >= 1);
  if (S > JV_MAX_MODES) return TK_ERR_UNSUPPORTED;
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one grid column per position: grid.x
  const long groups = tk_item_groups(pw, SW_COLS, SW_ROWS);
  TK_CHECK_ARG(groups > 0);
  const long set = (long)S * pw * pw;
  hipLaunchKernelGGL(slice_wave_tangent_kernel, dim3((unsigned)nscan, (unsigned)groups),
                     dim3(256), 0, stream, (const cf*)psi, (const cf*)dpsi, scan, dscan,
                     (const cf*)beam, beam_per_scan ? set : 0L, (const cf*)dbeam,
                     dbeam_per_scan ? set : 0L, (cf*)dwave, S, pw, H, W);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_intensity_tangent(const void* farplane, const void* dfarplane,
                                      float* intensity, float* dintensity, long nframe, int P,
                                      long npix, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && dfarplane && dintensity);
  TK_CHECK_ARG(nframe >= 0 && P >= 1 && npix >= 1);
  if (nframe == 0) return TK_OK;
  // lanes of a frame: one per vector of JV_PX pixels, one per pixel of the tail
  const long lanes = npix / JV_PX + npix % JV_PX;
  const long bpf = (lanes + 255) / 256;
  TK_CHECK_ARG(bpf <= 0x7fffffffL / nframe);  // the workgroups of all frames: grid.x
  hipLaunchKernelGGL(intensity_tangent_kernel, dim3((unsigned)(nframe * bpf)), dim3(256), 0,
                     stream, (const cf*)farplane, (const cf*)dfarplane, intensity, dintensity, P,
                     npix, bpf);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
