// Position refinement by the gradient of intensity (Dwivedi et al. 2018;
// reference ptycho/position.py:631-703): the five sums of the 2 x 2 normal
// equations of every position, and the gaussian cost, in ONE streaming pass
// over the three far planes and the pattern.
//
// Byte model per position: 3 * S * npix * 8 bytes of far plane and npix * 4
// (or * 2) bytes of pattern are read once; 24 bytes are written.
#include "../../include/tike_amd.h"
#include "frame_lanes.h"

namespace {

// eight counts in one 16-byte load, element-aligned as the types of frame_lanes.h
typedef unsigned short pd_h8 __attribute__((ext_vector_type(8), aligned(2)));

// Everything past the loads is float64.  The five sums are not sums of
// positive terms: a r and b r (and a b) cancel over the pixels down to a small
// share of their terms, so float32 rounding of I, a, b and of the running sums,
// harmless against the terms, is not harmless against the result.  The inputs
// are exact in float64 and the only rounding left is the final one to float32.
// The kernel stays bound by its loads: about 20 float64 operations per 24
// bytes read.
struct PdAcc {
  double aa, ab, bb, ar, br, cost;
};

// one pixel: I, a, b complete over the modes, d the measured count
__device__ __forceinline__ void pd_add(PdAcc& k, double I, double a, double b, float d) {
  const double r = (double)d - I;
  k.aa += a * a;
  k.ab += a * b;
  k.bb += b * b;
  k.ar += a * r;
  k.br += b * r;
  // a sum of squares: float32 roots are enough for the cost
  const float q = sqrtf((float)I) - sqrtf(d);
  k.cost += (double)(q * q);
}

// one mode of one pixel: I += |f0|^2, b += Re((f0 - fx) conj(f0)), a with fy;
// the factor 2 goes with inv_dx
__device__ __forceinline__ void pd_mode(double& I, double& a, double& b, float f0r, float f0i,
                                        float fxr, float fxi, float fyr, float fyi) {
  const double r0 = f0r, i0 = f0i;
  I += r0 * r0 + i0 * i0;
  b += (r0 - (double)fxr) * r0 + (i0 - (double)fxi) * i0;
  a += (r0 - (double)fyr) * r0 + (i0 - (double)fyi) * i0;
}

// One workgroup per position.  A lane owns PX consecutive pixels per sweep
// (PX * 2 or 4 bytes of pattern = one 16-byte load) and walks the modes with
// I, a and b of those pixels in registers; the last npix % PX pixels are taken
// one per lane.
template <bool U16>
__global__ __launch_bounds__(256) void position_pd_sums_kernel(
    const cf* __restrict__ far0, const cf* __restrict__ far_dx, const cf* __restrict__ far_dy,
    const void* __restrict__ data_, float inv_dx, float* __restrict__ sums,
    float* __restrict__ costs, int S, long npix) {
  constexpr int PX = U16 ? 8 : 4;
  __shared__ double red[4][6];
  const long n = blockIdx.x;
  const long row = n * S * npix;  // first mode of this position
  const float* __restrict__ d32 = U16 ? nullptr : (const float*)data_ + n * npix;
  const unsigned short* __restrict__ d16 =
      U16 ? (const unsigned short*)data_ + n * npix : nullptr;
  PdAcc k = {0., 0., 0., 0., 0., 0.};
  const double scale = 2.0 * (double)inv_dx;
  const long nvec = npix / PX;
  for (long v = threadIdx.x; v < nvec; v += blockDim.x) {
    const long p = v * PX;
    double I[PX], a[PX], b[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) I[j] = a[j] = b[j] = 0.;
    for (int s = 0; s < S; ++s) {
      const long at = row + s * npix + p;
#pragma unroll
      for (int h = 0; h < PX / 2; ++h) {
        const tk_f4a8 f0 = *reinterpret_cast<const tk_f4a8*>(far0 + at + 2 * h);
        const tk_f4a8 fx = *reinterpret_cast<const tk_f4a8*>(far_dx + at + 2 * h);
        const tk_f4a8 fy = *reinterpret_cast<const tk_f4a8*>(far_dy + at + 2 * h);
        pd_mode(I[2 * h], a[2 * h], b[2 * h], f0.x, f0.y, fx.x, fx.y, fy.x, fy.y);
        pd_mode(I[2 * h + 1], a[2 * h + 1], b[2 * h + 1], f0.z, f0.w, fx.z, fx.w, fy.z, fy.w);
      }
    }
    float d[PX];
    if (U16) {
      const pd_h8 c = *reinterpret_cast<const pd_h8*>(d16 + p);
#pragma unroll
      for (int j = 0; j < PX; ++j) d[j] = (float)c[j];
    } else {
      const tk_f4a4 c = *reinterpret_cast<const tk_f4a4*>(d32 + p);
#pragma unroll
      for (int j = 0; j < PX; ++j) d[j] = c[j];
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) pd_add(k, I[j], a[j] * scale, b[j] * scale, d[j]);
  }
  // scalar tail: fewer than PX pixels, one per lane
  for (long p = nvec * PX + threadIdx.x; p < npix; p += blockDim.x) {
    double I = 0., a = 0., b = 0.;
    for (int s = 0; s < S; ++s) {
      const long at = row + s * npix + p;
      const cf f0 = far0[at], fx = far_dx[at], fy = far_dy[at];
      pd_mode(I, a, b, f0.x, f0.y, fx.x, fx.y, fy.x, fy.y);
    }
    pd_add(k, I, a * scale, b * scale, U16 ? (float)d16[p] : d32[p]);
  }
  // wave64 shuffles, then the four waves through LDS in a fixed order
  double w[6] = {k.aa, k.ab, k.bb, k.ar, k.br, k.cost};
#pragma unroll
  for (int i = 0; i < 6; ++i) w[i] = tk_wave_sum(w[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) red[threadIdx.x >> 6][i] = w[i];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int i = threadIdx.x;
    const double t = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    if (i < 5)
      sums[n * 5 + i] = (float)t;
    else if (costs != nullptr)
      costs[n] = (float)(t / (double)npix);
  }
}

}  // namespace

extern "C" int tike_position_pd_sums(const void* far0, const void* far_dx, const void* far_dy,
                                     const void* data, int data_u16, float inv_dx, float* sums,
                                     float* costs, long nscan, int S, long npix, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(far0 && far_dx && far_dy && data && sums);
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && npix >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(nscan <= 0x7fffffffL);  // one workgroup per position: grid.x
  const dim3 grid((unsigned)nscan), block(256);
  if (data_u16)
    hipLaunchKernelGGL((position_pd_sums_kernel<true>), grid, block, 0, stream, (const cf*)far0,
                       (const cf*)far_dx, (const cf*)far_dy, data, inv_dx, sums, costs, S, npix);
  else
    hipLaunchKernelGGL((position_pd_sums_kernel<false>), grid, block, 0, stream,
                       (const cf*)far0, (const cf*)far_dx, (const cf*)far_dy, data, inv_dx, sums,
                       costs, S, npix);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
