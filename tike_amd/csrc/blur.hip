// Far-field blur (no reference counterpart): partial spatial coherence in the
// Gaussian-Schell approximation and the detector's point-spread function both
// convolve the recorded intensity with a small non-negative kernel,
//   I_model[f] = K (*) I[f],   I[f][p] = sum_{j < fly*S} |farplane[f][j][p]|^2,
//   I_model[y][x] = sum_{u,v} K[u][v] I[(y - u + r) mod det][(x - v + r) mod det],
// K (k,k) f32, k in {3,5,7}, r = k / 2, centre at [r][r].  The convolution is
// CYCLIC over the (det,det) plane in the stored (FFT-shifted) layout of the
// data; the shift between the stored and the physical layout is itself cyclic,
// so this is the physical convolution with the detector's opposite edges
// joined.  The noise-model formulas of noise_model.h are taken at I_model.
//   tike_blur_cost_factor   costs, the table T = K (star) (up mask l') -- the
//                           cyclic CORRELATION, the adjoint of the blur -- and
//                           I_model, from STORED intensities
//   tike_blur_kernel_sums   cost partials and d cost / d K from stored
//                           intensities: a CG block on K needs no transform
//
// Blur couples neighbouring pixels, and a lane of the far-plane kernels owns a
// pixel over all planes and cannot see its neighbours; the stencil therefore
// lives on the intensity array, 1 / (2 fly S) of the far plane's bytes, where a
// halo read twice costs little.
//
// Byte model of tike_blur_cost_factor per pixel and frame: 4 bytes of
// intensity, 4 or 2 of counts and 1 of mask read, 4 of table written (4 more
// with `blurred`); the halo (2r around a 32 x 32 tile) comes from cache.
#include "../../include/tike_amd.h"
#include "noise_model.h"

namespace {

constexpr int BT = 32;      // tile edge of tike_blur_cost_factor
constexpr int ST = 16;      // tile edge of tike_blur_kernel_sums: one pixel per lane
constexpr int SPLITS = 4;   // contiguous frame ranges of tike_blur_kernel_sums

// a mod det for a in [-det, 2 det): EVERY index into a frame goes through here
__device__ __forceinline__ int wrap(int a, int det) {
  const int m = a % det;
  return m < 0 ? m + det : m;
}

__device__ __forceinline__ float count_at(const void* data, bool u16, long i) {
  return u16 ? (float)((const unsigned short*)data)[i] : ((const float*)data)[i];
}

// One workgroup per frame walks the frame's BT x BT tiles (the last of a row or
// column may be narrower) in row-major order.  Per tile:
//   1. the tile plus a halo of hs = hr + R is staged into S with modular
//      indices (hr = R when the table is asked for, else 0);
//   2. on the tile plus hr, I_model is the K*K-tap sum, taps ascending u then
//      v, float32; the factor g = up l'(I_model, d) on measured pixels and
//      exactly 0 elsewhere goes to G; pixels of the tile proper give `blurred`
//      and their cost term -- every pixel of the frame exactly once, by the
//      same lane with or without a table;
//   3. the table is the K*K-tap correlation of G on the tile, the same order.
// The cost is summed per lane in float64 over the tiles, then as the siblings
// sum a frame: wave shuffles, the four waves through LDS.
template <int MODEL, bool U16, int K>
__global__ __launch_bounds__(256) void blur_cost_factor_kernel(
    const float* __restrict__ intensity, const float* __restrict__ kernel,
    const void* __restrict__ data, const unsigned char* __restrict__ mask,
    const float* __restrict__ upstream, float* __restrict__ costs, float* __restrict__ table,
    float* __restrict__ blurred, int det, double inv_nmeasured) {
#pragma clang fp contract(off)
  constexpr int R = K / 2, SW = BT + 4 * R, GW = BT + 2 * R;
  __shared__ float S[SW * SW];
  __shared__ float G[GW * GW];
  __shared__ double red[4];
  const long n = blockIdx.x;
  const long npix = (long)det * det;
  const float* __restrict__ I = intensity + n * npix;
  float kr[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) kr[i] = kernel[i];
  const bool factor = data != nullptr;
  const int hr = table != nullptr ? R : 0;
  const int hs = hr + R;
  // upstream / num_measured, rounded once
  const float up = (float)((upstream != nullptr ? (double)upstream[n] : 1.0) * inv_nmeasured);
  double cost = 0.;
  for (int ty0 = 0; ty0 < det; ty0 += BT) {
    const int th = det - ty0 < BT ? det - ty0 : BT;
    for (int tx0 = 0; tx0 < det; tx0 += BT) {
      const int tw = det - tx0 < BT ? det - tx0 : BT;
      const int sh = th + 2 * hs, sw = tw + 2 * hs;
      __syncthreads();  // the readers of the tile before are done
      for (int i = threadIdx.x; i < sh * sw; i += blockDim.x) {
        const int sy = i / sw, sx = i - sy * sw;
        const int yy = wrap(ty0 - hs + sy, det), xx = wrap(tx0 - hs + sx, det);
        S[sy * SW + sx] = I[(long)yy * det + xx];
      }
      __syncthreads();
      const int gw = tw + 2 * hr;
      // I_model and the factor of pixel (ty0 - hr + gy, tx0 - hr + gx), which
      // sits at S[gy + R][gx + R]
      auto pixel = [&](int gy, int gx, bool inner) {
        float im = 0.f;
#pragma unroll
        for (int u = 0; u < K; ++u)
#pragma unroll
          for (int v = 0; v < K; ++v)
            im += kr[u * K + v] * S[(gy + 2 * R - u) * SW + (gx + 2 * R - v)];
        const int yy = wrap(ty0 - hr + gy, det), xx = wrap(tx0 - hr + gx, det);
        const long p = (long)yy * det + xx;
        if (inner && blurred != nullptr) blurred[n * npix + p] = im;
        float g = 0.f;
        if (factor) {
          const bool measured = mask != nullptr ? mask[p] != 0 : true;
          const float d = count_at(data, U16, n * npix + p);
          float term;
          const float lp = tk_noise_pixel<MODEL>(im, d, term);
          g = measured ? up * lp : 0.0f;
          if (inner) cost += measured ? (double)term : 0.0;
        }
        G[gy * GW + gx] = g;
      };
      // the tile proper, one lane per pixel whatever the halo: the lanes'
      // cost sums, and with them the bits of costs, do not depend on which
      // outputs are asked for
      for (int i = threadIdx.x; i < th * tw; i += blockDim.x) {
        const int y = i / tw;
        pixel(hr + y, hr + (i - y * tw), true);
      }
      // the ring of width hr around it: hr rows above and below over the full
      // width, then hr columns left and right of the tile's rows
      const int bands = 2 * hr * gw;
      for (int j = threadIdx.x; j < bands + 2 * hr * th; j += blockDim.x) {
        if (j < bands) {
          const int row = j / gw;
          pixel(row < hr ? row : th + row, j - row * gw, false);
        } else {
          const int y = (j - bands) / (2 * hr), c = (j - bands) - y * (2 * hr);
          pixel(hr + y, c < hr ? c : tw + c, false);
        }
      }
      if (table != nullptr) {
        __syncthreads();
        for (int i = threadIdx.x; i < th * tw; i += blockDim.x) {
          const int y = i / tw, x = i - y * tw;
          // pixel (ty0 + y, tx0 + x) sits at G[y + R][x + R]
          float t = 0.f;
#pragma unroll
          for (int u = 0; u < K; ++u)
#pragma unroll
            for (int v = 0; v < K; ++v) t += kr[u * K + v] * G[(y + u) * GW + (x + v)];
          table[n * npix + (long)(ty0 + y) * det + (tx0 + x)] = t;
        }
      }
    }
  }
  if (costs != nullptr) {
    cost = tk_frame_sum_f64(cost, red);
    if (threadIdx.x == 0) costs[n] = (float)(cost * inv_nmeasured);
  }
}

// Workgroup (t, s) owns the ST x ST tile t of the plane, one pixel per lane,
// through the frames of range s (SPLITS contiguous ranges of
// ceil(nframe / SPLITS) frames), ascending.  Per frame the tile plus a halo of
// R is staged with modular indices; a lane forms I_model (taps ascending u then
// v, float32), the factor g = up_f l' (0 exactly when unmeasured) and, with
// GRAD, the K*K float32 products g I[p - (u - R, v - R)], each summed in
// float64 in its own accumulator.  The workgroup's sums -- wave shuffles, the
// four waves through LDS -- go to `partials`: the cost at [w], the K*K kernel
// sums at [nwg + w K*K ..], w = s ntiles + t.
template <int MODEL, bool U16, int K, bool GRAD>
__global__ __launch_bounds__(256) void blur_sums_kernel(
    const float* __restrict__ intensity, const float* __restrict__ kernel,
    const void* __restrict__ data, const unsigned char* __restrict__ mask,
    const float* __restrict__ upstream, double* __restrict__ partials, long nframe, int det,
    double inv_nmeasured) {
#pragma clang fp contract(off)
  constexpr int R = K / 2, SW = ST + 2 * R;
  __shared__ float S[SW * SW];
  __shared__ double red[4];
  const long npix = (long)det * det;
  const int ntx = (det + ST - 1) / ST;
  const int ty0 = (int)(blockIdx.x / ntx) * ST, tx0 = (int)(blockIdx.x % ntx) * ST;
  const int th = det - ty0 < ST ? det - ty0 : ST, tw = det - tx0 < ST ? det - tx0 : ST;
  const int y = threadIdx.x / ST, x = threadIdx.x % ST;
  const bool active = y < th && x < tw;
  const long p = active ? (long)(ty0 + y) * det + (tx0 + x) : 0;
  const bool measured = active && (mask != nullptr ? mask[p] != 0 : true);
  float kr[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) kr[i] = kernel[i];
  const long per = (nframe + SPLITS - 1) / SPLITS;
  const long f0 = (long)blockIdx.y * per;
  const long f1 = f0 + per < nframe ? f0 + per : nframe;
  const int sh = th + 2 * R, sw = tw + 2 * R;
  double cost = 0.;
  double acc[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) acc[i] = 0.;
  for (long f = f0; f < f1; ++f) {
    const float* __restrict__ I = intensity + f * npix;
    __syncthreads();  // the readers of the frame before are done
    for (int i = threadIdx.x; i < sh * sw; i += blockDim.x) {
      const int sy = i / sw, sx = i - sy * sw;
      const int yy = wrap(ty0 - R + sy, det), xx = wrap(tx0 - R + sx, det);
      S[sy * SW + sx] = I[(long)yy * det + xx];
    }
    __syncthreads();
    if (active) {
      // pixel (ty0 + y, tx0 + x) sits at S[y + R][x + R]
      float im = 0.f;
#pragma unroll
      for (int u = 0; u < K; ++u)
#pragma unroll
        for (int v = 0; v < K; ++v)
          im += kr[u * K + v] * S[(y + 2 * R - u) * SW + (x + 2 * R - v)];
      const float d = count_at(data, U16, f * npix + p);
      const double u64 = upstream != nullptr ? (double)upstream[f] : 1.0;
      const float up = (float)(u64 * inv_nmeasured);
      float term;
      const float lp = tk_noise_pixel<MODEL>(im, d, term);
      const float g = measured ? up * lp : 0.0f;
      cost += measured ? u64 * (double)term : 0.0;
      if (GRAD) {
#pragma unroll
        for (int u = 0; u < K; ++u)
#pragma unroll
          for (int v = 0; v < K; ++v)
            acc[u * K + v] += (double)(g * S[(y + 2 * R - u) * SW + (x + 2 * R - v)]);
      }
    }
  }
  const long nwg = (long)gridDim.x * gridDim.y;
  const long w = (long)blockIdx.y * gridDim.x + blockIdx.x;
  __syncthreads();
  cost = tk_frame_sum_f64(cost, red);
  if (threadIdx.x == 0) partials[w] = cost * inv_nmeasured;
  if (GRAD) {
#pragma unroll
    for (int i = 0; i < K * K; ++i) {
      __syncthreads();  // `red` of the sum before has been read
      const double s = tk_frame_sum_f64(acc[i], red);
      if (threadIdx.x == 0) partials[nwg + w * (K * K) + i] = s;
    }
  }
}

// kgrad[i] = the workgroups' kernel sums added in ascending w: tile, then
// frame range.  One lane per entry of K.
__global__ __launch_bounds__(64) void blur_kgrad_finish_kernel(
    const double* __restrict__ partials, double* __restrict__ kgrad, long nwg, int kk) {
  const int i = threadIdx.x;
  if (i >= kk) return;
  double s = 0.;
  for (long w = 0; w < nwg; ++w) s += partials[nwg + w * kk + i];
  kgrad[i] = s;
}

long sums_tiles(int det) {
  const long nt = ((long)det + ST - 1) / ST;
  return nt * nt;
}

template <int MODEL, bool U16>
void cost_factor_launch(int k, dim3 grid, hipStream_t stream, const float* intensity,
                        const float* kernel, const void* data, const unsigned char* measured,
                        const float* upstream, float* costs, float* table, float* blurred,
                        int det, double inv) {
#define TK_BLUR_CF(KK)                                                                    \
  hipLaunchKernelGGL((blur_cost_factor_kernel<MODEL, U16, KK>), grid, dim3(256), 0, stream, \
                     intensity, kernel, data, measured, upstream, costs, table, blurred, det, inv)
  if (k == 3)
    TK_BLUR_CF(3);
  else if (k == 5)
    TK_BLUR_CF(5);
  else
    TK_BLUR_CF(7);
#undef TK_BLUR_CF
}

template <int MODEL, bool U16, bool GRAD>
void sums_launch(int k, dim3 grid, hipStream_t stream, const float* intensity,
                 const float* kernel, const void* data, const unsigned char* measured,
                 const float* upstream, double* partials, long nframe, int det, double inv) {
#define TK_BLUR_SUMS(KK)                                                                  \
  hipLaunchKernelGGL((blur_sums_kernel<MODEL, U16, KK, GRAD>), grid, dim3(256), 0, stream, \
                     intensity, kernel, data, measured, upstream, partials, nframe, det, inv)
  if (k == 3)
    TK_BLUR_SUMS(3);
  else if (k == 5)
    TK_BLUR_SUMS(5);
  else
    TK_BLUR_SUMS(7);
#undef TK_BLUR_SUMS
}

}  // namespace

extern "C" int tike_blur_cost_factor(const float* intensity, const float* kernel, int k,
                                     const void* data, int data_u16,
                                     const unsigned char* measured, const float* upstream,
                                     float* costs, float* table, float* blurred, long nframe,
                                     int det, int model, long num_measured, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(intensity && kernel);
  TK_CHECK_ARG(k == 3 || k == 5 || k == 7);
  TK_CHECK_ARG(det >= k);
  TK_CHECK_ARG(nframe >= 0);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  TK_CHECK_ARG(data || (!costs && !table));
  if (nframe == 0) return TK_OK;
  TK_CHECK_ARG(nframe <= 0x7fffffffL);  // one workgroup per frame: grid.x
  const double inv = 1.0 / (double)num_measured;
  const dim3 grid((unsigned)nframe);
  // without counts only `blurred` is formed, and no model formula runs
  const void* d = (costs || table) ? data : nullptr;
#define TK_BLUR_ARGS k, grid, stream, intensity, kernel, d, measured, upstream, costs, table, \
                     blurred, det, inv
  if (model == 0 && data_u16)
    cost_factor_launch<0, true>(TK_BLUR_ARGS);
  else if (model == 0)
    cost_factor_launch<0, false>(TK_BLUR_ARGS);
  else if (data_u16)
    cost_factor_launch<1, true>(TK_BLUR_ARGS);
  else
    cost_factor_launch<1, false>(TK_BLUR_ARGS);
#undef TK_BLUR_ARGS
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_blur_kernel_sums_partials(int det, int k) {
  if (!(k == 3 || k == 5 || k == 7) || det < k) return 0;
  const long n = sums_tiles(det) * SPLITS * (1 + (long)k * k);
  return n <= 0x7fffffffL ? (int)n : 0;
}

extern "C" int tike_blur_kernel_sums(const float* intensity, const float* kernel, int k,
                                     const void* data, int data_u16,
                                     const unsigned char* measured, const float* upstream,
                                     double* partials, double* kgrad, long nframe, int det,
                                     int model, long num_measured, void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(intensity && kernel && data && partials);
  TK_CHECK_ARG(k == 3 || k == 5 || k == 7);
  TK_CHECK_ARG(det >= k);
  TK_CHECK_ARG(nframe >= 0);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  if (nframe == 0) return TK_OK;
  const long tiles = sums_tiles(det);
  TK_CHECK_ARG(tike_blur_kernel_sums_partials(det, k) > 0);  // grid.x and the partials fit
  const double inv = 1.0 / (double)num_measured;
  const dim3 grid((unsigned)tiles, SPLITS);
#define TK_BLUR_ARGS k, grid, stream, intensity, kernel, data, measured, upstream, partials, \
                     nframe, det, inv
#define TK_BLUR_GRAD(M, U)                 \
  do {                                     \
    if (kgrad != nullptr)                  \
      sums_launch<M, U, true>(TK_BLUR_ARGS);  \
    else                                   \
      sums_launch<M, U, false>(TK_BLUR_ARGS); \
  } while (0)
  if (model == 0 && data_u16)
    TK_BLUR_GRAD(0, true);
  else if (model == 0)
    TK_BLUR_GRAD(0, false);
  else if (data_u16)
    TK_BLUR_GRAD(1, true);
  else
    TK_BLUR_GRAD(1, false);
#undef TK_BLUR_GRAD
#undef TK_BLUR_ARGS
  TK_LAUNCH_CHECK();
  if (kgrad != nullptr) {
    hipLaunchKernelGGL(blur_kgrad_finish_kernel, dim3(1), dim3(64), 0, stream,
                       (const double*)partials, kgrad, tiles * SPLITS, k * k);
    TK_LAUNCH_CHECK();
  }
  return TK_OK;
}
