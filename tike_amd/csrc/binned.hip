// Detector binning: the far plane is modelled on a grid B times finer than the
// measured pixels, and a measured pixel is the incoherent sum over its B x B
// far-plane pixels (no reference counterpart: `binned_pix` in the reference's
// readers bins the data, never the model).  With det the far-plane width,
// w = det / B the data width and P = fly * S planes per frame:
//   I[f][U][V] = sum_{u<B} sum_{v<B} sum_{j<P} |far[f][j][U B + u][V B + v]|^2
//   gaussian: cost terms (sqrt(I) - sqrt(d))^2, factor 1 - sqrt(d) / (sqrt(I) + 1e-9)
//             (operators/cupy/objective.py:11-15, :31-44)
//   poisson:  cost terms I - d log(I + 1e-9),   factor 1 - d / (I + 1e-9)
//             (objective.py:72-74, :90-104)
// with a bin's count, mask and factor broadcast over its B x B pixels and the
// P planes.  The formulas live in noise_model.h; B = 1 is fly.hip's model and
// is forwarded there.
//
// Byte model per frame: P * det^2 * 8 bytes of far plane read once (and
// written once with the gradient), w^2 * 4 (or * 2) bytes of counts, w^2
// bytes of mask when there is one; the table of tike_binned_cost_factor adds
// det^2 * 4 bytes written.
#include "../../include/tike_amd.h"
#include "frame_lanes.h"
#include "noise_model.h"

// No contraction anywhere below: the helpers are inlined into every
// instantiation, and what the compiler fuses there must not decide the bits.
#pragma clang fp contract(off)

namespace {

enum { BIN_COSTS = 0, BIN_GRAD = 1, BIN_TABLE = 2 };

// A lane's segment of a far-plane row: PX = 4 pixels (two 16-byte loads, as in
// fly.hip) or PX = 2 (one).
template <int PX>
struct BinSeg {
  tk_f4a8 v[PX / 2];
  __device__ __forceinline__ void load(const cf* at) {
#pragma unroll
    for (int h = 0; h < PX / 2; ++h) v[h] = *reinterpret_cast<const tk_f4a8*>(at + 2 * h);
  }
  // pixels 2 h and 2 h + 1 times g[h]
  __device__ __forceinline__ void scale_store(cf* at, const float (&g)[2]) const {
#pragma unroll
    for (int h = 0; h < PX / 2; ++h) {
      tk_f4a8 a = v[h];
      const float gh = g[PX == 4 ? h : 0];
      a.x *= gh, a.y *= gh, a.z *= gh, a.w *= gh;
      *reinterpret_cast<tk_f4a8*>(at + 2 * h) = a;
    }
  }
  __device__ __forceinline__ void norms(float (&px)[PX]) const {
#pragma unroll
    for (int h = 0; h < PX / 2; ++h) {
      px[2 * h] += v[h].x * v[h].x + v[h].y * v[h].y;
      px[2 * h + 1] += v[h].z * v[h].z + v[h].w * v[h].w;
    }
  }
};

// One far-plane row of a lane's segment, its planes summed, folded into the
// lane's bins: the pixels of a bin's row are summed as a balanced tree -- pairs,
// pairs of pairs, across the LPB = B / PX lanes that share a bin when B > PX --
// so the bits do not depend on PX; every lane of a bin ends with the sum.
template <int VB, int PX>
__device__ __forceinline__ void bin_fold(float (&px)[PX], float (&I)[2]) {
  if constexpr (PX == 4 && VB == 2) {
    I[0] += px[0] + px[1];
    I[1] += px[2] + px[3];
  } else {
    float row = px[0] + px[1];
    if constexpr (PX == 4) row += px[2] + px[3];
#pragma unroll
    for (int o = 1; o < VB / PX; o <<= 1) row += __shfl_xor(row, o, 64);
    I[0] += row;
  }
#pragma unroll
  for (int k = 0; k < PX; ++k) px[k] = 0.f;
}

// One workgroup per frame.  VB in {2, 4, 8} (B == VB, det a multiple of 4): a
// lane owns PX consecutive far-plane pixels of the B rows of one bin row --
// 16-byte loads along a row, as in fly.hip -- and walks the P planes of each
// row.  A pixel's planes are summed first (planes ascending, as tike_intensity
// sums them), then the pixels of a bin's row (bin_fold), then the rows:
// partial sums stay short whatever B * B * P is.  With B > PX the B / PX
// neighbouring lanes of a bin add their row sums across lanes and the first of
// them owns the bin's cost and intensity.
// R > 0 (BIN_GRAD, B * P <= R): the B * P row-planes stay in registers between
// the intensity sum and the scaling -- the far plane is read from memory once.
// PX = 4 holds up to 16 row-planes (fly.hip's classes 4 / 8 / 16), PX = 2 up
// to 32 in the registers of the last class.  R == 0: the rows are read a
// second time for the scaling, within the same sweep of the workgroup.
// VB == 0: any B dividing det, any det: a lane owns one bin and walks its
// B x B pixels one by one.
// The frame's cost is summed in float64 in a fixed order (lane, wave shuffles,
// the four waves through LDS).  Contraction is off in this file so that the
// three modes and every register class give one set of bits.
template <int MODEL, int MODE, int VB, int R, int PX>
__global__ __launch_bounds__(256) void binned_kernel(
    cf* __restrict__ farplane, const void* __restrict__ data_, int u16,
    const unsigned char* __restrict__ mask, const float* __restrict__ upstream,
    float* __restrict__ intensity, float* __restrict__ costs, float* __restrict__ table, int P,
    int det, int B, float ums1, double inv_nmeasured) {
  constexpr int RR = R > 0 ? R : 1;
  __shared__ double red[4];
  const long n = blockIdx.x;
  const int w = det / B;
  const long npix = (long)det * det;
  const long nbin = (long)w * w;
  cf* __restrict__ F = farplane + n * P * npix;
  const float* __restrict__ d32 = (const float*)data_ + n * nbin;
  const unsigned short* __restrict__ d16 = (const unsigned short*)data_ + n * nbin;
  float* __restrict__ T = MODE == BIN_TABLE ? table + n * npix : nullptr;
  // upstream / num_measured, rounded once (tike_cost_factor's table)
  const float up =
      MODE == BIN_TABLE
          ? (float)((upstream != nullptr ? (double)upstream[n] : 1.0) * inv_nmeasured)
          : 0.f;
  double cost = 0.;

  if constexpr (VB > 0) {
    constexpr int NB = PX > VB ? PX / VB : 1;   // bins a lane's pixels touch
    constexpr int LPB = VB > PX ? VB / PX : 1;  // lanes that share a bin
    const int nv = det / PX;                    // lane segments per row
    const long nitem = (long)w * nv;
    const int BP = VB * P;
    // the LPB lanes of a bin are neighbours: nv is a multiple of LPB, so they
    // are in the same row and all inside nitem
    const bool owner = (threadIdx.x & (LPB - 1)) == 0;
    for (long v = threadIdx.x; v < nitem; v += blockDim.x) {
      const int U = (int)(v / nv);
      const int c = (int)(v - (long)U * nv) * PX;
      const long b0 = (long)U * w + c / VB;
      // the counts and the mask are requested with the planes, not behind them
      float d[NB];
      bool measured[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        d[k] = u16 ? (float)d16[b0 + k] : d32[b0 + k];
        measured[k] = mask != nullptr ? mask[b0 + k] != 0 : true;
      }
      cf* __restrict__ base = F + (long)U * VB * det + c;
      float I[2] = {0.f, 0.f};
      float px[PX];
#pragma unroll
      for (int k = 0; k < PX; ++k) px[k] = 0.f;
      BinSeg<PX> r[RR];
      if (MODE == BIN_GRAD && R > 0) {
        int u = 0, j = 0;
#pragma unroll
        for (int q = 0; q < RR; ++q) {
          if (q < BP) {
            r[q].load(base + j * npix + (long)u * det);
            if (++j == P) j = 0, ++u;
          }
        }
        j = 0;
#pragma unroll
        for (int q = 0; q < RR; ++q) {
          if (q < BP) {
            r[q].norms(px);
            if (++j == P) {
              j = 0;
              bin_fold<VB, PX>(px, I);
            }
          }
        }
      } else {
        for (int u = 0; u < VB; ++u) {
          for (int j = 0; j < P; ++j) {
            BinSeg<PX> a;
            a.load(base + j * npix + (long)u * det);
            a.norms(px);
          }
          bin_fold<VB, PX>(px, I);
        }
      }
      float g[2];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        float term;
        const float lp = tk_noise_pixel<MODEL>(I[k], d[k], term);
        cost += (measured[k] && owner) ? (double)term : 0.0;
        if (MODE == BIN_TABLE)
          g[k] = measured[k] ? up * lp : 0.0f;
        else
          g[k] = measured[k] ? -lp : ums1;
        if (intensity != nullptr && owner) intensity[n * nbin + b0 + k] = I[k];
      }
      if (NB == 1) g[1] = g[0];  // pixels 0, 1 take g[0], pixels 2, 3 g[1]
      if (MODE == BIN_GRAD && R > 0) {
        int u = 0, j = 0;
#pragma unroll
        for (int q = 0; q < RR; ++q) {
          if (q < BP) {
            r[q].scale_store(base + j * npix + (long)u * det, g);
            if (++j == P) j = 0, ++u;
          }
        }
      } else if (MODE == BIN_GRAD) {
        for (int u = 0; u < VB; ++u) {
          for (int j = 0; j < P; ++j) {
            cf* at = base + j * npix + (long)u * det;
            BinSeg<PX> a;
            a.load(at);
            a.scale_store(at, g);
          }
        }
      } else if (MODE == BIN_TABLE) {
        // (BIN_TABLE and BIN_COSTS run with PX == 4)
        tk_f4a4 o;
        o.x = g[0], o.y = g[0], o.z = g[1], o.w = g[1];
        for (int u = 0; u < VB; ++u)
          *reinterpret_cast<tk_f4a4*>(T + ((long)U * VB + u) * det + c) = o;
      }
    }
  } else {
    // general path: one bin per lane, its B x B pixels one by one
    for (long v = threadIdx.x; v < nbin; v += blockDim.x) {
      const int U = (int)(v / w);
      const int V = (int)(v - (long)U * w);
      const float dv = u16 ? (float)d16[v] : d32[v];
      const bool measured = mask != nullptr ? mask[v] != 0 : true;
      const long at0 = (long)U * B * det + (long)V * B;
      float I = 0.f;
      for (int u = 0; u < B; ++u) {
        float row = 0.f;
        for (int c = 0; c < B; ++c) {
          float px = 0.f;
          for (int j = 0; j < P; ++j) {
            const cf a = F[j * npix + at0 + (long)u * det + c];
            px += a.x * a.x + a.y * a.y;
          }
          row += px;
        }
        I += row;
      }
      float term;
      const float lp = tk_noise_pixel<MODEL>(I, dv, term);
      cost += measured ? (double)term : 0.0;
      if (intensity != nullptr) intensity[n * nbin + v] = I;
      if (MODE == BIN_GRAD) {
        const float g = measured ? -lp : ums1;
        for (int u = 0; u < B; ++u)
          for (int c = 0; c < B; ++c)
            for (int j = 0; j < P; ++j) {
              cf* at = F + j * npix + at0 + (long)u * det + c;
              cf a = *at;
              a.x *= g, a.y *= g;
              *at = a;
            }
      } else if (MODE == BIN_TABLE) {
        const float g = measured ? up * lp : 0.0f;
        for (int u = 0; u < B; ++u)
          for (int c = 0; c < B; ++c) T[at0 + (long)u * det + c] = g;
      }
    }
  }
  if (costs != nullptr) {
    cost = tk_frame_sum_f64(cost, red);
    if (threadIdx.x == 0) costs[n] = (float)(cost * inv_nmeasured);
  }
}

struct BinArgs {
  cf* far;
  const void* data;
  int u16;
  const unsigned char* measured;
  const float* upstream;
  float* intensity;
  float* costs;
  float* table;
  long nframe;
  int P, det, B;
  float ums1;
  double inv;
  hipStream_t stream;
};

template <int MODEL, int MODE, int VB, int R, int PX = 4>
void bin_launch1(const BinArgs& a) {
  const dim3 grid((unsigned)a.nframe), block(256);
  hipLaunchKernelGGL((binned_kernel<MODEL, MODE, VB, R, PX>), grid, block, 0, a.stream, a.far,
                     a.data, a.u16, a.measured, a.upstream, a.intensity, a.costs, a.table, a.P,
                     a.det, a.B, a.ums1, a.inv);
}

// Costs only and the table walk the rows without keeping them.  The register
// class of a gradient launch: B * P row-planes per lane in the classes of
// fly.hip (4 / 8 / 16) with four pixels per lane, up to 32 in the registers of
// the last class with two pixels per lane, a second read above.
template <int MODEL, int VB>
void bin_launch_mode(const BinArgs& a, int mode) {
  const long BP = (long)VB * a.P;
  if (mode == BIN_COSTS) {
    bin_launch1<MODEL, BIN_COSTS, VB, 0>(a);
  } else if (mode == BIN_TABLE) {
    bin_launch1<MODEL, BIN_TABLE, VB, 0>(a);
  } else if constexpr (VB == 0) {
    bin_launch1<MODEL, BIN_GRAD, 0, 0>(a);
  } else if (BP <= 4) {
    if constexpr (VB <= 4) bin_launch1<MODEL, BIN_GRAD, VB, 4>(a);
  } else if (BP <= 8) {
    bin_launch1<MODEL, BIN_GRAD, VB, 8>(a);
  } else if (BP <= 16) {
    bin_launch1<MODEL, BIN_GRAD, VB, 16>(a);
  } else if (BP <= 32) {
    bin_launch1<MODEL, BIN_GRAD, VB, 32, 2>(a);
  } else {
    bin_launch1<MODEL, BIN_GRAD, VB, 0>(a);
  }
}

template <int MODEL>
void bin_launch(const BinArgs& a, int mode) {
  const bool vec = a.det % 4 == 0;
  if (vec && a.B == 2)
    bin_launch_mode<MODEL, 2>(a, mode);
  else if (vec && a.B == 4)
    bin_launch_mode<MODEL, 4>(a, mode);
  else if (vec && a.B == 8)
    bin_launch_mode<MODEL, 8>(a, mode);
  else
    bin_launch_mode<MODEL, 0>(a, mode);
}

}  // namespace

extern "C" int tike_binned_farplane_gradient(void* farplane, const void* data, int data_u16,
                                             const unsigned char* measured, float* intensity,
                                             float* costs, int nframe, int fly, int S, int det,
                                             int binning, int model, int apply_gradient,
                                             float unmeasured_scaling, long num_measured,
                                             void* stream_) {
  TK_ENTER();
  TK_CHECK_ARG(binning >= 1 && det >= 1 && det % binning == 0);
  if (binning == 1)
    return tike_fly_farplane_gradient(farplane, data, data_u16, measured, intensity, costs,
                                      nframe, fly, S, det, model, apply_gradient,
                                      unmeasured_scaling, num_measured, stream_);
  TK_CHECK_ARG(farplane && data);
  TK_CHECK_ARG(nframe >= 0 && fly >= 1 && S >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured > 0);
  TK_CHECK_ARG((long)fly * S <= 0x7fffffffL);
  if (nframe == 0) return TK_OK;
  const BinArgs a = {(cf*)farplane, data,   data_u16 != 0, measured, nullptr,
                     intensity,     costs,  nullptr,       nframe,   fly * S,
                     det,           binning, unmeasured_scaling - 1.0f, 1.0 / (double)num_measured,
                     (hipStream_t)stream_};
  const int mode = apply_gradient ? BIN_GRAD : BIN_COSTS;
  if (model == 0)
    bin_launch<0>(a, mode);
  else
    bin_launch<1>(a, mode);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_binned_cost_factor(const void* farplane, const void* data, int data_u16,
                                       const unsigned char* measured, const float* upstream,
                                       float* costs, float* table, long nframe, int P,
                                       long npix, int model, long num_measured, int det,
                                       int binning, void* stream_) {
  TK_ENTER();
  TK_CHECK_ARG(binning >= 1 && det >= 1 && det % binning == 0);
  TK_CHECK_ARG(npix == (long)det * det);
  if (binning == 1)
    return tike_cost_factor(farplane, data, data_u16, measured, upstream, costs, table, nframe,
                            P, npix, model, num_measured, stream_);
  TK_CHECK_ARG(farplane && data);
  TK_CHECK_ARG(nframe >= 0 && P >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured >= 1);
  if (nframe == 0) return TK_OK;
  TK_CHECK_ARG(nframe <= 0x7fffffffL);  // one workgroup per frame: grid.x
  // (the far plane is only read: BIN_COSTS and BIN_TABLE never store to it)
  const BinArgs a = {(cf*)farplane, data,  data_u16 != 0, measured, upstream,
                     nullptr,       costs, table,         nframe,   P,
                     det,           binning, 0.0f,        1.0 / (double)num_measured,
                     (hipStream_t)stream_};
  const int mode = table != nullptr ? BIN_TABLE : BIN_COSTS;
  if (model == 0)
    bin_launch<0>(a, mode);
  else
    bin_launch<1>(a, mode);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
