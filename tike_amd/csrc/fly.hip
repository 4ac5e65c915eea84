// Fly scans: `fly` consecutive scan positions expose one detector frame
// (reference ptycho/ptycho.py:95-125 and :128-179; operators/cupy/ptycho.py:
// 104-125).  Intensity, per-frame cost and the far-plane gradient factor of a
// frame in ONE pass over its fly * S far planes:
//   I_f = sum_{j < fly} sum_{m < S} |far[f * fly + j, m]|^2
//   gaussian: cost terms (sqrt(I) - sqrt(d))^2, factor 1 - sqrt(d) / (sqrt(I) + 1e-9)
//             (operators/cupy/objective.py:11-15, :31-44)
//   poisson:  cost terms I - d log(I + 1e-9),   factor 1 - d / (I + 1e-9)
//             (objective.py:72-74, :90-104)
// with the frame's counts and intensity broadcast over j and m.
//
// Byte model per frame, P = fly * S planes of npix pixels: P * npix * 8 bytes of
// far plane read once (and written once with apply_gradient), npix * 4 (or * 2)
// bytes of counts, npix bytes of mask when there is one.
#include "../../include/tike_amd.h"
#include "fly_frame.h"

namespace {

// The kernel, its register classes R and the fixed order of the cost sum are
// in fly_frame.h (shared with background.hip); here without a background.
template <int MODEL, bool U16>
void fly_launch(cf* far, const void* data, const unsigned char* measured, float* intensity,
                float* costs, int nframe, int P, long npix, int apply_gradient, float ums1,
                double inv, hipStream_t stream) {
  const dim3 grid((unsigned)nframe), block(256);
#define TK_FLY(G, R)                                                                          \
  hipLaunchKernelGGL((fly_farplane_gradient_kernel<MODEL, G, U16, R, false>), grid, block, 0, \
                     stream, far, data, measured, intensity, costs, P, npix, ums1, inv,      \
                     (const float*)nullptr)
  if (!apply_gradient)
    TK_FLY(false, 0);
  else if (P <= 4)
    TK_FLY(true, 4);
  else if (P <= 8)
    TK_FLY(true, 8);
  else if (P <= 16)
    TK_FLY(true, 16);
  else
    TK_FLY(true, 0);
#undef TK_FLY
}

}  // namespace

extern "C" int tike_fly_farplane_gradient(void* farplane, const void* data, int data_u16,
                                          const unsigned char* measured, float* intensity,
                                          float* costs, int nframe, int fly, int S, int det,
                                          int model, int apply_gradient,
                                          float unmeasured_scaling, long num_measured,
                                          void* stream_) {
  TK_ENTER();
  hipStream_t stream = (hipStream_t)stream_;
  TK_CHECK_ARG(farplane && data);
  TK_CHECK_ARG(nframe >= 0 && fly >= 1 && S >= 1 && det >= 1);
  TK_CHECK_ARG(model == 0 || model == 1);
  TK_CHECK_ARG(num_measured > 0);
  TK_CHECK_ARG((long)fly * S <= 0x7fffffffL);
  if (nframe == 0) return TK_OK;
  const int P = fly * S;
  const long npix = (long)det * det;
  const double inv = 1.0 / (double)num_measured;
  const float ums1 = unmeasured_scaling - 1.0f;
  cf* far = (cf*)farplane;
  if (model == 0 && data_u16)
    fly_launch<0, true>(far, data, measured, intensity, costs, nframe, P, npix, apply_gradient,
                        ums1, inv, stream);
  else if (model == 0)
    fly_launch<0, false>(far, data, measured, intensity, costs, nframe, P, npix, apply_gradient,
                         ums1, inv, stream);
  else if (data_u16)
    fly_launch<1, true>(far, data, measured, intensity, costs, nframe, P, npix, apply_gradient,
                        ums1, inv, stream);
  else
    fly_launch<1, false>(far, data, measured, intensity, costs, nframe, P, npix, apply_gradient,
                         ums1, inv, stream);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
