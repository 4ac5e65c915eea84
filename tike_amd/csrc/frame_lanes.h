// What the kernels in which a lane owns four consecutive pixels of a frame and
// walks its planes share: ONE home for farplane_scale_kernel (autograd.hip),
// intensity_tangent_kernel (autograd_jvp.hip), cost_factor_kernel and
// cost_curvature_kernel (autograd_cost.hip), fly_farplane_gradient_kernel
// (fly.hip) and position_pd_sums_kernel (position_pd.hip).
#pragma once

#include "common.h"

// 16-, 8- and 4-byte accesses whose ADDRESS is only as aligned as an element:
// a plane or a row starts at a multiple of npix elements, which is a multiple
// of the vector's size only when npix is a multiple of the vector width.
// gfx950 under HSA serves misaligned global accesses; the type tells the
// compiler not to assume more.
typedef float tk_f4a8 __attribute__((ext_vector_type(4), aligned(8)));  // two cf
typedef float tk_f4a4 __attribute__((ext_vector_type(4), aligned(4)));  // four floats
typedef unsigned short tk_h4a2 __attribute__((ext_vector_type(4), aligned(2)));
typedef unsigned char tk_m4a1 __attribute__((ext_vector_type(4), aligned(1)));

// The counts of the four pixels at p, uint16 or float32.
template <bool U16>
__device__ __forceinline__ void tk_counts4(const void* __restrict__ data, long p, float (&d)[4]) {
  if (U16) {
    const tk_h4a2 c = *reinterpret_cast<const tk_h4a2*>((const unsigned short*)data + p);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = (float)c[k];
  } else {
    const tk_f4a4 c = *reinterpret_cast<const tk_f4a4*>((const float*)data + p);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = c[k];
  }
}

// Which of the four pixels at p are measured.
__device__ __forceinline__ void tk_mask4(const unsigned char* __restrict__ mask, long p,
                                         bool (&measured)[4]) {
  const tk_m4a1 m = *reinterpret_cast<const tk_m4a1*>(mask + p);
#pragma unroll
  for (int k = 0; k < 4; ++k) measured[k] = m[k] != 0;
}
