// The strip / halo tap scheme of the bilinear patch and its two slopes: ONE
// home for tike_scan_gradient and tike_scan_gradient_slices (autograd.hip),
// tike_conv_fwd_tangent and tike_slice_wave_tangent (autograd_jvp.hip) and
// tike_eigen_wave_tangent (autograd_eigen_jvp.hip): the scheme, its device
// helpers (no kernel lives here) and the launch geometry of its item grids.
//
// A (rows, columns) plane of a position -- the patch, or the detector plane it
// is centred in -- is cut into ITEMS of ROWS rows x COLS columns, one per wave.
// A lane owns one OBJECT column of its item and walks down the STRIP: ROWS + 1
// object rows, each loaded once -- row y + 1 of pixel row y is row y of pixel
// row y + 1, and a row serves the patch, Dy, Dx and every mode alike.  The tap
// to the right comes from the next lane by wave shuffle.  What feeds the last
// lane decides COLS:
//   halo LANE    COLS = 63: lane 63 loads the column behind the item, only
//                feeds lane 62 and owns no pixel;
//   halo COLUMN  COLS = 64: every lane owns a pixel column, so a row segment of
//                an item is 512 contiguous bytes; the column behind the item
//                comes from ONE more load per lane (lane j its row j,
//                j <= ROWS; the other lanes repeat the last row), and lane 63
//                takes its right tap from there.
// With the taps
//   O00 = psi[sy + y][sx + x], O01 the pixel to its right, O10 the pixel below,
//   O11 below right, and the weights of tk_corner,
//   patch = w00 O00 + w01 O01 + w10 O10 + w11 O11
//   Dy = (1 - fx)(O10 - O00) + fx (O11 - O01)      d patch / d scan[n][0]
//   Dx = (1 - fy)(O01 - O00) + fy (O11 - O10)      d patch / d scan[n][1]
// (the integer part of the position held fixed).  Every load is unconditional
// (clamped address, value selected): a tap outside the object counts as zero
// and nothing outside the arrays is touched, whatever the positions.  Products
// are float32.
#pragma once

#include "common.h"
#include "tike_amd.h"

__device__ __forceinline__ cf tk_cf_lane_up(cf v) {  // lane i receives lane i + 1
  return mk(__shfl_down(v.x, 1, 64), __shfl_down(v.y, 1, 64));
}

// The tap to the right of a lane's own with a halo column: from the next lane,
// in lane COLS - 1 from the halo column, whose row j lane j holds.
template <int COLS>
__device__ __forceinline__ cf tk_right_tap(cf own, cf halo, int j, int lane) {
  const cf next = tk_cf_lane_up(own);
  const cf edge = mk(__shfl(halo.x, j, 64), __shfl(halo.y, j, 64));
  return lane == COLS - 1 ? edge : next;
}

// The bilinear patch pixel from its four taps, in the order of tk_gather.
__device__ __forceinline__ cf tk_bilinear(cf o00, cf o01, cf o10, cf o11, const TkCorner& c) {
  cf r = mk(o00.x * c.w00, o00.y * c.w00);
  r.x += o01.x * c.w01;
  r.y += o01.y * c.w01;
  r.x += o10.x * c.w10;
  r.y += o10.y * c.w10;
  r.x += o11.x * c.w11;
  r.y += o11.y * c.w11;
  return r;
}

// One component (real or imaginary) of a slope.  f is the fraction of the
// position ACROSS the slope's direction (fx for Dy, fy for Dx); a0 -> a1 are
// that component of the two taps along the direction on the near side (O00 ->
// O10 for Dy, O00 -> O01 for Dx), b0 -> b1 on the far side (O01 -> O11 for Dy,
// O10 -> O11 for Dx).  It takes floats, and a kernel calls it four times in
// the order Dy.re, Dy.im, Dx.re, Dx.im: a helper that takes the four taps as
// cf, or that forms both slopes of a component at once, changes the registers
// and the order of instructions of the tangent kernels.
__device__ __forceinline__ float tk_slope(float f, float a0, float a1, float b0, float b1) {
  return (1.0f - f) * (a1 - a0) + f * (b1 - b0);
}

// The tangent of a patch pixel: `t`, the bilinear sum of the tangent taps,
// plus dscan times the slopes.
__device__ __forceinline__ cf tk_patch_tangent(cf t, float dsy, float dyr, float dyi, float dsx,
                                               float dxr, float dxi) {
  t.x += dsy * dyr;
  t.y += dsy * dyi;
  t.x += dsx * dxr;
  t.y += dsx * dxi;
  return t;
}

// NOT here: the loads.  The strip load (ROWS + 1 clamped loads of a column,
// each with its selection; the object and its tangent interleaved in the
// tangent kernels) and the halo-column load stand in each of the five kernels
// -- the same text, the object's array and the names of ROWS / COLS apart.
// tools/kernel_identity.py decided it: every helper tried for them (the whole
// strip by reference with the column's test and clamp passed in or formed
// inside, one tap per call, one array or both, the row as one argument or
// two, the bare clamp) left scan_gradient_kernel alone at best and changed
// the registers or the instruction order of one to four of the others.  A
// helper is optimised on its own before it is inlined, and these short-circuit
// selections and clamps come out of that in another shape than they do in the
// kernel.  For the same reason the two scan-gradient kernels share their
// final reduction but not the loop over the items.

// Host side: the workgroups that serve the (extent, extent) plane of one
// position, four items of `rows` x `cols` each (one per wave), as a launch
// puts them into grid.y; 0 when the device takes no such grid.
static inline long tk_item_groups(int extent, int cols, int rows) {
  const long items = (long)((extent + cols - 1) / cols) * ((extent + rows - 1) / rows);
  const long groups = (items + 3) / 4;
  return groups <= (long)tike_max_grid_dim_y() ? groups : 0;
}
