// Internal (non-ABI) entry points shared between translation units.
#pragma once
#include "common.h"

int tk_fft2(const cf* in, cf* out, long ntile, int n, int inverse, float scale,
            hipStream_t stream);
// csrc/fft_mixed.hip: the shape-general engine (any n it supports; l_rows /
// l_cols = lines per workgroup group, 0 = planner's choice)
int tk_fft2_general(const cf* in, cf* out, long ntile, int n, int inverse, float scale,
                    int l_rows, int l_cols, hipStream_t stream);
int tk_conv_fwd(const cf* psi, const float* scan, const TkProbe& probe, cf* nearplane, int nscan,
                int S, int pw, int det, int H, int W, hipStream_t stream);
int tk_conv_adj(const cf* nearplane, const float* scan, const TkProbe& probe, cf* psi, int nscan,
                int S, int pw, int det, int H, int W, hipStream_t stream);
int tk_conv_adj_probe(const cf* nearplane, const float* scan, const cf* psi, cf* probe_adj,
                      int nscan, int S, int pw, int det, int H, int W, hipStream_t stream);

// csrc/adjoint.hip: pass 1 of the two-pass transform on plain tiles (out != in),
// and inverse pass 2 in place fused with the adjoint products
int tk_fft2_pass1(const cf* in, cf* out, long ntile, int det, bool inverse, bool keep,
                  hipStream_t stream);
int tk_ifft2_pass2_products(cf* work, const cf* psi, const float* scan, const cf* probe,
                            int probe_per_scan, cf* objproj, float* pnum, float pnum_scale,
                            cf* chi0, int out, int nscan, int S, int det, int H, int W,
                            float inv_scale, hipStream_t stream);

// csrc/forward.hip: the 128^2 forward operator, whole tile in LDS (a launch with
// *skip != 0 returns at once), and pass 1 of the 256^2 / 512^2 forward operator
// alone, which leaves the column-pass input of every tile in `scratch`
int launch_fwd128_lds(const cf* psi, const float* scan, const TkProbe& probe, cf* farplane,
                      float* intensity, int nscan, int S, int H, int W, float scale,
                      hipStream_t stream, cf* patches, const int* skip = nullptr);
int tk_fwd_pass1(const void* psi, const float* scan, const void* probe, int probe_per_scan,
                 const void* unique_probe, const void* eigen_probe, const float* eigen_weights,
                 int num_eigen, int eigen_modes, void* scratch, void* patches, int nscan, int S,
                 int pw, int det, int H, int W, hipStream_t stream, const int* skip,
                 bool keep = false);
// csrc/ptycho.hip: intensity, per-pattern cost and gradient factor from
// that column-pass input, or from a stored far plane
int tk_fwd_gradient_scale(const void* scratch, const void* data, int data_u16,
                          const unsigned char* measured, float* gscale, float* intensity,
                          float* costs, void* farplane, int nscan, int S, int det, float scale,
                          int model, float unmeasured_scaling, long num_measured,
                          hipStream_t stream, const int* skip);
int tk_farplane_gradient(void* farplane, const float* data, const unsigned char* measured,
                         float* intensity, float* costs, int nscan, int S, int det, int model,
                         int apply_gradient, float unmeasured_scaling, long num_measured,
                         hipStream_t stream, const int* skip);

// csrc/lstsq_gradients.hip: positions per chunk of a sum over positions (also
// the eigen pixel updates of csrc/lstsq.hip) and, in deterministic mode, where
// the chunks leave their partial sums
int probe_chunk(int nscan, long len = 0, float** part = nullptr);

// read by the probe preconditioner (csrc/lstsq_gradients.hip), the minibatch
// tail (lstsq.hip) and position correction (position_sums.hip): defined once,
// so that one replacement flips all three
#ifndef TK_STATS_PAIRS
#define TK_STATS_PAIRS 1  // build switch of the A/B (tools/build_variant.py)
#endif
static const bool g_stats_pairs = TK_STATS_PAIRS != 0;

// csrc/fft2.hip: the largest gridDim.y of a launch on the current device
// (hipDeviceAttributeMaxGridDimY; 0: the attribute could not be read).  Launches
// that put a position / tile count into y walk it in slices of at most this.
long tk_max_grid_y();
#define TK_GRID_Y_LIMIT(var)                           \
  const long var = tk_max_grid_y();                    \
  if (var < 1) return (int)hipErrorInvalidDevice

// ---- deterministic mode (tike_set_deterministic, fft2.hip).  Off: sums that
// several workgroups contribute to are float atomics (the reference's scheme,
// operators/cupy/convolution.cu:51-66): their order, and with it the last bits
// of every result, change from run to run.  On: every such sum has ONE
// contributor per address, or its partial sums go to the caller's scratch
// buffer and are added in a fixed order.
bool tk_deterministic();
// `bytes` of the caller's scratch buffer (nullptr when it is too small or the
// mode is off); one user at a time: launches are stream ordered
float* tk_det_scratch(size_t bytes);

// Per-pattern cost sink: costs[n] += v by one atomic per workgroup, or -- in
// deterministic mode -- part[n * nslots + slot] = v, summed in slot order by
// tk_cost_finish after the launch.
struct TkCostSink {
  float* costs;
  float* part;
  int nslots;
};
#if defined(__HIPCC__)
__device__ __forceinline__ void tk_cost_add(const TkCostSink& k, long n, int slot, float v) {
  if (k.part != nullptr)
    k.part[n * k.nslots + slot] = v;
  else
    unsafeAtomicAdd(&k.costs[n], v);
}
#endif
// sink for `nslots` contributors per pattern (zeroes costs when atomics are used)
int tk_cost_sink(float* costs, long nscan, int nslots, hipStream_t stream, TkCostSink* sink);
int tk_cost_finish(const TkCostSink& sink, long nscan, hipStream_t stream);
// out[i] (+)= sum_c part[c * n + i], c ascending
int tk_ordered_sum(float* out, const float* part, long n, int nparts, bool accumulate,
                   hipStream_t stream, int out_stride = 1);
