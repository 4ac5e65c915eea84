// Position correction of the least-squares + gradient update loop for gfx950:
// per position, the sums of the least-squares shift along the two Gaussian
// derivatives of the object patch.
//
// Reference:
//   ptycho/solvers/lstsq.py:545-579 + ptycho/position.py:779-810, mode 0 -> tike_position_sums
//   ptycho/solvers/rpie.py:508-548, the same summed over every mode      -> tike_rpie_position_sums
#include "internal.h"
#include "tike_amd.h"

// ------------------------------------------------------- position correction
// lstsq.py:545-579.  Per position n (mode m = 0, central window [crop, pw-crop)):
//   gx = gaussian derivative of the object patch along rows, gy along columns
//        (position.py:779-810: scipy gaussian_filter1d(-x, order=1, mode
//        'nearest'); the taps come precomputed from the host),
//   num[n] = ( sum Re(conj(gx P) chi), sum Re(conj(gy P) chi) ),
//   den[n] = ( sum |gx P|^2,           sum |gy P|^2 ),    P = probe_n mode 0.
// One workgroup per position.
struct TkTaps {
  float t[9];
  int r;
};

template <int RT>  // tap radius at compile time (-1: taps.r), so that the 2 (2 r + 1) tap
                   // loads of a pixel are requested together with its probe and chi values
__global__ __launch_bounds__(256) void position_sums_kernel(
    const cf* __restrict__ patches, const cf* __restrict__ chi, int chi_modes,
    const TkProbe probe, const TkTaps taps, float* __restrict__ num, float* __restrict__ den,
    int pw, int nsplit) {
  __shared__ float red[4];
  // work item = (position, 1 / nsplit of the window): see step_stats_kernel
  const long n = blockIdx.x / nsplit;
  const int part = blockIdx.x % nsplit;
  const long P = (long)pw * pw;
  const cf* __restrict__ O = patches + n * P;
  const cf* __restrict__ X = chi + n * chi_modes * P;
  const int crop = pw / 4;
  const int w = pw - 2 * crop;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  const int ilen = (w * w + nsplit - 1) / nsplit;
  const int iend = min(w * w, (part + 1) * ilen);
  for (int i = part * ilen + threadIdx.x; i < iend; i += blockDim.x) {
    const int y = crop + i / w, x = crop + i % w;
    cf gx = mk(0.f, 0.f), gy = mk(0.f, 0.f);
    const long pix = (long)y * pw + x;
    const cf Pm = probe.at(n, 0, pix);
    const cf c = X[pix];
    auto tap = [&](int d, int r) {
      const float t = taps.t[d + r];
      int yy = y + d, xx = x + d;
      yy = yy < 0 ? 0 : (yy >= pw ? pw - 1 : yy);
      xx = xx < 0 ? 0 : (xx >= pw ? pw - 1 : xx);
      const cf oy = O[yy * pw + x], ox = O[y * pw + xx];
      gx.x += t * oy.x;
      gx.y += t * oy.y;
      gy.x += t * ox.x;
      gy.y += t * ox.y;
    };
    if (RT >= 0) {
#pragma unroll
      for (int d = -RT; d <= RT; ++d) tap(d, RT);
    } else {
      for (int d = -taps.r; d <= taps.r; ++d) tap(d, taps.r);
    }
    const cf px = gx * Pm, py = gy * Pm;
    a[0] += px.x * c.x + px.y * c.y;
    a[1] += py.x * c.x + py.y * c.y;
    a[2] += norm2(px);
    a[3] += norm2(py);
  }
  for (int k = 0; k < 4; ++k) a[k] = tk_block_sum256(a[k], red);
  if (threadIdx.x == 0) {
    if (nsplit > 1) {
      unsafeAtomicAdd(&num[2 * n], a[0]);
      unsafeAtomicAdd(&num[2 * n + 1], a[1]);
      unsafeAtomicAdd(&den[2 * n], a[2]);
      unsafeAtomicAdd(&den[2 * n + 1], a[3]);
    } else {
      num[2 * n] = a[0];
      num[2 * n + 1] = a[1];
      den[2 * n] = a[2];
      den[2 * n + 1] = a[3];
    }
  }
}

// Radius 2, two positions per work item, row walk (see step_stats_pair_kernel):
// a thread keeps its column of the central window and goes down the rows of
// its share with the five vertical taps of each position in registers -- one
// new 8-byte load per pixel instead of five -- the four horizontal neighbours
// come as two 16-byte loads, and a shared probe is loaded once for the pair:
// 9 loads per pixel pair instead of 24.  cols = min(w, 256) columns per thread
// group, 256 / cols groups stacked over the rows.
__global__ __launch_bounds__(256) void position_sums_pair_kernel(
    const cf* __restrict__ patches, const cf* __restrict__ chi, int chi_modes,
    const TkProbe probe, const TkTaps taps, float* __restrict__ num, float* __restrict__ den,
    int pw, int nscan, int nsplit) {
  __shared__ float red[4];
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const long P = (long)pw * pw;
  const int crop = pw / 4;
  const int w = pw - 2 * crop;
  const int cols = w < 256 ? w : 256, groups = 256 / cols, rows = w / (nsplit * groups);
  const int npair = (nscan + 1) / 2;
  const bool shared = probe.weights == nullptr && probe.pos_stride == 0;
  const float t0 = taps.t[0], t1 = taps.t[1], t2 = taps.t[2], t3 = taps.t[3], t4 = taps.t[4];
  auto ld16 = [](const cf* p) {
    tk_v4f v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
  };
  auto add = [&](float* a, const cf (&v)[5], const tk_v4f hl, const tk_v4f hr, const cf Pm,
                 const cf c) {
    cf gx = mk(t0 * v[0].x, t0 * v[0].y), gy = mk(t0 * hl.x, t0 * hl.y);
    gx.x += t1 * v[1].x;
    gx.y += t1 * v[1].y;
    gy.x += t1 * hl.z;
    gy.y += t1 * hl.w;
    gx.x += t2 * v[2].x;
    gx.y += t2 * v[2].y;
    gy.x += t2 * v[2].x;
    gy.y += t2 * v[2].y;
    gx.x += t3 * v[3].x;
    gx.y += t3 * v[3].y;
    gy.x += t3 * hr.x;
    gy.y += t3 * hr.y;
    gx.x += t4 * v[4].x;
    gx.y += t4 * v[4].y;
    gy.x += t4 * hr.z;
    gy.y += t4 * hr.w;
    const cf px = gx * Pm, py = gy * Pm;
    a[0] += px.x * c.x + px.y * c.y;
    a[1] += py.x * c.x + py.y * c.y;
    a[2] += norm2(px);
    a[3] += norm2(py);
  };
  for (int item = blockIdx.x; item < npair * nsplit; item += gridDim.x) {
    const long n0 = 2 * (item / nsplit);
    const int part = item % nsplit;
    const bool two = n0 + 1 < nscan;
    const long n1 = two ? n0 + 1 : n0;
    const cf* __restrict__ O0 = patches + n0 * P;
    const cf* __restrict__ O1 = patches + n1 * P;
    const cf* __restrict__ X0 = chi + n0 * chi_modes * P;
    const cf* __restrict__ X1 = chi + n1 * chi_modes * P;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    const int ybeg = crop + (part * groups + (int)threadIdx.x / cols) * rows;
    for (int x = crop + (int)threadIdx.x % cols; x < crop + w; x += 256) {
      cf u[5], v[5];  // rows y - 2 .. y + 2 of column x, positions n0 / n1
#pragma unroll
      for (int d = 1; d < 5; ++d) {
        u[d] = O0[(ybeg - 3 + d) * pw + x];
        v[d] = O1[(ybeg - 3 + d) * pw + x];
      }
      for (int y = ybeg; y < ybeg + rows; ++y) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          u[d] = u[d + 1];
          v[d] = v[d + 1];
        }
        const int pix = y * pw + x;
        u[4] = O0[pix + 2 * pw];
        v[4] = O1[pix + 2 * pw];
        const tk_v4f ul = ld16(O0 + pix - 2), ur = ld16(O0 + pix + 1);
        const tk_v4f vl = ld16(O1 + pix - 2), vr = ld16(O1 + pix + 1);
        const cf c0 = X0[pix], c1 = X1[pix];
        const cf P0 = probe.at(n0, 0, pix);
        const cf P1 = shared ? P0 : probe.at(n1, 0, pix);
        add(a, u, ul, ur, P0, c0);
        add(b, v, vl, vr, P1, c1);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = tk_block_sum256(a[k], red);
      b[k] = tk_block_sum256(b[k], red);
    }
    if (threadIdx.x == 0) {
      if (nsplit > 1) {
        unsafeAtomicAdd(&num[2 * n0], a[0]);
        unsafeAtomicAdd(&num[2 * n0 + 1], a[1]);
        unsafeAtomicAdd(&den[2 * n0], a[2]);
        unsafeAtomicAdd(&den[2 * n0 + 1], a[3]);
        if (two) {
          unsafeAtomicAdd(&num[2 * n1], b[0]);
          unsafeAtomicAdd(&num[2 * n1 + 1], b[1]);
          unsafeAtomicAdd(&den[2 * n1], b[2]);
          unsafeAtomicAdd(&den[2 * n1 + 1], b[3]);
        }
      } else {
        num[2 * n0] = a[0];
        num[2 * n0 + 1] = a[1];
        den[2 * n0] = a[2];
        den[2 * n0 + 1] = a[3];
        if (two) {
          num[2 * n1] = b[0];
          num[2 * n1 + 1] = b[1];
          den[2 * n1] = b[2];
          den[2 * n1 + 1] = b[3];
        }
      }
    }
  }
}

extern "C" int tike_position_sums(const void* patches, const void* chi, int chi_modes,
                                  const void* probe, const void* eigen_probe,
                                  const float* eigen_weights, int num_eigen, int eigen_modes,
                                  const float* taps_host, int radius, float* numerator,
                                  float* denominator, int nscan, int S, int pw, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 4 && chi_modes >= 1 && radius >= 0 && radius <= 4);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(patches && chi && probe && taps_host && numerator && denominator);
  TkTaps taps;
  taps.r = radius;
  for (int k = 0; k < 9; ++k) taps.t[k] = k <= 2 * radius ? taps_host[k] : 0.f;
  const TkProbe pr =
      tk_make_probe(probe, 0, eigen_probe, eigen_weights, num_eigen, eigen_modes, S, pw);
  // the pair kernel: radius 2, a window whose columns tile 256 threads
  const int win = pw - 2 * (pw / 4), wcols = win < 256 ? win : 256;
  const bool pairs = g_stats_pairs && radius == 2 && pw >= 16 && nscan > 1 &&
                     (win % 256 == 0 || 256 % win == 0) && win % (256 / wcols) == 0;
  const long nitem = pairs ? (nscan + 1) / 2 : nscan;
  int nsplit = 1;
  while (nsplit < 16 && nitem * nsplit * 2 <= 8192 && pw >= 64 &&
         (!pairs || win % (2 * nsplit * (256 / wcols)) == 0))
    nsplit *= 2;
  if (tk_deterministic()) nsplit = 1;
  if (nsplit > 1) {
    hipError_t e = hipMemsetAsync(numerator, 0, sizeof(float) * 2 * (size_t)nscan,
                                  (hipStream_t)stream);
    if (e == hipSuccess)
      e = hipMemsetAsync(denominator, 0, sizeof(float) * 2 * (size_t)nscan, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  if (pairs)
    hipLaunchKernelGGL(position_sums_pair_kernel, dim3(tk_grid(nitem * nsplit, 16)), dim3(256), 0,
                       (hipStream_t)stream, (const cf*)patches, (const cf*)chi, chi_modes, pr,
                       taps, numerator, denominator, pw, nscan, nsplit);
  else if (radius == 2)  // position.py:779-810: sigma = 0.333, truncate 4 -> radius 2
    hipLaunchKernelGGL(position_sums_kernel<2>, dim3((unsigned)nscan * nsplit), dim3(256), 0,
                       (hipStream_t)stream, (const cf*)patches, (const cf*)chi, chi_modes, pr,
                       taps, numerator, denominator, pw, nsplit);
  else
    hipLaunchKernelGGL(position_sums_kernel<-1>, dim3((unsigned)nscan * nsplit), dim3(256), 0,
                       (hipStream_t)stream, (const cf*)patches, (const cf*)chi, chi_modes, pr,
                       taps, numerator, denominator, pw, nsplit);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ------------------------------------------- position correction, every mode
// rpie.py:508-548 (the sums the reference sketches for rPIE): as above, but
// summed over ALL probe modes.  chi of the modes above 0 is stored by no
// gradient route, and it need not be:
//   sum_s Re(conj(g P_s) chi_s) = Re(conj(g) sum_s conj(P_s) chi_s) = Re(conj(g) objproj)
//   sum_s |g P_s|^2             = |g|^2 sum_s |P_s|^2
// with objproj[n] the input of tike_scatter_patches.  The object patch is not
// read from memory either: its Gaussian derivatives are taken from psi, the
// bilinear interpolation folded into the taps (both are linear).

// out[pix] = sum_s |probe[s][pix]|^2 of a shared probe, once per call
__global__ __launch_bounds__(256) void probe_intensity_kernel(const cf* __restrict__ probe,
                                                              float* __restrict__ out, int S,
                                                              long P) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < P;
       i += (long)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += norm2(probe[s * P + i]);
    out[i] = acc;
  }
}

struct TkPatchOrigin {
  const cf* img;  // psi at the patch's minimum corner
  float fy, fx;
};

// (a corner outside check_allowed_positions is moved inside: the caller
// refuses such positions, this kernel never reads outside psi for them)
__device__ __forceinline__ TkPatchOrigin tk_patch_origin(const cf* __restrict__ psi,
                                                         const float* __restrict__ scan, long n,
                                                         int pw, int H, int W) {
  const float y = scan[2 * n], x = scan[2 * n + 1];
  const float fy0 = floorf(y), fx0 = floorf(x);
  int sy = (int)fy0, sx = (int)fx0;
  sy = sy < 0 ? 0 : (sy > H - pw - 1 ? H - pw - 1 : sy);
  sx = sx < 0 ? 0 : (sx > W - pw - 1 ? W - pw - 1 : sx);
  TkPatchOrigin o;
  o.img = psi + (long)sy * W + sx;
  o.fy = y - fy0;
  o.fx = x - fx0;
  return o;
}

__device__ __forceinline__ float tk_probe_intensity(const TkProbe& probe, long n, long pix) {
  float acc = 0.f;
  for (int s = 0; s < probe.S; ++s) acc += norm2(probe.at(n, s, pix));
  return acc;
}

__device__ __forceinline__ void tk_sums_store(float* __restrict__ num, float* __restrict__ den,
                                              long n, const float (&a)[4], bool atomic) {
  if (atomic) {
    unsafeAtomicAdd(&num[2 * n], a[0]);
    unsafeAtomicAdd(&num[2 * n + 1], a[1]);
    unsafeAtomicAdd(&den[2 * n], a[2]);
    unsafeAtomicAdd(&den[2 * n + 1], a[3]);
  } else {
    num[2 * n] = a[0];
    num[2 * n + 1] = a[1];
    den[2 * n] = a[2];
    den[2 * n + 1] = a[3];
  }
}

// Any window, any radius <= 4 (pw < 8: the window is closer to the patch
// border than the taps reach, edge mode 'nearest' ON THE PATCH): every tap is
// a bilinear gather of its own.  One workgroup per position.
template <bool SHARED>
__global__ __launch_bounds__(256) void rpie_position_sums_edge_kernel(
    const cf* __restrict__ objproj, const cf* __restrict__ psi, const float* __restrict__ scan,
    const float* __restrict__ inten, const TkProbe probe, const TkTaps taps,
    float* __restrict__ num, float* __restrict__ den, int pw, int H, int W, long nscan) {
  __shared__ float red[4];
  const long P = (long)pw * pw;
  const int crop = pw / 4;
  const int w = pw - 2 * crop;
  for (long n = blockIdx.x; n < nscan; n += gridDim.x) {
    const TkPatchOrigin o = tk_patch_origin(psi, scan, n, pw, H, W);
    const float w00 = (1.f - o.fx) * (1.f - o.fy), w01 = o.fx * (1.f - o.fy);
    const float w10 = (1.f - o.fx) * o.fy, w11 = o.fx * o.fy;
    auto patch = [&](int yy, int xx) {
      yy = yy < 0 ? 0 : (yy >= pw ? pw - 1 : yy);
      xx = xx < 0 ? 0 : (xx >= pw ? pw - 1 : xx);
      const cf* __restrict__ p = o.img + (long)yy * W + xx;
      const cf a = p[0], b = p[1], d = p[W], e = p[W + 1];
      return mk(a.x * w00 + b.x * w01 + d.x * w10 + e.x * w11,
                a.y * w00 + b.y * w01 + d.y * w10 + e.y * w11);
    };
    const cf* __restrict__ X = objproj + n * P;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < w * w; i += blockDim.x) {
      const int y = crop + i / w, x = crop + i % w;
      const long pix = (long)y * pw + x;
      cf gx = mk(0.f, 0.f), gy = mk(0.f, 0.f);
      for (int d = -taps.r; d <= taps.r; ++d) {
        const float t = taps.t[d + taps.r];
        const cf oy = patch(y + d, x), ox = patch(y, x + d);
        gx.x += t * oy.x;
        gx.y += t * oy.y;
        gy.x += t * ox.x;
        gy.y += t * ox.y;
      }
      const cf c = X[pix];
      const float I = SHARED ? inten[pix] : tk_probe_intensity(probe, n, pix);
      a[0] += gx.x * c.x + gx.y * c.y;
      a[1] += gy.x * c.x + gy.y * c.y;
      a[2] += norm2(gx) * I;
      a[3] += norm2(gy) * I;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = tk_block_sum256(a[k], red);
    if (threadIdx.x == 0) tk_sums_store(num, den, n, a, false);
  }
}

// Radius 2, pw >= 8 (no tap leaves the patch).  A thread owns a column x of the
// central window and walks down the rows of its share.  Each image row r is
// loaded once, as three 16-byte loads psi[r][x - 2 .. x + 3]; with the
// horizontal interpolation folded into the taps,
//   hc(r) = (1 - fx) psi[r][x] + fx psi[r][x + 1]            (the column itself)
//   hr(r) = sum_k u[k] psi[r][x - 2 + k], u[k] = (1 - fx) t[k] + fx t[k - 1]
// and two consecutive rows give the patch and its derivative along the row:
//   O(y, x) = (1 - fy) hc(y) + fy hc(y + 1),  gy(y, x) = (1 - fy) hr(y) + fy hr(y + 1).
// The five O of the vertical taps stay in registers.  Per pixel: 3 x 16 bytes
// of psi (L2), 8 of objproj, 4 of the probe intensity.
// cols = min(w, 256) columns per thread group, 256 / cols groups (and nsplit
// workgroups) stacked over the rows.
template <bool SHARED>
__global__ __launch_bounds__(256) void rpie_position_sums_kernel(
    const cf* __restrict__ objproj, const cf* __restrict__ psi, const float* __restrict__ scan,
    const float* __restrict__ inten, const TkProbe probe, const TkTaps taps,
    float* __restrict__ num, float* __restrict__ den, int pw, int H, int W, long nscan,
    int nsplit) {
  __shared__ float red[4];
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const long P = (long)pw * pw;
  const int crop = pw / 4;
  const int w = pw - 2 * crop;
  const int cols = w < 256 ? w : 256, groups = 256 / cols;
  const int slabs = nsplit * groups;
  const int rows = (w + slabs - 1) / slabs;
  const int group = (int)threadIdx.x / cols;
  const float t0 = taps.t[0], t1 = taps.t[1], t2 = taps.t[2], t3 = taps.t[3], t4 = taps.t[4];
  for (long item = blockIdx.x; item < nscan * nsplit; item += gridDim.x) {
    const long n = item / nsplit;
    const int part = (int)(item % nsplit);
    const TkPatchOrigin o = tk_patch_origin(psi, scan, n, pw, H, W);
    const float fx = o.fx, gx1 = 1.f - o.fx, fy = o.fy, gy1 = 1.f - o.fy;
    const float u0 = gx1 * t0, u1 = gx1 * t1 + fx * t0, u2 = gx1 * t2 + fx * t1,
                u3 = gx1 * t3 + fx * t2, u4 = gx1 * t4 + fx * t3, u5 = fx * t4;
    const cf* __restrict__ X = objproj + n * P;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    const int ybeg = crop + (part * groups + group) * rows;
    const int yend = min(crop + w, ybeg + rows);
    if (group < groups && ybeg < yend) {
      for (int x = crop + (int)threadIdx.x % cols; x < crop + w; x += cols) {
        // row r of the patch's footprint: hc, hr
        auto row = [&](int r, cf& hc, cf& hr) {
          const cf* __restrict__ p = o.img + (long)r * W + x;
          tk_v4f A, B, C;
          __builtin_memcpy(&A, p - 2, sizeof(A));
          __builtin_memcpy(&B, p, sizeof(B));
          __builtin_memcpy(&C, p + 2, sizeof(C));
          hc = mk(gx1 * B.x + fx * B.z, gx1 * B.y + fx * B.w);
          hr = mk(u0 * A.x + u1 * A.z + u2 * B.x + u3 * B.z + u4 * C.x + u5 * C.z,
                  u0 * A.y + u1 * A.w + u2 * B.y + u3 * B.w + u4 * C.y + u5 * C.w);
        };
        cf v[5], q[3];  // O(y - 2 .. y + 2, x); gy(y .. y + 2, x)
        cf hc0, hr0, hc1, hr1;
        row(ybeg - 2, hc0, hr0);
#pragma unroll
        for (int k = 1; k < 5; ++k) {  // O and gy of rows ybeg - 2 .. ybeg + 1
          row(ybeg - 2 + k, hc1, hr1);
          v[k] = mk(gy1 * hc0.x + fy * hc1.x, gy1 * hc0.y + fy * hc1.y);
          if (k >= 3) q[k - 2] = mk(gy1 * hr0.x + fy * hr1.x, gy1 * hr0.y + fy * hr1.y);
          hc0 = hc1;
          hr0 = hr1;
        }
        for (int y = ybeg; y < yend; ++y) {
#pragma unroll
          for (int d = 0; d < 4; ++d) v[d] = v[d + 1];
          q[0] = q[1];
          q[1] = q[2];
          row(y + 3, hc1, hr1);
          v[4] = mk(gy1 * hc0.x + fy * hc1.x, gy1 * hc0.y + fy * hc1.y);
          q[2] = mk(gy1 * hr0.x + fy * hr1.x, gy1 * hr0.y + fy * hr1.y);
          hc0 = hc1;
          hr0 = hr1;
          const long pix = (long)y * pw + x;
          const cf c = X[pix];
          const float I = SHARED ? inten[pix] : tk_probe_intensity(probe, n, pix);
          const cf gx = mk(t0 * v[0].x + t1 * v[1].x + t2 * v[2].x + t3 * v[3].x + t4 * v[4].x,
                           t0 * v[0].y + t1 * v[1].y + t2 * v[2].y + t3 * v[3].y + t4 * v[4].y);
          const cf gy = q[0];
          a[0] += gx.x * c.x + gx.y * c.y;
          a[1] += gy.x * c.x + gy.y * c.y;
          a[2] += norm2(gx) * I;
          a[3] += norm2(gy) * I;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = tk_block_sum256(a[k], red);
    if (threadIdx.x == 0) tk_sums_store(num, den, n, a, nsplit > 1);
  }
}

extern "C" int tike_rpie_position_sums(const void* objproj, const void* psi, const float* scan,
                                       const void* probe, int probe_per_scan,
                                       const void* eigen_probe, const float* eigen_weights,
                                       int num_eigen, int eigen_modes, const float* taps_host,
                                       int radius, float* intensity_work, float* numerator,
                                       float* denominator, int nscan, int S, int pw, int H, int W,
                                       void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 4 && radius >= 0 && radius <= 4);
  TK_CHECK_ARG(H >= pw + 2 && W >= pw + 2);
  TK_CHECK_ARG(!(probe_per_scan && eigen_weights));
  TK_CHECK_ARG(num_eigen >= 0 && eigen_modes >= 0 && eigen_modes <= S);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(objproj && psi && scan && probe && taps_host && numerator && denominator);
  TK_CHECK_ARG(!eigen_weights || num_eigen == 0 || (eigen_probe && eigen_modes >= 1));
  const bool shared = !probe_per_scan && !eigen_weights;
  TK_CHECK_ARG(!shared || intensity_work);
  TkTaps taps;
  taps.r = radius;
  for (int k = 0; k < 9; ++k) taps.t[k] = k <= 2 * radius ? taps_host[k] : 0.f;
  const TkProbe pr = tk_make_probe(probe, probe_per_scan, eigen_weights ? eigen_probe : nullptr,
                                   eigen_weights, num_eigen, eigen_modes, S, pw);
  hipStream_t st = (hipStream_t)stream;
  const long P = (long)pw * pw;
  if (shared) {
    hipLaunchKernelGGL(probe_intensity_kernel, dim3(tk_grid((P + 255) / 256, 16)), dim3(256), 0,
                       st, (const cf*)probe, intensity_work, S, P);
    TK_LAUNCH_CHECK();
  }
  const cf* X = (const cf*)objproj;
  const cf* O = (const cf*)psi;
  if (radius != 2 || pw < 8) {
    if (shared)
      hipLaunchKernelGGL(rpie_position_sums_edge_kernel<true>, dim3(tk_grid(nscan, 16)),
                         dim3(256), 0, st, X, O, scan, intensity_work, pr, taps, numerator,
                         denominator, pw, H, W, (long)nscan);
    else
      hipLaunchKernelGGL(rpie_position_sums_edge_kernel<false>, dim3(tk_grid(nscan, 16)),
                         dim3(256), 0, st, X, O, scan, intensity_work, pr, taps, numerator,
                         denominator, pw, H, W, (long)nscan);
    TK_LAUNCH_CHECK();
    return TK_OK;
  }
  // small batches: the window in nsplit slabs of at least 16 rows per thread
  // (a slab starts with five rows of its own), summed with float atomics
  const int win = pw - 2 * (pw / 4), groups = 256 / (win < 256 ? win : 256);
  int nsplit = 1;
  while (nsplit < 16 && (long)nscan * nsplit < 2048 && win / (groups * nsplit * 2) >= 16)
    nsplit *= 2;
  if (tk_deterministic()) nsplit = 1;  // one workgroup per position: no atomics
  if (nsplit > 1) {
    hipError_t e = hipMemsetAsync(numerator, 0, sizeof(float) * 2 * (size_t)nscan, st);
    if (e == hipSuccess) e = hipMemsetAsync(denominator, 0, sizeof(float) * 2 * (size_t)nscan, st);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid(tk_grid((long)nscan * nsplit, 16));
  if (shared)
    hipLaunchKernelGGL(rpie_position_sums_kernel<true>, grid, dim3(256), 0, st, X, O, scan,
                       intensity_work, pr, taps, numerator, denominator, pw, H, W, (long)nscan,
                       nsplit);
  else
    hipLaunchKernelGGL(rpie_position_sums_kernel<false>, grid, dim3(256), 0, st, X, O, scan,
                       intensity_work, pr, taps, numerator, denominator, pw, H, W, (long)nscan,
                       nsplit);
  TK_LAUNCH_CHECK();
  return TK_OK;
}
