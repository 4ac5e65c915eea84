// The minibatch tail of the least-squares + gradient update loop (lstsq_grad)
// for gfx950 (the footprint scatter is scatter.hip, the two gradients and the
// probe preconditioner lstsq_gradients.hip, position correction
// position_sums.hip; this unit keeps the name of the file they were cut from,
// so that its history follows).
//
// Reference: src/tike/ptycho/solvers/lstsq.py (one minibatch):
//   :619-718  step-size normal equations, per position               -> tike_lstsq_step_stats
//   :721-738  eigen-probe intensity coefficients                     -> (same kernel)
//   :297-364,740-761 + ptycho/probe.py:362-476 eigen-probe update    -> tike_eigen_position_sums{,1}, tike_eigen_pixel_update{,1,1q},
//                                                                       tike_lstsq_step_stats_eigen1
//   ptycho/probe.py:272-303 varying probe                            -> tike_varying_probe
// where chi is the exit-wave update (IFFT2 of the far-plane gradient cropped
// to the probe window), P_n,s the probe at position n (shared probe plus
// eigen probes synthesised on the fly) and O_n the bilinear object patch.
#include <type_traits>

#include "internal.h"
#include "tike_amd.h"

// ------------------------------------------------- step-size normal equations
// One workgroup per position.  With m = 0 (lstsq.py:169):
//   dOP = patch_n(g) * P_n,0        g = preconditioned object update
//   dPO = mpu_0 * O_n               mpu = common probe update, O_n = patch_n(psi)
//   stats[n] = { sum|dOP|^2, sum|dPO|^2, Re sum dOP conj(dPO), Im sum dOP conj(dPO),
//                sum Re(conj(dOP) chi_n,0), sum Re(conj(dPO) chi_n,0),
//                sum Re(conj(O_n P_0) chi_n,0), sum |O_n P_0|^2 }
// (the last two feed _get_coefs_intensity, lstsq.py:721-738, which uses the
// SHARED probe P_0).  eps terms (:641,661,667) are added by the solver.
// the sums of work item (position n, part `part` of nsplit) -- the body of
// step_stats_kernel, also the fall-back of step_stats_pair_kernel
template <bool HAVE_PATCHES, bool HAVE_GOBJ>
__device__ __forceinline__ void step_stats_item(
    const cf* __restrict__ chi, const float* __restrict__ scan, const cf* __restrict__ psi,
    const cf* __restrict__ gobj, const TkProbe& probe, const cf* __restrict__ mpu,
    const cf* __restrict__ patches, float* __restrict__ stats, int chi_modes, int pw, int H,
    int W, const cf* __restrict__ eigen0, float* __restrict__ eigen_proj, int nsplit, int n,
    int part, float* red) {
  const long P = (long)pw * pw;
  const long total = (long)H * W;
  const int plen = (int)(P / nsplit);
  {
    const TkCorner c = tk_corner(scan, n);
    // the varying probe of mode 0 (probe.py:272-303): weights and bases are
    // per position, hoisted here (TkProbe::at re-read them for every pixel)
    const cf* __restrict__ pbase = probe.probe + n * probe.pos_stride;
    float pw0 = 1.0f, pw1 = 0.f;
    int nE = 0;
    const float* __restrict__ wn = nullptr;
    if (probe.weights != nullptr) {
      if (probe.unique != nullptr && 0 < probe.Sm) {
        pbase = probe.unique + (long)n * probe.Sm * P;
      } else {
        wn = probe.weights + n * (long)(probe.C + 1) * probe.S;
        pw0 = wn[0];
        if (probe.eigen != nullptr && 0 < probe.Sm) {
          nE = probe.C;
          pw1 = wn[probe.S];
        }
      }
    }
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float ep = 0.f;  // sum Re(conj(R_n) E_0), R_n = conj(O_n) chi_n,0 - mpu_0
    // branch-free body (clamped addresses, results zeroed by select) so that
    // the loads of two pixels are in flight together
    // (row, column) of the pixel advance with the stride instead of a
    // division per pixel
    const int qstep = (int)blockDim.x / pw, rstep = (int)blockDim.x % pw;
    const int pbeg = part * plen + (int)threadIdx.x;
    const int pend = part + 1 == nsplit ? (int)P : (part + 1) * plen;
    int py = pbeg / pw, px = pbeg % pw;
    // interior position (every tap of every pixel inside the image): the two
    // taps of a row are adjacent complex values, fetched with one 16-byte load
    const bool interior = HAVE_GOBJ && c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W &&
                          total < (1L << 28);
    // E_0 of the first eigen probe is the array the varying probe adds: one load
    const bool same_e = eigen_proj != nullptr && nE > 0 && eigen0 == probe.eigen;
    // ... and the shared probe P_0 is the base of the varying one unless a
    // synthesised array was given: one load serves both.
    const bool same_p = pbase == probe.probe;
    // The body is compiled for four cases.  A load behind a run-time
    // condition (`mpu ? mpu[p] : 0`, `same_e ? e1 : eigen0[p]`, the eigen
    // probes behind `nE > 0`) is a branch around the load, and the memory
    // latencies on either side of a branch add up: with the conditions of the
    // two common configurations settled at compile time every load of a pixel
    // is requested together (0.48 -> 0.36 ms per 1000 positions at 256^2).
    //   K = 0  any position, any configuration (clamped taps)
    //   K = 1  interior position, any configuration
    //   K = 2  interior, shared probe, no eigen probes, probe update given
    //   K = 3  interior, shared probe + ONE eigen probe whose projection is
    //          asked for (eigen0 is that eigen probe), probe update given
    auto body = [&](auto k_tag) {
      constexpr int K = decltype(k_tag)::value;
      constexpr bool FAST = K >= 1;
      constexpr bool HOT = K >= 2;
#pragma unroll 2
      for (int p = pbeg; p < pend; p += blockDim.x) {
        cf o, g;
        if (FAST) {
          typedef float tk_v4f __attribute__((ext_vector_type(4)));
          const unsigned off =
              (unsigned)((c.sy + py) * W + c.sx + px) * (unsigned)sizeof(cf);
          tk_v4f u, l;
          __builtin_memcpy(&u, reinterpret_cast<const char*>(gobj) + off, sizeof(u));
          __builtin_memcpy(&l, reinterpret_cast<const char*>(gobj) + off + (unsigned)W * 8u,
                           sizeof(l));
          if (HAVE_PATCHES) {
            o = patches[n * P + p];
          } else {
            // O_n from the object itself: the same two 16-byte tap loads at
            // the same offsets as the update's (L2) instead of 8 bytes of HBM
            tk_v4f uo, lo_;
            __builtin_memcpy(&uo, reinterpret_cast<const char*>(psi) + off, sizeof(uo));
            __builtin_memcpy(&lo_, reinterpret_cast<const char*>(psi) + off + (unsigned)W * 8u,
                             sizeof(lo_));
            o = mk(uo.x * c.w00, uo.y * c.w00);
            o.x += uo.z * c.w01;
            o.y += uo.w * c.w01;
            o.x += lo_.x * c.w10;
            o.y += lo_.y * c.w10;
            o.x += lo_.z * c.w11;
            o.y += lo_.w * c.w11;
          }
          g = mk(u.x * c.w00, u.y * c.w00);
          g.x += u.z * c.w01;
          g.y += u.w * c.w01;
          g.x += l.x * c.w10;
          g.y += l.y * c.w10;
          g.x += l.z * c.w11;
          g.y += l.w * c.w11;
        } else {
          const int y = c.sy + py, x = c.sx + px;
          const bool ok = y >= 0 && y < H && x >= 0 && x < W;
          const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
          const int xc = x < 0 ? 0 : (x >= W ? W - 1 : x);
          const long ii = (long)yc * W + xc;
          // O_n: the patch stored by tike_lstsq_gradients when available
          o = HAVE_PATCHES ? patches[n * P + p] : tk_gather(psi, ii, W, total, c);
          g = HAVE_GOBJ ? tk_gather(gobj, ii, W, total, c) : mk(0.f, 0.f);
          if (!ok) {
            if (!HAVE_PATCHES) o = mk(0.f, 0.f);
            g = mk(0.f, 0.f);
          }
        }
        const cf x0 = chi[((long)n * chi_modes) * P + p];
        const cf p0 = probe.probe[p];
        cf pn = (HOT ? p0 : pbase[p]) * pw0;
        cf e1 = mk(0.f, 0.f);
        if (K == 3) {
          e1 = probe.eigen[p];
          pn.x += pw1 * e1.x;
          pn.y += pw1 * e1.y;
        } else if (K < 2 && nE > 0) {
          e1 = probe.eigen[p];
          pn.x += pw1 * e1.x;
          pn.y += pw1 * e1.y;
          for (int e = 1; e < nE; ++e) {  // uniform, rare
            const cf ee = probe.eigen[(long)e * probe.Sm * P + p];
            const float we = wn[(e + 1) * probe.S];
            pn.x += we * ee.x;
            pn.y += we * ee.y;
          }
        }
        const cf dOP = g * pn;
        const cf m0 = HOT ? mpu[p] : (mpu ? mpu[p] : mk(0.f, 0.f));
        const cf dPO = m0 * o;
        const cf OP = o * p0;
        a[0] += norm2(dOP);
        a[1] += norm2(dPO);
        const cf a2 = dOP * conjf(dPO);
        a[2] += a2.x;
        a[3] += a2.y;
        a[4] += dOP.x * x0.x + dOP.y * x0.y;
        a[5] += dPO.x * x0.x + dPO.y * x0.y;
        a[6] += OP.x * x0.x + OP.y * x0.y;
        a[7] += norm2(OP);
        if (K == 3) {
          const cf r = conjf(o) * x0 - m0;
          ep += r.x * e1.x + r.y * e1.y;
        } else if (K < 2 && eigen_proj) {
          const cf r = conjf(o) * x0 - m0;
          const cf e = same_e ? e1 : eigen0[p];
          ep += r.x * e.x + r.y * e.y;
        }
        py += qstep;
        px += rstep;
        if (px >= pw) {
          px -= pw;
          ++py;
        }
      }
    };
    const bool hot = interior && same_p && mpu != nullptr;
    if (hot && nE == 1 && same_e)
      body(std::integral_constant<int, 3>{});
    else if (hot && nE == 0 && eigen_proj == nullptr)
      body(std::integral_constant<int, 2>{});
    else if (interior)
      body(std::integral_constant<int, 1>{});
    else
      body(std::integral_constant<int, 0>{});
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float t = tk_block_sum256(a[k], red);
      if (threadIdx.x == 0) {
        if (nsplit > 1)
          unsafeAtomicAdd(&stats[(long)n * 8 + k], t);
        else
          stats[(long)n * 8 + k] = t;
      }
    }
    if (eigen_proj) {
      const float t = tk_block_sum256(ep, red);
      if (threadIdx.x == 0) {
        if (nsplit > 1)
          unsafeAtomicAdd(&eigen_proj[n], t);
        else
          eigen_proj[n] = t;
      }
    }
  }
}

template <bool HAVE_PATCHES, bool HAVE_GOBJ>
__global__ __launch_bounds__(256) void step_stats_kernel(
    const cf* __restrict__ chi, const float* __restrict__ scan, const cf* __restrict__ psi,
    const cf* __restrict__ gobj, const TkProbe probe, const cf* __restrict__ mpu,
    const cf* __restrict__ patches, float* __restrict__ stats, int nscan, int chi_modes, int pw,
    int H, int W, const cf* __restrict__ eigen0, float* __restrict__ eigen_proj, int nsplit) {
  __shared__ float red[4];
  // work item = (position, 1 / nsplit of its pixels): a minibatch of a few
  // hundred positions would otherwise leave most of the chip idle; with
  // nsplit > 1 the sums are accumulated into the (zeroed) tables by atomics
  for (int v = blockIdx.x; v < nscan * nsplit; v += gridDim.x)
    step_stats_item<HAVE_PATCHES, HAVE_GOBJ>(chi, scan, psi, gobj, probe, mpu, patches, stats,
                                             chi_modes, pw, H, W, eigen0, eigen_proj, nsplit,
                                             v / nsplit, v % nsplit, red);
}

// Two positions per work item (the common configurations K = 2 / K = 3 of
// step_stats_item, stored patches and the preconditioned update given): the
// shared operands of a pixel -- P_0, the probe update and the eigen probe --
// are loaded once for both positions, 11 loads per pixel pair instead of 14.
// A pair with a position on the border falls back to step_stats_item.
template <bool EIGEN>
__global__ __launch_bounds__(256) void step_stats_pair_kernel(
    const cf* __restrict__ chi, const float* __restrict__ scan, const cf* __restrict__ psi,
    const cf* __restrict__ gobj, const TkProbe probe, const cf* __restrict__ mpu,
    const cf* __restrict__ patches, float* __restrict__ stats, int nscan, int chi_modes, int pw,
    int H, int W, const cf* __restrict__ eigen0, float* __restrict__ eigen_proj, int nsplit) {
  __shared__ float red[4];
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const long P = (long)pw * pw;
  const int plen = (int)(P / nsplit);
  const int npair = (nscan + 1) / 2;
  for (int v = blockIdx.x; v < npair * nsplit; v += gridDim.x) {
    const int n0 = 2 * (v / nsplit), part = v % nsplit;
    const TkCorner c0 = tk_corner(scan, n0);
    const bool two = n0 + 1 < nscan;
    const TkCorner c1 = tk_corner(scan, two ? n0 + 1 : n0);
    const bool in0 = c0.sy >= 0 && c0.sx >= 0 && c0.sy + pw < H && c0.sx + pw < W;
    const bool in1 = c1.sy >= 0 && c1.sx >= 0 && c1.sy + pw < H && c1.sx + pw < W;
    if (!(two && in0 && in1)) {  // uniform
      step_stats_item<true, true>(chi, scan, psi, gobj, probe, mpu, patches, stats, chi_modes,
                                  pw, H, W, eigen0, eigen_proj, nsplit, n0, part, red);
      if (two)
        step_stats_item<true, true>(chi, scan, psi, gobj, probe, mpu, patches, stats, chi_modes,
                                    pw, H, W, eigen0, eigen_proj, nsplit, n0 + 1, part, red);
      continue;
    }
    float s0 = 1.0f, s1 = 1.0f, t0 = 0.f, t1 = 0.f;  // weights of P_0 and of E_0
    if (probe.weights != nullptr) {
      const float* w = probe.weights + n0 * (long)(probe.C + 1) * probe.S;
      s0 = w[0];
      s1 = w[(long)(probe.C + 1) * probe.S];
      if (EIGEN) {
        t0 = w[probe.S];
        t1 = w[(long)(probe.C + 1) * probe.S + probe.S];
      }
    }
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float ea = 0.f, eb = 0.f;
    const int qstep = (int)blockDim.x / pw, rstep = (int)blockDim.x % pw;
    const int pbeg = part * plen + (int)threadIdx.x;
    const int pend = part + 1 == nsplit ? (int)P : (part + 1) * plen;
    int py = pbeg / pw, px = pbeg % pw;
    const unsigned base0 = (unsigned)(c0.sy * W + c0.sx), base1 = (unsigned)(c1.sy * W + c1.sx);
    const cf* __restrict__ chi_a = chi + ((long)n0 * chi_modes) * P;
    const cf* __restrict__ chi_b = chi + ((long)(n0 + 1) * chi_modes) * P;
    const cf* __restrict__ pat_a = patches + (long)n0 * P;
    const cf* __restrict__ pat_b = pat_a + P;
    auto tap = [](const tk_v4f u, const tk_v4f l, const TkCorner& c) {
      cf g = mk(u.x * c.w00, u.y * c.w00);
      g.x += u.z * c.w01;
      g.y += u.w * c.w01;
      g.x += l.x * c.w10;
      g.y += l.y * c.w10;
      g.x += l.z * c.w11;
      g.y += l.w * c.w11;
      return g;
    };
    auto sums = [](float* acc, float& e_acc, const cf g, const cf o, const cf x0, const cf p0,
                   const cf pn, const cf m0, const cf e1) {
      const cf dOP = g * pn;
      const cf dPO = m0 * o;
      const cf OP = o * p0;
      acc[0] += norm2(dOP);
      acc[1] += norm2(dPO);
      const cf a2 = dOP * conjf(dPO);
      acc[2] += a2.x;
      acc[3] += a2.y;
      acc[4] += dOP.x * x0.x + dOP.y * x0.y;
      acc[5] += dPO.x * x0.x + dPO.y * x0.y;
      acc[6] += OP.x * x0.x + OP.y * x0.y;
      acc[7] += norm2(OP);
      if (EIGEN) {
        const cf r = conjf(o) * x0 - m0;
        e_acc += r.x * e1.x + r.y * e1.y;
      }
    };
    auto pixel = [&](const int p, const tk_v4f u0, const tk_v4f l0, const tk_v4f u1,
                     const tk_v4f l1) {
      const cf oa = pat_a[p], ob = pat_b[p];
      const cf xa = chi_a[p], xb = chi_b[p];
      const cf p0 = probe.probe[p];
      const cf m0 = mpu[p];
      cf e1 = mk(0.f, 0.f);
      cf pa = p0 * s0, pb = p0 * s1;
      if (EIGEN) {
        e1 = probe.eigen[p];
        pa.x += t0 * e1.x;
        pa.y += t0 * e1.y;
        pb.x += t1 * e1.x;
        pb.y += t1 * e1.y;
      }
      sums(a, ea, tap(u0, l0, c0), oa, xa, p0, pa, m0, e1);
      sums(b, eb, tap(u1, l1, c1), ob, xb, p0, pb, m0, e1);
    };
    auto taps16 = [&](const unsigned off) {
      tk_v4f t;
      __builtin_memcpy(&t, reinterpret_cast<const char*>(gobj) + off, sizeof(t));
      return t;
    };
    // Row walk: a thread keeps its column and goes down the rows of its
    // share, so the lower taps of one pixel are the upper taps of the next --
    // one 16-byte load per pixel and position instead of two.  Windows of
    // 256 k columns: the column blocks one after the other; narrower windows
    // that divide 256: 256 / pw thread groups stacked over the rows.
    const int cols = pw < 256 ? pw : 256, groups = 256 / cols;
    const bool walk = (pw % 256 == 0 || 256 % pw == 0) && pw % (nsplit * groups) == 0;
    if (walk) {
      const int rows = pw / (nsplit * groups);
      const int ybeg = (part * groups + (int)threadIdx.x / cols) * rows;
      for (int x = (int)threadIdx.x % cols; x < pw; x += 256) {
        unsigned rel = (unsigned)(ybeg * W + x);
        tk_v4f u0 = taps16((base0 + rel) * 8u), u1 = taps16((base1 + rel) * 8u);
        int p = ybeg * pw + x;
#pragma unroll 2
        for (int y = 0; y < rows; ++y) {
          rel += (unsigned)W;
          const tk_v4f l0 = taps16((base0 + rel) * 8u), l1 = taps16((base1 + rel) * 8u);
          pixel(p, u0, l0, u1, l1);
          u0 = l0;
          u1 = l1;
          p += pw;
        }
      }
    } else {
      for (int p = pbeg; p < pend; p += blockDim.x) {
        const unsigned rel = (unsigned)(py * W + px);
        const unsigned off0 = (base0 + rel) * 8u, off1 = (base1 + rel) * 8u;
        pixel(p, taps16(off0), taps16(off0 + (unsigned)W * 8u), taps16(off1),
              taps16(off1 + (unsigned)W * 8u));
        py += qstep;
        px += rstep;
        if (px >= pw) {
          px -= pw;
          ++py;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float ta = tk_block_sum256(a[k], red);
      const float tb = tk_block_sum256(b[k], red);
      if (threadIdx.x == 0) {
        if (nsplit > 1) {
          unsafeAtomicAdd(&stats[(long)n0 * 8 + k], ta);
          unsafeAtomicAdd(&stats[(long)n0 * 8 + 8 + k], tb);
        } else {
          stats[(long)n0 * 8 + k] = ta;
          stats[(long)n0 * 8 + 8 + k] = tb;
        }
      }
    }
    if (EIGEN) {
      const float ta = tk_block_sum256(ea, red);
      const float tb = tk_block_sum256(eb, red);
      if (threadIdx.x == 0) {
        if (nsplit > 1) {
          unsafeAtomicAdd(&eigen_proj[n0], ta);
          unsafeAtomicAdd(&eigen_proj[n0 + 1], tb);
        } else {
          eigen_proj[n0] = ta;
          eigen_proj[n0 + 1] = tb;
        }
      }
    }
  }
}

extern "C" int tike_lstsq_step_stats(const void* chi, const float* scan, const void* psi,
                                     const void* object_update_precond, const void* probe,
                                     const void* eigen_probe, const float* eigen_weights,
                                     int num_eigen, int eigen_modes, const void* unique_probe,
                                     const void* m_probe_update, const void* patches,
                                     float* stats, int nscan, int S, int chi_modes, int pw, int H,
                                     int W, const void* eigen0, float* eigen_proj, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && chi_modes >= 1 && pw >= 1 && H >= 1 && W >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(chi && scan && psi && probe && stats);
  TK_CHECK_ARG(!eigen_proj || (eigen0 && m_probe_update));
  const TkProbe pr = tk_make_probe(probe, 0, eigen_probe, eigen_weights, num_eigen, eigen_modes,
                                   S, pw, unique_probe);
  // split the pixels of a position over several workgroups until the launch
  // holds ~8192 of them (probe windows that are a multiple of 1024 pixels)
  // two positions per work item where the common configurations allow it
  const bool no_eigen = (eigen_probe == nullptr || eigen_modes == 0) && eigen_proj == nullptr;
  const bool one_eigen = eigen_probe != nullptr && eigen_weights != nullptr && eigen_modes > 0 &&
                         num_eigen == 1 && eigen_proj != nullptr && eigen0 == eigen_probe;
  const bool pairs = g_stats_pairs && patches && object_update_precond && m_probe_update &&
                     unique_probe == nullptr && (no_eigen || one_eigen) &&
                     (long)H * W < (1L << 28) && nscan > 1;
  const long nitem = pairs ? (nscan + 1) / 2 : nscan;
  int nsplit = 1;
  while (nsplit < 16 && nitem * nsplit * 2 <= 8192 && ((long)pw * pw) % (2048L * nsplit) == 0)
    nsplit *= 2;
  if (tk_deterministic()) nsplit = 1;  // one workgroup per position: no atomics
  if (nsplit > 1) {
    hipError_t e = hipMemsetAsync(stats, 0, sizeof(float) * 8 * (size_t)nscan, (hipStream_t)stream);
    if (e == hipSuccess && eigen_proj)
      e = hipMemsetAsync(eigen_proj, 0, sizeof(float) * (size_t)nscan, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
#define TK_SS(HP, HG)                                                                         \
  hipLaunchKernelGGL((step_stats_kernel<HP, HG>), dim3(tk_grid((long)nscan * nsplit, 16)),    \
                     dim3(256), 0,                                                            \
                     (hipStream_t)stream, (const cf*)chi, scan, (const cf*)psi,               \
                     (const cf*)object_update_precond, pr, (const cf*)m_probe_update,         \
                     (const cf*)patches, stats, nscan, chi_modes, pw, H, W, (const cf*)eigen0, \
                     eigen_proj, nsplit)
#define TK_SP(EIG)                                                                            \
  hipLaunchKernelGGL((step_stats_pair_kernel<EIG>), dim3(tk_grid(nitem * nsplit, 16)),        \
                     dim3(256), 0,                                                            \
                     (hipStream_t)stream, (const cf*)chi, scan, (const cf*)psi,               \
                     (const cf*)object_update_precond, pr, (const cf*)m_probe_update,         \
                     (const cf*)patches, stats, nscan, chi_modes, pw, H, W, (const cf*)eigen0, \
                     eigen_proj, nsplit)
  if (pairs && one_eigen) TK_SP(true);
  else if (pairs) TK_SP(false);
  else if (patches && object_update_precond) TK_SS(true, true);
  else if (patches) TK_SS(true, false);
  else if (object_update_precond) TK_SS(false, true);
  else TK_SS(false, false);
#undef TK_SS
#undef TK_SP
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ------------------------------------------------------- eigen-probe update
// Residual probe update of position n for eigen probe index c (mode 0):
//   R_n = conj(O_n) chi_n,0 - mpu_0 - sum_{c' < c} coef[n][c'] E_c'
// (lstsq.py:740-761 _get_residuals/_update_residuals; probe.py:362-476).
// O_n = patches[n], chi_n,0 = chi0[n]; eigen (C, Sm, pw, pw) holds the CURRENT
// eigen probes (mode 0 slice used), coefs (nscan, C) complex the projections
// already removed.  Never materialised: every pass recomputes it.
struct TkResidual {
  const cf* patches;
  const cf* chi0;
  const cf* mpu0;
  const cf* eigen;
  const cf* coefs;
  int C, Sm, c;
  long P;
  long XS;  // elements between chi0 of consecutive positions (chi_modes * P)
  // C0: the residual of the FIRST eigen probe (c == 0) has no projections to
  // remove -- without that run-time loop in the body the callers' loops unroll
  // and the loads of several pixels / positions are in flight together
  template <bool C0>
  __device__ __forceinline__ cf at(long n, long p) const {
    cf r = conjf(patches[n * P + p]) * chi0[n * XS + p] - mpu0[p];
    if (!C0)
      for (int k = 0; k < c; ++k) r = r - coefs[n * C + k] * eigen[((long)k * Sm) * P + p];
    return r;
  }
};

// sums[n] = { sum Re(conj(R) E_c), sum Re(chi0 conj(O E_c)), sum |O E_c|^2,
//             Re sum R conj(E_c), Im sum R conj(E_c) }
template <bool C0>
__global__ __launch_bounds__(256) void eigen_position_sums_kernel(const TkResidual R,
                                                                  float* __restrict__ sums,
                                                                  int nscan) {
  __shared__ float red[4];
  const cf* __restrict__ E = R.eigen + ((long)R.c * R.Sm) * R.P;
  for (int n = blockIdx.x; n < nscan; n += gridDim.x) {
    float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (long p = threadIdx.x; p < R.P; p += blockDim.x) {  // (unrolled by 4: 0.217 -> 0.234 ms)
      const cf e = E[p];
      const cf r = R.at<C0>(n, p);
      const cf phi = R.patches[n * R.P + p] * e;
      const cf x = R.chi0[n * R.XS + p];
      a[0] += r.x * e.x + r.y * e.y;
      a[1] += x.x * phi.x + x.y * phi.y;
      a[2] += norm2(phi);
      const cf re = r * conjf(e);
      a[3] += re.x;
      a[4] += re.y;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float v = tk_block_sum256(a[k], red);
      if (threadIdx.x == 0) sums[(long)n * 5 + k] = v;
    }
  }
}

// update[p] += sum_n R_n[p] * pm[n]      (probe.py:432-436 before the mean)
template <bool C0>
__global__ __launch_bounds__(256) void eigen_pixel_update_kernel(const TkResidual R,
                                                                 const float* __restrict__ pm,
                                                                 float* __restrict__ update,
                                                                 int nscan, int chunk,
                                                                 float* __restrict__ part) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= R.P) return;
  const int b0 = blockIdx.y * chunk;
  const int b1 = min(nscan, b0 + chunk);
  cf acc = mk(0.f, 0.f);
#pragma unroll 4
  for (int n = b0; n < b1; ++n) {
    const cf r = R.at<C0>(n, p);
    const float w = pm[n];
    acc.x += r.x * w;
    acc.y += r.y * w;
  }
  if (part != nullptr) {  // deterministic mode: see probe_grad_kernel
    part[2 * ((long)blockIdx.y * R.P + p)] = acc.x;
    part[2 * ((long)blockIdx.y * R.P + p) + 1] = acc.y;
    return;
  }
  unsafeAtomicAdd(&update[2 * p], acc.x);
  unsafeAtomicAdd(&update[2 * p + 1], acc.y);
}

// O_n = patch_n(psi) at one pixel of an INTERIOR position, recomputed from the
// object (L2-resident: neighbouring positions share most of their footprint)
// exactly as forward pass 1 formed the stored patch -- same taps, same order
// of operations -- instead of streaming the stored patch from HBM.
// off: byte offset of the pixel's upper-left tap inside psi.
__device__ __forceinline__ cf tk_patch_pixel(const cf* __restrict__ psi, unsigned off,
                                             unsigned row_bytes, const TkCorner& c) {
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  tk_v4f u, l;
  __builtin_memcpy(&u, reinterpret_cast<const char*>(psi) + off, sizeof(u));
  __builtin_memcpy(&l, reinterpret_cast<const char*>(psi) + off + row_bytes, sizeof(l));
  cf o = mk(u.x * c.w00, u.y * c.w00);
  o.x += u.z * c.w01;
  o.y += u.w * c.w01;
  o.x += l.x * c.w10;
  o.y += l.y * c.w10;
  o.x += l.z * c.w11;
  o.y += l.w * c.w11;
  return o;
}
__device__ __forceinline__ bool tk_interior(const TkCorner& c, int pw, int H, int W) {
  return c.sy >= 0 && c.sx >= 0 && c.sy + pw < H && c.sx + pw < W && (long)H * W < (1L << 28);
}

// part[b] = sum over pixels p = 256 b + t (mod 256 TK_C0_PARTS) of Re(mpu_0 conj(E_0)):
// the position-independent term of the eigen projections (plain stores, added
// up in a fixed order by their reader)
constexpr int TK_C0_PARTS = 64;
__global__ __launch_bounds__(256) void eigen_proj_offset_kernel(const cf* __restrict__ mpu0,
                                                                const cf* __restrict__ E,
                                                                long P,
                                                                float* __restrict__ part) {
  __shared__ float red[4];
  float a = 0.f;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < P; p += 256L * TK_C0_PARTS) {
    const cf m = mpu0[p], e = E[p];
    a += m.x * e.x + m.y * e.y;
  }
  a = tk_block_sum256(a, red);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// The packed tail (one eigen probe per mode, c = 0): the per-position factor
// pm[n] = (eproj[n] / P + w[n]) / norm (probe.py:429-433) is formed on the fly
// from the projection the step statistics left and the batch norm.
// The one workgroup past the pixel blocks (blockIdx.x == gridDim.x - 1,
// blockIdx.y == 0) forms sums3 = { sum(A1 + eps), sum(A4 + eps), sum(costs) }
// of the step-statistics table (tike_lstsq_step_sums) -- the two go into one
// all-reduce.
__global__ __launch_bounds__(256) void eigen_pixel_update1_kernel(
    const TkResidual R, const float* __restrict__ eproj, const float* __restrict__ weights_c,
    long row, const float* __restrict__ norm, float inv_P, float* __restrict__ update, int nscan,
    int chunk, const float* __restrict__ stats, const float* __restrict__ costs, float eps,
    float* __restrict__ sums3, const cf* __restrict__ psi, const float* __restrict__ scan, int pw,
    int H, int W, float* __restrict__ part, const float* __restrict__ c0part,
    float* __restrict__ eproj_out) {
  // c0part (tike_eigen_pixel_update1q): eproj holds q_n, the projection is
  // q_n - c0 with c0 = sum_p Re(mpu_0 conj(E_0)) the sum of the 64 partials
  float c0 = 0.f;
  if (c0part != nullptr) {
    for (int b = 0; b < TK_C0_PARTS; ++b) c0 += c0part[b];
  }
  if (blockIdx.x + 1 == gridDim.x) {
    if (blockIdx.y != 0) return;
    if (eproj_out != nullptr) {
      for (int n = threadIdx.x; n < nscan; n += 256) eproj_out[n] = eproj[n] - c0;
    }
    if (sums3 == nullptr) return;
    __shared__ float red[4];
    float a1 = 0.f, a4 = 0.f, c = 0.f;
    for (int n = threadIdx.x; n < nscan; n += 256) {
      a1 += stats[8 * n] + eps;
      a4 += stats[8 * n + 1] + eps;
      c += costs[n];
    }
    a1 = tk_block_sum256(a1, red);
    a4 = tk_block_sum256(a4, red);
    c = tk_block_sum256(c, red);
    if (threadIdx.x == 0) {
      sums3[0] = a1;
      sums3[1] = a4;
      sums3[2] = c;
    }
    return;
  }
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= R.P) return;
  const int b0 = blockIdx.y * chunk;
  const int b1 = min(nscan, b0 + chunk);
  const float inv_norm = 1.0f / norm[0];
  cf acc = mk(0.f, 0.f);
  // O_n recomputed from the object when every position of the chunk is
  // interior (decided once: no load sits behind a per-position branch)
  bool gather = psi != nullptr;
  if (gather) {
    for (int n = b0; n < b1; ++n) gather = gather && tk_interior(tk_corner(scan, n), pw, H, W);
  }
  if (gather) {
    const int py = (int)(p / pw), px = (int)(p % pw);
    const unsigned row_bytes = (unsigned)W * (unsigned)sizeof(cf);
    const unsigned lane_off = (unsigned)py * row_bytes + (unsigned)px * (unsigned)sizeof(cf);
    const cf m0 = R.mpu0[p];
#pragma unroll 4
    for (int n = b0; n < b1; ++n) {
      const TkCorner c = tk_corner(scan, n);  // uniform
      const cf x = R.chi0[n * R.XS + p];
      const cf o = tk_patch_pixel(
          psi, (unsigned)(c.sy * W + c.sx) * (unsigned)sizeof(cf) + lane_off, row_bytes, c);
      const cf r = conjf(o) * x - m0;
      const float w = ((eproj[n] - c0) * inv_P + weights_c[n * row]) * inv_norm;
      acc.x += r.x * w;
      acc.y += r.y * w;
    }
  } else {
#pragma unroll 4
    for (int n = b0; n < b1; ++n) {
      const cf r = R.at<true>(n, p);
      const float w = ((eproj[n] - c0) * inv_P + weights_c[n * row]) * inv_norm;
      acc.x += r.x * w;
      acc.y += r.y * w;
    }
  }
  if (part != nullptr) {  // deterministic mode: see probe_grad_kernel
    part[2 * ((long)blockIdx.y * R.P + p)] = acc.x;
    part[2 * ((long)blockIdx.y * R.P + p) + 1] = acc.y;
    return;
  }
  unsafeAtomicAdd(&update[2 * p], acc.x);
  unsafeAtomicAdd(&update[2 * p + 1], acc.y);
}

// out[0] += scale * sum_n table[n * stride + col]: one workgroup, thread t takes
// rows t, t + 256, ..., then the fixed tree of tk_block_sum256
__global__ __launch_bounds__(256) void column_sum_ordered_kernel(const float* __restrict__ table,
                                                                 int stride, int col, int n,
                                                                 float scale,
                                                                 float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += table[(long)i * stride + col] * scale;
  a = tk_block_sum256(a, red);
  if (threadIdx.x == 0) out[0] += a;
}

// Position sums against the (already updated) first eigen probe, plus
// dsum[0] += sum_n sums[n][2] / P (the denominator mean, probe.py:463-469).
__global__ __launch_bounds__(256) void eigen_position_sums1_kernel(
    const TkResidual R, float* __restrict__ sums, float* __restrict__ dsum, int nscan,
    const cf* __restrict__ psi, const float* __restrict__ scan, int pw, int H, int W) {
  __shared__ float red[4];
  const cf* __restrict__ E = R.eigen;
  const unsigned row_bytes = (unsigned)W * (unsigned)sizeof(cf);
  const int qstep = (int)blockDim.x / pw, rstep = (int)blockDim.x % pw;
  for (int n = blockIdx.x; n < nscan; n += gridDim.x) {
    float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    TkCorner c = {0, 0, 0.f, 0.f, 0.f, 0.f};
    if (psi != nullptr) c = tk_corner(scan, n);  // uniform
    const bool gather = psi != nullptr && tk_interior(c, pw, H, W);
    const unsigned off0 = gather ? (unsigned)(c.sy * W + c.sx) * (unsigned)sizeof(cf) : 0u;
    // (the choice is settled outside the pixel loop: a load behind a run-time
    // condition would wait for the loads in front of the branch)
    auto body = [&](auto g_tag) {
      constexpr bool G = decltype(g_tag)::value;
      int py = (int)threadIdx.x / pw, px = (int)threadIdx.x % pw;
      for (long p = threadIdx.x; p < R.P; p += blockDim.x) {
        const cf e = E[p];
        const cf x = R.chi0[n * R.XS + p];
        const cf m0 = R.mpu0[p];
        cf o;
        if constexpr (G)
          o = tk_patch_pixel(psi, off0 + (unsigned)py * row_bytes + (unsigned)px * 8u, row_bytes, c);
        else
          o = R.patches[n * R.P + p];
        const cf r = conjf(o) * x - m0;
        const cf phi = o * e;
        py += qstep;
        px += rstep;
        if (px >= pw) {
          px -= pw;
          ++py;
        }
        a[0] += r.x * e.x + r.y * e.y;
        a[1] += x.x * phi.x + x.y * phi.y;
        a[2] += norm2(phi);
        const cf re = r * conjf(e);
        a[3] += re.x;
        a[4] += re.y;
      }
    };
    if (gather)
      body(std::true_type{});
    else
      body(std::false_type{});
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float v = tk_block_sum256(a[k], red);
      if (threadIdx.x == 0) {
        sums[(long)n * 5 + k] = v;
        if (k == 2 && dsum != nullptr) unsafeAtomicAdd(dsum, v / (float)R.P);
      }
    }
  }
}

// Two positions per workgroup of 512 threads, row walk (see
// step_stats_pair_kernel): E_0 and the probe update are loaded once for both
// positions and every pixel costs one 16-byte tap load per position -- 6 loads
// per pixel pair instead of 10.  cols = min(pw, 256) columns per thread group,
// 512 / cols groups stacked over the rows; a pair with a position on the
// border (or the odd last position) takes the strided per-position loop.
__global__ __launch_bounds__(512) void eigen_position_sums1_pair_kernel(
    const TkResidual R, float* __restrict__ sums, float* __restrict__ dsum, int nscan,
    const cf* __restrict__ psi, const float* __restrict__ scan, int pw, int H, int W) {
  __shared__ float red[8];
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const cf* __restrict__ E = R.eigen;
  const unsigned row_bytes = (unsigned)W * (unsigned)sizeof(cf);
  const int cols = pw < 256 ? pw : 256, rows = pw / (512 / cols);
  const int npair = (nscan + 1) / 2;
  auto add = [](float* a, const cf o, const cf x, const cf e, const cf m0) {
    const cf r = conjf(o) * x - m0;
    const cf phi = o * e;
    a[0] += r.x * e.x + r.y * e.y;
    a[1] += x.x * phi.x + x.y * phi.y;
    a[2] += norm2(phi);
    const cf re = r * conjf(e);
    a[3] += re.x;
    a[4] += re.y;
  };
  auto finish = [&](const float* a, const int n) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float v = tk_block_sum512(a[k], red);
      if (threadIdx.x == 0) {
        sums[(long)n * 5 + k] = v;
        if (k == 2 && dsum != nullptr) unsafeAtomicAdd(dsum, v / (float)R.P);
      }
    }
  };
  auto one = [&](const int n, const TkCorner& c, const bool gather) {
    float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned off0 = gather ? (unsigned)(c.sy * W + c.sx) * 8u : 0u;
    for (long p = threadIdx.x; p < R.P; p += blockDim.x) {
      const cf o = gather ? tk_patch_pixel(psi, off0 + (unsigned)(p / pw) * row_bytes +
                                                    (unsigned)(p % pw) * 8u, row_bytes, c)
                          : R.patches[n * R.P + p];
      add(a, o, R.chi0[n * R.XS + p], E[p], R.mpu0[p]);
    }
    finish(a, n);
  };
  auto taps16 = [&](const unsigned off) {
    tk_v4f t;
    __builtin_memcpy(&t, reinterpret_cast<const char*>(psi) + off, sizeof(t));
    return t;
  };
  auto tap = [](const tk_v4f u, const tk_v4f l, const TkCorner& c) {
    cf o = mk(u.x * c.w00, u.y * c.w00);  // the order of tk_patch_pixel
    o.x += u.z * c.w01;
    o.y += u.w * c.w01;
    o.x += l.x * c.w10;
    o.y += l.y * c.w10;
    o.x += l.z * c.w11;
    o.y += l.w * c.w11;
    return o;
  };
  for (int pair = blockIdx.x; pair < npair; pair += gridDim.x) {
    const int n0 = 2 * pair;
    const bool two = n0 + 1 < nscan;
    const TkCorner c0 = tk_corner(scan, n0);
    const TkCorner c1 = tk_corner(scan, two ? n0 + 1 : n0);
    const bool in0 = tk_interior(c0, pw, H, W), in1 = tk_interior(c1, pw, H, W);
    if (!(two && in0 && in1)) {  // uniform
      one(n0, c0, in0);
      if (two) one(n0 + 1, c1, in1);
      continue;
    }
    float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, b[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const unsigned base0 = (unsigned)(c0.sy * W + c0.sx), base1 = (unsigned)(c1.sy * W + c1.sx);
    const cf* __restrict__ chi_a = R.chi0 + (long)n0 * R.XS;
    const cf* __restrict__ chi_b = chi_a + R.XS;
    const int ybeg = ((int)threadIdx.x / cols) * rows;
    for (int x = (int)threadIdx.x % cols; x < pw; x += 256) {
      unsigned rel = (unsigned)(ybeg * W + x);
      tk_v4f u0 = taps16((base0 + rel) * 8u), u1 = taps16((base1 + rel) * 8u);
      int p = ybeg * pw + x;
#pragma unroll 2
      for (int y = 0; y < rows; ++y) {
        rel += (unsigned)W;
        const tk_v4f l0 = taps16((base0 + rel) * 8u), l1 = taps16((base1 + rel) * 8u);
        const cf e = E[p], m0 = R.mpu0[p];
        const cf xa = chi_a[p], xb = chi_b[p];
        add(a, tap(u0, l0, c0), xa, e, m0);
        add(b, tap(u1, l1, c1), xb, e, m0);
        u0 = l0;
        u1 = l1;
        p += pw;
      }
    }
    finish(a, n0);
    finish(b, n0 + 1);
  }
}

// The step statistics (step_stats_pair_kernel<true>, without the eigen
// projection) and the eigen position sums (eigen_position_sums1) in ONE pass
// over chi_n,0 and the patches.  The sums are taken against the renormalised
// first eigen probe E' = (E + k update) / |.| (the arithmetic of
// eigen_apply1_kernel, from nacc), formed on the fly: E itself stays the probe
// the step statistics' varying probe is made of until the launch after this one
// writes E'.  Two positions per work item, row walk; a pair with a position on
// the border takes step_stats_item and a per-position strided loop.
// sums5[n] = { s0, s1, s2, s0, s4 }: Re sum R conj(E') is s0 and s3 alike.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
void step_stats_eigen_pair_kernel(
    const cf* __restrict__ chi, const float* __restrict__ scan, const cf* __restrict__ gobj,
    const TkProbe probe, const cf* __restrict__ mpu, const cf* __restrict__ patches,
    const cf* __restrict__ update, const float* __restrict__ nacc, float inv_count, float beta,
    float* __restrict__ stats, float* __restrict__ sums5, int nscan, int chi_modes, int pw,
    int H, int W, int nsplit) {
  __shared__ float red[4];
  typedef float tk_v4f __attribute__((ext_vector_type(4)));
  const long P = (long)pw * pw;
  const int plen = (int)(P / nsplit);
  const int npair = (nscan + 1) / 2;
  // E' = (E + k u) inv (eigen_apply1_kernel)
  const float uu = nacc[0], ee = nacc[1], eu = nacc[2];
  const float mu = sqrtf(uu * inv_count * inv_count / (float)P);
  const float kk = beta / mu * inv_count;
  const float inv = 1.0f / sqrtf((ee + 2.0f * kk * eu + kk * kk * uu) / (float)P);
  auto enew = [&](const cf e, const long p) { return (e + update[p] * kk) * inv; };
  auto esum = [](float* a, const cf o, const cf x, const cf e, const cf m0) {
    const cf r = conjf(o) * x - m0;
    const cf phi = o * e;
    a[0] += r.x * e.x + r.y * e.y;
    a[1] += x.x * phi.x + x.y * phi.y;
    a[2] += norm2(phi);
    a[3] += r.y * e.x - r.x * e.y;  // Im(r conj(e))
  };
  auto put = [&](float* dst, const float v) {
    if (nsplit > 1)
      unsafeAtomicAdd(dst, v);
    else
      *dst = v;
  };
  auto finish5 = [&](const float* a, const int n) {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = tk_block_sum256(a[k], red);
    if (threadIdx.x == 0) {
      float* o = sums5 + (long)n * 5;
      put(o, t[0]);
      put(o + 1, t[1]);
      put(o + 2, t[2]);
      put(o + 3, t[0]);
      put(o + 4, t[3]);
    }
  };
  for (int v = blockIdx.x; v < npair * nsplit; v += gridDim.x) {
    const int n0 = 2 * (v / nsplit), part = v % nsplit;
    const TkCorner c0 = tk_corner(scan, n0);
    const bool two = n0 + 1 < nscan;
    const TkCorner c1 = tk_corner(scan, two ? n0 + 1 : n0);
    const bool in0 = c0.sy >= 0 && c0.sx >= 0 && c0.sy + pw < H && c0.sx + pw < W;
    const bool in1 = c1.sy >= 0 && c1.sx >= 0 && c1.sy + pw < H && c1.sx + pw < W;
    const int pbeg = part * plen + (int)threadIdx.x;
    const int pend = part + 1 == nsplit ? (int)P : (part + 1) * plen;
    if (!(two && in0 && in1)) {  // uniform
      for (int i = 0; i < (two ? 2 : 1); ++i) {
        const int n = n0 + i;
        step_stats_item<true, true>(chi, scan, nullptr, gobj, probe, mpu, patches, stats,
                                    chi_modes, pw, H, W, nullptr, nullptr, nsplit, n, part, red);
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = pbeg; p < pend; p += blockDim.x)
          esum(a, patches[(long)n * P + p], chi[(long)n * chi_modes * P + p],
               enew(probe.eigen[p], p), mpu[p]);
        finish5(a, n);
      }
      continue;
    }
    float s0 = 1.0f, s1 = 1.0f, t0 = 0.f, t1 = 0.f;  // weights of P_0 and of E_0
    if (probe.weights != nullptr) {
      const float* w = probe.weights + n0 * (long)(probe.C + 1) * probe.S;
      s0 = w[0];
      s1 = w[(long)(probe.C + 1) * probe.S];
      t0 = w[probe.S];
      t1 = w[(long)(probe.C + 1) * probe.S + probe.S];
    }
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float ea[4] = {0.f, 0.f, 0.f, 0.f}, eb[4] = {0.f, 0.f, 0.f, 0.f};
    const unsigned base0 = (unsigned)(c0.sy * W + c0.sx), base1 = (unsigned)(c1.sy * W + c1.sx);
    const cf* __restrict__ chi_a = chi + ((long)n0 * chi_modes) * P;
    const cf* __restrict__ chi_b = chi + ((long)(n0 + 1) * chi_modes) * P;
    const cf* __restrict__ pat_a = patches + (long)n0 * P;
    const cf* __restrict__ pat_b = pat_a + P;
    auto tap = [](const tk_v4f u, const tk_v4f l, const TkCorner& c) {
      cf g = mk(u.x * c.w00, u.y * c.w00);
      g.x += u.z * c.w01;
      g.y += u.w * c.w01;
      g.x += l.x * c.w10;
      g.y += l.y * c.w10;
      g.x += l.z * c.w11;
      g.y += l.w * c.w11;
      return g;
    };
    auto sums = [](float* acc, const cf g, const cf o, const cf x0, const cf p0, const cf pn,
                   const cf m0) {
      const cf dOP = g * pn;
      const cf dPO = m0 * o;
      const cf OP = o * p0;
      acc[0] += norm2(dOP);
      acc[1] += norm2(dPO);
      const cf a2 = dOP * conjf(dPO);
      acc[2] += a2.x;
      acc[3] += a2.y;
      acc[4] += dOP.x * x0.x + dOP.y * x0.y;
      acc[5] += dPO.x * x0.x + dPO.y * x0.y;
      acc[6] += OP.x * x0.x + OP.y * x0.y;
      acc[7] += norm2(OP);
    };
    auto pixel = [&](const int p, const tk_v4f u0, const tk_v4f l0, const tk_v4f u1,
                     const tk_v4f l1) {
      const cf oa = pat_a[p], ob = pat_b[p];
      const cf xa = chi_a[p], xb = chi_b[p];
      const cf p0 = probe.probe[p];
      const cf m0 = mpu[p];
      const cf e1 = probe.eigen[p];
      const cf en = enew(e1, p);
      cf pa = p0 * s0, pb = p0 * s1;
      pa.x += t0 * e1.x;
      pa.y += t0 * e1.y;
      pb.x += t1 * e1.x;
      pb.y += t1 * e1.y;
      sums(a, tap(u0, l0, c0), oa, xa, p0, pa, m0);
      sums(b, tap(u1, l1, c1), ob, xb, p0, pb, m0);
      esum(ea, oa, xa, en, m0);
      esum(eb, ob, xb, en, m0);
    };
    auto taps16 = [&](const unsigned off) {
      tk_v4f t;
      __builtin_memcpy(&t, reinterpret_cast<const char*>(gobj) + off, sizeof(t));
      return t;
    };
    // row walk of step_stats_pair_kernel (the launcher admits only windows
    // that allow it)
    const int cols = pw < 256 ? pw : 256, groups = 256 / cols;
    const int rows = pw / (nsplit * groups);
    const int ybeg = (part * groups + (int)threadIdx.x / cols) * rows;
    for (int x = (int)threadIdx.x % cols; x < pw; x += 256) {
      unsigned rel = (unsigned)(ybeg * W + x);
      tk_v4f u0 = taps16((base0 + rel) * 8u), u1 = taps16((base1 + rel) * 8u);
      int p = ybeg * pw + x;
#pragma unroll 2
      for (int y = 0; y < rows; ++y) {
        rel += (unsigned)W;
        const tk_v4f l0 = taps16((base0 + rel) * 8u), l1 = taps16((base1 + rel) * 8u);
        pixel(p, u0, l0, u1, l1);
        u0 = l0;
        u1 = l1;
        p += pw;
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float ta = tk_block_sum256(a[k], red);
      const float tb = tk_block_sum256(b[k], red);
      if (threadIdx.x == 0) {
        put(&stats[(long)n0 * 8 + k], ta);
        put(&stats[(long)n0 * 8 + 8 + k], tb);
      }
    }
    finish5(ea, n0);
    finish5(eb, n0 + 1);
  }
}

// Workgroups [0, gridDim.x - 1): nacc[0..2] += { sum |update|^2, sum |E|^2,
// sum Re(conj(E) update) } (lstsq_tail_mid_kernel's summing workgroups).
__global__ __launch_bounds__(256) void eigen_norm_sums1_kernel(const cf* __restrict__ E,
                                                               const cf* __restrict__ update,
                                                               int npix, float* __restrict__ nacc,
                                                               float* __restrict__ part) {
  __shared__ float red[4];
  float uu = 0.f, ee = 0.f, eu = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const cf e = E[i], u = update[i];
    uu += norm2(u);
    ee += norm2(e);
    eu += e.x * u.x + e.y * u.y;
  }
  uu = tk_block_sum256(uu, red);
  ee = tk_block_sum256(ee, red);
  eu = tk_block_sum256(eu, red);
  if (threadIdx.x == 0) {
    if (part != nullptr) {  // deterministic mode: added in workgroup order afterwards
      part[3 * blockIdx.x] = uu;
      part[3 * blockIdx.x + 1] = ee;
      part[3 * blockIdx.x + 2] = eu;
    } else {
      unsafeAtomicAdd(&nacc[0], uu);
      unsafeAtomicAdd(&nacc[1], ee);
      unsafeAtomicAdd(&nacc[2], eu);
    }
  }
}

extern "C" int tike_lstsq_step_stats_eigen1(const void* chi, const float* scan,
                                            const void* object_update_precond, const void* probe,
                                            const void* eigen_probe, const float* eigen_weights,
                                            int eigen_modes, const void* m_probe_update,
                                            const void* patches, const void* update, float* nacc,
                                            double count, float beta_eigen, float* stats,
                                            float* sums5, int nscan, int S, int chi_modes,
                                            int pw, int H, int W, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && chi_modes >= 1 && pw >= 1 && H >= 1 && W >= 1 &&
               eigen_modes >= 1 && count > 0);
  TK_CHECK_ARG(probe && eigen_probe && eigen_weights && m_probe_update && update && nacc);
  const long P = (long)pw * pw;
  const long nitem = (nscan + 1) / 2;
  int nsplit = 1;
  while (nsplit < 16 && nitem * nsplit * 2 <= 8192 && P % (2048L * nsplit) == 0) nsplit *= 2;
  if (tk_deterministic()) nsplit = 1;  // one workgroup per position pair: no atomics
  // the row walk of the pair kernel: windows of 256 k columns or dividing 256
  const int groups = 256 / (pw < 256 ? pw : 256);
  if (!((pw % 256 == 0 || 256 % pw == 0) && pw % (nsplit * groups) == 0 &&
        (long)H * W < (1L << 28)))
    return TK_ERR_UNSUPPORTED;
  // nacc (zero on entry) from E and the all-ranks update
  int grid = P >= 256 * 64 ? 64 : (int)((P + 255) / 256);
  float* part = nullptr;
  if (tk_deterministic()) {
    part = tk_det_scratch(sizeof(float) * 3 * (size_t)grid);
    if (part == nullptr) grid = 1;
  }
  hipLaunchKernelGGL(eigen_norm_sums1_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     (const cf*)eigen_probe, (const cf*)update, (int)P, nacc, part);
  TK_LAUNCH_CHECK();
  if (part != nullptr) {
    int rc = tk_ordered_sum(nacc, part, 3, grid, true, (hipStream_t)stream);
    if (rc) return rc;
  }
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(chi && scan && object_update_precond && patches && stats && sums5);
  const TkProbe pr = tk_make_probe(probe, 0, eigen_probe, eigen_weights, 1, eigen_modes, S, pw,
                                   nullptr);
  if (nsplit > 1) {
    hipError_t e = hipMemsetAsync(stats, 0, sizeof(float) * 8 * (size_t)nscan, (hipStream_t)stream);
    if (e == hipSuccess)
      e = hipMemsetAsync(sums5, 0, sizeof(float) * 5 * (size_t)nscan, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(step_stats_eigen_pair_kernel, dim3(tk_grid(nitem * nsplit, 16)), dim3(256),
                     0, (hipStream_t)stream, (const cf*)chi, scan,
                     (const cf*)object_update_precond, pr, (const cf*)m_probe_update,
                     (const cf*)patches, (const cf*)update, (const float*)nacc,
                     (float)(1.0 / count), beta_eigen, stats, sums5, nscan, chi_modes, pw, H, W,
                     nsplit);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

static TkResidual make_residual(const void* patches, const void* chi0, const void* mpu0,
                                const void* eigen, const void* coefs, int C, int Sm, int c,
                                int pw, int chi_modes) {
  TkResidual R;
  R.patches = (const cf*)patches;
  R.chi0 = (const cf*)chi0;
  R.mpu0 = (const cf*)mpu0;
  R.eigen = (const cf*)eigen;
  R.coefs = (const cf*)coefs;
  R.C = C;
  R.Sm = Sm;
  R.c = c;
  R.P = (long)pw * pw;
  R.XS = R.P * chi_modes;
  return R;
}

extern "C" int tike_eigen_position_sums(const void* patches, const void* chi0, const void* mpu0,
                                        const void* eigen_probe, const void* coefs,
                                        int num_eigen, int eigen_modes, int c, float* sums,
                                        int nscan, int pw, int chi_modes, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && num_eigen >= 1 && c >= 0 && c < num_eigen &&
               chi_modes >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(patches && chi0 && mpu0 && eigen_probe && sums && (c == 0 || coefs));
  const TkResidual R = make_residual(patches, chi0, mpu0, eigen_probe, coefs, num_eigen,
                                     eigen_modes, c, pw, chi_modes);
  if (c == 0)
    hipLaunchKernelGGL(eigen_position_sums_kernel<true>, dim3(tk_grid(nscan, 16)), dim3(256), 0,
                       (hipStream_t)stream, R, sums, nscan);
  else
    hipLaunchKernelGGL(eigen_position_sums_kernel<false>, dim3(tk_grid(nscan, 16)), dim3(256),
                       0, (hipStream_t)stream, R, sums, nscan);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

extern "C" int tike_eigen_pixel_update(const void* patches, const void* chi0, const void* mpu0,
                                       const void* eigen_probe, const void* coefs,
                                       int num_eigen, int eigen_modes, int c, const float* pm,
                                       void* update, int nscan, int pw, int chi_modes,
                                       void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && num_eigen >= 1 && c >= 0 && c < num_eigen &&
               chi_modes >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(patches && chi0 && mpu0 && eigen_probe && pm && update && (c == 0 || coefs));
  const long P = (long)pw * pw;
  float* part = nullptr;
  const int chunk = probe_chunk(nscan, 2 * P, &part);
  dim3 grid((unsigned)((P + 255) / 256), (unsigned)((nscan + chunk - 1) / chunk));
  const TkResidual R = make_residual(patches, chi0, mpu0, eigen_probe, coefs, num_eigen,
                                     eigen_modes, c, pw, chi_modes);
  if (c == 0)
    hipLaunchKernelGGL(eigen_pixel_update_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream,
                       R, pm, (float*)update, nscan, chunk, part);
  else
    hipLaunchKernelGGL(eigen_pixel_update_kernel<false>, grid, dim3(256), 0,
                       (hipStream_t)stream, R, pm, (float*)update, nscan, chunk, part);
  TK_LAUNCH_CHECK();
  if (part != nullptr)
    return tk_ordered_sum((float*)update, part, 2 * P, (int)grid.y, true, (hipStream_t)stream);
  return TK_OK;
}

extern "C" int tike_eigen_pixel_update1(const void* patches, const void* chi0,
                                        const void* mpu0, const void* eigen0,
                                        const float* eigen_proj, const float* weights_c,
                                        long weights_row, const float* norm, void* update,
                                        int nscan, int pw, int chi_modes, const float* stats,
                                        const float* costs, float eps, float* sums3,
                                        const void* psi, const float* scan, int H, int W,
                                        void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && chi_modes >= 1 && weights_row >= 1);
  // (an EMPTY share of a minibatch -- more ranks than positions -- comes with
  // null per-position arrays: nothing to check, the sums are zero)
  if (nscan == 0) {
    if (sums3) return (int)hipMemsetAsync(sums3, 0, 3 * sizeof(float), (hipStream_t)stream);
    return TK_OK;
  }
  TK_CHECK_ARG(!sums3 || (stats && costs));
  TK_CHECK_ARG(!psi || (scan && H >= 1 && W >= 1));
  TK_CHECK_ARG(patches && chi0 && mpu0 && eigen0 && eigen_proj && weights_c && norm && update);
  const long P = (long)pw * pw;
  float* part = nullptr;
  const int chunk = probe_chunk(nscan, 2 * P, &part);
  dim3 grid((unsigned)((P + 255) / 256) + 1, (unsigned)((nscan + chunk - 1) / chunk));
  const TkResidual R = make_residual(patches, chi0, mpu0, eigen0, nullptr, 1, 1, 0, pw, chi_modes);
  hipLaunchKernelGGL(eigen_pixel_update1_kernel, grid, dim3(256), 0, (hipStream_t)stream, R,
                     eigen_proj, weights_c, weights_row, norm, 1.0f / (float)P, (float*)update,
                     nscan, chunk, stats, costs, eps, sums3, (const cf*)psi, scan, pw, H, W,
                     part, nullptr, nullptr);
  TK_LAUNCH_CHECK();
  if (part != nullptr)
    return tk_ordered_sum((float*)update, part, 2 * P, (int)grid.y, true, (hipStream_t)stream);
  return TK_OK;
}

// tike_eigen_pixel_update1 from q (tike_ifft2_pass2_gradients_eproj) instead of
// the projections: eigen_proj[n] = q[n] - sum_p Re(mpu_0 conj(E_0)) formed on
// the fly (and left in eproj_out, when given); no sums3.  c0part: scratch of
// 64 floats.
extern "C" int tike_eigen_pixel_update1q(const void* patches, const void* chi0,
                                         const void* mpu0, const void* eigen0, const float* q,
                                         const float* weights_c, long weights_row,
                                         const float* norm, void* update, int nscan, int pw,
                                         int chi_modes, const void* psi, const float* scan,
                                         int H, int W, float* c0part, float* eproj_out,
                                         void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && chi_modes >= 1 && weights_row >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(!psi || (scan && H >= 1 && W >= 1));
  TK_CHECK_ARG(patches && chi0 && mpu0 && eigen0 && q && weights_c && norm && update && c0part);
  const long P = (long)pw * pw;
  hipLaunchKernelGGL(eigen_proj_offset_kernel, dim3(TK_C0_PARTS), dim3(256), 0,
                     (hipStream_t)stream, (const cf*)mpu0, (const cf*)eigen0, P, c0part);
  float* part = nullptr;
  const int chunk = probe_chunk(nscan, 2 * P, &part);
  dim3 grid((unsigned)((P + 255) / 256) + 1, (unsigned)((nscan + chunk - 1) / chunk));
  const TkResidual R = make_residual(patches, chi0, mpu0, eigen0, nullptr, 1, 1, 0, pw, chi_modes);
  hipLaunchKernelGGL(eigen_pixel_update1_kernel, grid, dim3(256), 0, (hipStream_t)stream, R, q,
                     weights_c, weights_row, norm, 1.0f / (float)P, (float*)update, nscan, chunk,
                     nullptr, nullptr, 0.f, nullptr, (const cf*)psi, scan, pw, H, W, part,
                     c0part, eproj_out);
  TK_LAUNCH_CHECK();
  if (part != nullptr)
    return tk_ordered_sum((float*)update, part, 2 * P, (int)grid.y, true, (hipStream_t)stream);
  return TK_OK;
}

extern "C" int tike_eigen_position_sums1(const void* patches, const void* chi0,
                                         const void* mpu0, const void* eigen0, float* sums,
                                         float* dsum, int nscan, int pw, int chi_modes,
                                         const void* psi, const float* scan, int H, int W,
                                         void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && pw >= 1 && chi_modes >= 1);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(!psi || (scan && H >= 1 && W >= 1));
  TK_CHECK_ARG(patches && chi0 && mpu0 && eigen0 && sums && dsum);
  const TkResidual R = make_residual(patches, chi0, mpu0, eigen0, nullptr, 1, 1, 0, pw, chi_modes);
  const bool det = tk_deterministic();
  const int cols = pw < 256 ? pw : 256;
  const bool pairs = g_stats_pairs && psi != nullptr && nscan > 1 &&
                     (pw % 256 == 0 || 256 % pw == 0) && pw % (512 / cols) == 0 &&
                     (long)H * W < (1L << 28);
  if (pairs)
    hipLaunchKernelGGL(eigen_position_sums1_pair_kernel, dim3(tk_grid((nscan + 1) / 2, 16)),
                       dim3(512), 0, (hipStream_t)stream, R, sums, det ? nullptr : dsum, nscan,
                       (const cf*)psi, scan, pw, H, W);
  else
    hipLaunchKernelGGL(eigen_position_sums1_kernel, dim3(tk_grid(nscan, 16)), dim3(256), 0,
                       (hipStream_t)stream, R, sums, det ? nullptr : dsum, nscan, (const cf*)psi,
                       scan, pw, H, W);
  if (det)  // dsum += sum_n sums[n][2] / P, one workgroup, a fixed order
    hipLaunchKernelGGL(column_sum_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums,
                       5, 2, nscan, 1.0f / (float)((long)pw * pw), dsum);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

// ------------------------------------------------------- varying probe
// out[n][s] = weights[n][0][s] * probe[s] + sum_c weights[n][c+1][s] * eigen[c][s]
// for the first Sm modes (probe.py:272-303 get_varying_probe); the modes
// without eigen probes only need the scalar weights[n][0][s].
__global__ __launch_bounds__(256) void varying_probe_kernel(const TkProbe probe,
                                                            cf* __restrict__ out, long total,
                                                            long PP) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long pix = i % PP;
    const long ns = i / PP;
    out[i] = probe.at(ns / probe.Sm, (int)(ns % probe.Sm), pix);
  }
}

extern "C" int tike_varying_probe(const void* probe, const void* eigen_probe,
                                  const float* eigen_weights, int num_eigen, int eigen_modes,
                                  void* out, int nscan, int S, int pw, void* stream) {
  TK_ENTER();
  TK_CHECK_ARG(nscan >= 0 && S >= 1 && pw >= 1 && eigen_modes >= 1 && eigen_modes <= S);
  if (nscan == 0) return TK_OK;
  TK_CHECK_ARG(probe && eigen_weights && out && (num_eigen == 0 || eigen_probe));
  const long PP = (long)pw * pw;
  const long total = (long)nscan * eigen_modes * PP;
  hipLaunchKernelGGL(varying_probe_kernel, dim3(tk_grid((total + 255) / 256, 16)), dim3(256), 0,
                     (hipStream_t)stream,
                     tk_make_probe(probe, 0, eigen_probe, eigen_weights, num_eigen, eigen_modes,
                                   S, pw),
                     (cf*)out, total, PP);
  TK_LAUNCH_CHECK();
  return TK_OK;
}

