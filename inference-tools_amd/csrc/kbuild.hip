// Covariance-matrix build for SquaredExponential / RationalQuadratic / Matern32 / Matern52 / Periodic on gfx950.
//
// Replaces the reference's N x N x d broadcast tensors (covariance.py:218-219, 254, 315-316, 347)
// by a tiled kernel: a workgroup stages the two 64-point panels in LDS (transposed, [dim][point]) and
// every thread produces a 4 x 4 block of K, written as 32-byte row segments (16 threads -> 512
// contiguous bytes per row).  HBM-write bound: 8 bytes per element, x is read once per tile from L2.
#include <cassert>

#include "gpmi_internal.h"
#include "pair_tile.h"

namespace {

using pair_tile::KT;  // output tile edge

// The tile (staging, the thread's 4 x 4 block, s, the covariance function in two halves): pair_tile.h, shared with
// sparse.hip.  kfun and its kinds KFUN_M32_G / KFUN_M52_G: kfun.h.

// SQUARE: U == V, jitter + noise on the diagonal, identity in the padding (rows/cols >= n).
template <bool SQUARE, int KERNEL>
__device__ inline void kbuild_body(const KParams& p, const double* __restrict__ U, int64_t nu,
                                   const double* __restrict__ V, int64_t nv,
                                   const double* __restrict__ noise, double* __restrict__ out,
                                   int64_t ld, int lower_only);

template <bool SQUARE, int KERNEL>
__global__ __launch_bounds__(256) void kbuild_kernel(KParams p, const double* __restrict__ U,
                                                     int64_t nu, const double* __restrict__ V,
                                                     int64_t nv, const double* __restrict__ noise,
                                                     double* __restrict__ out, int64_t ld,
                                                     int lower_only) {
  kbuild_body<SQUARE, KERNEL>(p, U, nu, V, nv, noise, out, ld, lower_only);
}

// batched square build: problem z uses hyper-parameters pdev[z] and writes matrix out + z * stride
template <int KERNEL>
__global__ __launch_bounds__(256) void kbuild_batched_kernel(const KParams* __restrict__ pdev,
                                                             const double* __restrict__ x, int64_t n,
                                                             const double* __restrict__ noise,
                                                             double* __restrict__ out, int64_t ld,
                                                             int64_t stride, int64_t noise_stride) {
  // noise_stride > 0: every problem has noise variances of its own (HeteroscedasticNoise: they are hyper-parameters)
  kbuild_body<true, KERNEL>(pdev[blockIdx.z], x, n, x, n, noise + (int64_t)blockIdx.z * noise_stride,
                            out + (int64_t)blockIdx.z * stride, ld, 2);
}

// batched cross build: problem z builds its own K*_z (the rows of U against the rows of V) from pdev[z] into
// out + z * stride; tile (blockIdx.y, blockIdx.x) as in the single cross build, so an element has the value
// launch_kbuild_cross gives for those parameters
template <int KERNEL>
__global__ __launch_bounds__(256) void kbuild_cross_batched_kernel(const KParams* __restrict__ pdev,
                                                                   const double* __restrict__ U, int64_t nu,
                                                                   const double* __restrict__ V, int64_t nv,
                                                                   double* __restrict__ out, int64_t ld, int64_t stride) {
  kbuild_body<false, KERNEL>(pdev[blockIdx.z], U, nu, V, nv, nullptr, out + (int64_t)blockIdx.z * stride, ld, 0);
}

template <bool SQUARE, int KERNEL>
__device__ inline void kbuild_body(const KParams& p, const double* __restrict__ U, int64_t nu,
                                   const double* __restrict__ V, int64_t nv,
                                   const double* __restrict__ noise, double* __restrict__ out,
                                   int64_t ld, int lower_only) {
  int ti = blockIdx.y, tj = blockIdx.x;
  const int tile_off = lower_only >> 8;  // mode 2: the triangle starts at tile (tile_off, tile_off)
  lower_only &= 0xff;
  if (SQUARE && lower_only == 2) {
    // one-dimensional grid over the lower tiles only (row by row): id = ti (ti + 1) / 2 + tj.  (Half of a square
    // grid's 61 504 workgroups at N = 16384 did nothing but start and exit: 0.48 -> 0.45 ms per build; the rest is the f64 exp, VALU-bound.)
    const int id = blockIdx.x;
    ti = (int)((sqrt(8.0 * id + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
    while (ti * (ti + 1) / 2 > id) --ti;
    tj = id - ti * (ti + 1) / 2 + tile_off;
    ti += tile_off;
  } else if (SQUARE && lower_only && tj > ti) {
    return;
  }
  // the two point panels, [dim][point]: 2 x d x 64 doubles of dynamic LDS (a static 2 x GPMI_MAX_D x 64 = 64 KiB held
  // the kernel at two workgroups per CU whatever d was; at d = 8 it needs 8 KiB)
  extern __shared__ double kb_lds[];
  const int tid = threadIdx.x;
  const int d = p.d;
  double* su = kb_lds;
  double* sv = kb_lds + d * KT;
  const int64_t i0 = (int64_t)ti * KT, j0 = (int64_t)tj * KT;
  pair_tile::stage_panels(su, U, i0, nu, sv, V, j0, nv, d);
  __syncthreads();
  const int ty = pair_tile::thread_row(tid), tx = pair_tile::thread_col(tid);
  double s[4][4];  // s, then the covariance function of it
  if constexpr (KERNEL == GPMI_KERNEL_PER) {
    // the warped distance and its exp half by half: sinpi_sq and exp_neg each hold eight elements' temporaries
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double s8[8], C8[8];
      pair_tile::accumulate_s_periodic<2>(p, d, su, sv, ty, tx, 2 * h, s8);
      kfun<GPMI_KERNEL_PER>(p, s8, C8);
#pragma unroll
      for (int i = 0; i < 8; ++i) s[2 * h + (i >> 2)][i & 3] = C8[i];
    }
  } else {
    pair_tile::accumulate_s(p.inv_l2, d, su, sv, ty, tx, s);
    pair_tile::for_each_profile<KERNEL, false>(p, s, [&](int r, int c, double C) { s[r][c] = C; });
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t gi = i0 + ty * 4 + r;
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t gj = j0 + tx * 4 + c;
      double val;
      if (gi < nu && gj < nv) {
        double cfun = s[r][c];
        if (SQUARE && gi == gj) {
          // a^2 (C + 1e-12) + WhiteNoise + sig   (covariance.py:254-255, 163-169; regression.py:239)
          val = p.a2 * (cfun + 1e-12);
          val += p.extra_diag;
          val += noise[gi];
        } else {
          val = p.a2 * cfun;
        }
      } else {
        val = (SQUARE && gi == gj) ? 1.0 : 0.0;  // padding: identity keeps the factorisation trivial
      }
      v[c] = val;
    }
    double* dst = out + gi * ld + j0 + tx * 4;
    *reinterpret_cast<d2_t*>(dst) = d2_t{v[0], v[1]};
    *reinterpret_cast<d2_t*>(dst + 2) = d2_t{v[2], v[3]};
  }
}

__global__ void add_full_kernel(double* __restrict__ A, int64_t ld, const double* __restrict__ Y,
                                int64_t n) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t i = blockIdx.y;
  if (j < n) A[i * ld + j] += Y[i * n + j];
}

}  // namespace

// ---- sums of stationary kernels (GPMI_KERNEL_SUM) ---------------------------------------------------------------------
// K = sum_m a_m^2 C_m (+ a_m^2 1e-12 each on the diagonal, covariance.py:254-255,348) + WhiteNoise + data errors in ONE
// pass per 64 x 64 tile: the two point panels are staged once and shared by the components; per component the thread
// accumulates s_m = sum_k 1/2 dx_k^2 / l_{m,k}^2 with that component's length scales and applies its covariance function
// (kfun, the same lockstep exp / log1p as the single-kernel build), summing in component order - the order of the
// reference's sum(...) (covariance.py:94-98).  The component's kind is a uniform run-time branch (one per component and
// half-block), not a template parameter: one kernel serves every combination of two to four SE / RQ / Matern / Periodic components instead
// of one instantiation each competing for the instruction cache.  The choice rests on that code size: a per-combination
// instantiation was not built or timed.  Timings of this form: DESIGN.md (kernel table) and tools/sum_time.py.
// ksum_body is force-inlined: used by two kernels, the compiler otherwise made it a called function, and the batched
// kernel then took 248 VGPRs and a scratch spill behind the call (inlined: 130 VGPRs, no scratch, as ksum_kernel).
namespace {

template <bool SQUARE>
__device__ __forceinline__ void ksum_body(const CovParams& p, const double* __restrict__ U, int64_t nu,
                                 const double* __restrict__ V, int64_t nv, const double* __restrict__ noise,
                                 double* __restrict__ out, int64_t ld, int lower_only) {
  int ti = blockIdx.y, tj = blockIdx.x;
  const int tile_off = lower_only >> 8;  // (tile selection as in kbuild_body)
  lower_only &= 0xff;
  if (SQUARE && lower_only == 2) {
    const int id = blockIdx.x;
    ti = (int)((sqrt(8.0 * id + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
    while (ti * (ti + 1) / 2 > id) --ti;
    tj = id - ti * (ti + 1) / 2 + tile_off;
    ti += tile_off;
  } else if (SQUARE && lower_only && tj > ti) {
    return;
  }
  extern __shared__ double ks_lds[];
  const int tid = threadIdx.x;
  // (uniform values, read first-lane: a batched launch takes its parameters from memory, and the component branch and
  // the loop bounds stay scalar)
  const int d = __builtin_amdgcn_readfirstlane(p.d);
  double* su = ks_lds;
  double* sv = ks_lds + d * KT;
  const int64_t i0 = (int64_t)ti * KT, j0 = (int64_t)tj * KT;
  pair_tile::stage_panels(su, U, i0, nu, sv, V, j0, nv, d);
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  const int nk = __builtin_amdgcn_readfirstlane(p.nk);
  // two halves of eight elements (rows 2h, 2h + 1 of the thread's 4 x 4 block), each summed over all components and
  // written before the next: eight accumulators, one half's distances and covariance temporaries live at a time.  Still
  // about twice the single-kernel build's footprint: 130 VGPRs at occupancy 3 (124 / 4 for the cross build) against
  // 70 - 78 VGPRs at 6 - 7 for kbuild_kernel - both covariance functions are inlined behind the run-time branch, and
  // this VALU-bound kernel has half the waves to hide latency with.
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0;
    for (int m = 0; m < nk; ++m) {
      const KParams& q = p.comp[m];
      double sv8[8], cf8[8];
      const int kind = __builtin_amdgcn_readfirstlane(q.kernel);
      if (kind == GPMI_KERNEL_PER) {  // the component's warped distance (pair_tile.h)
        pair_tile::accumulate_s_periodic<2>(q, d, su, sv, ty, tx, 2 * h, sv8);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) sv8[i] = 0.0;
        for (int k = 0; k < d; ++k) {
          const double il2 = q.inv_l2[k];
          double ur[2], vc[4];
#pragma unroll
          for (int r = 0; r < 2; ++r) ur[r] = su[k * KT + ty * 4 + 2 * h + r];
#pragma unroll
          for (int c = 0; c < 4; ++c) vc[c] = sv[k * KT + tx * 4 + c];
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              double dx = ur[r] - vc[c];
              sv8[4 * r + c] = fma(0.5 * dx * dx, il2, sv8[4 * r + c]);
            }
        }
      }
      switch (kind) {  // (make_cov admits these five kinds only; Periodic: SE's exp of its own s)
        case GPMI_KERNEL_RQ: kfun<GPMI_KERNEL_RQ>(q, sv8, cf8); break;
        case GPMI_KERNEL_M32: kfun<GPMI_KERNEL_M32>(q, sv8, cf8); break;
        case GPMI_KERNEL_M52: kfun<GPMI_KERNEL_M52>(q, sv8, cf8); break;
        default: kfun<GPMI_KERNEL_SE>(q, sv8, cf8); break;
      }
      const double a2 = q.a2;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t gi = i0 + ty * 4 + 2 * h + r, gj = j0 + tx * 4 + c;
          const double cfun = cf8[4 * r + c];
          // a_m^2 (C_m + 1e-12) on the diagonal, a_m^2 C_m off it (covariance.py:254-255, 348), in component order
          acc[4 * r + c] += (SQUARE && gi == gj) ? a2 * (cfun + 1e-12) : a2 * cfun;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t gi = i0 + ty * 4 + 2 * h + r;
      double v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t gj = j0 + tx * 4 + c;
        double val;
        if (gi < nu && gj < nv) {
          val = acc[4 * r + c];
          if (SQUARE && gi == gj) {
            val += p.extra_diag;  // + WhiteNoise + sig, in kbuild_body's order
            val += noise[gi];
          }
        } else {
          val = (SQUARE && gi == gj) ? 1.0 : 0.0;  // identity padding
        }
        v[c] = val;
      }
      double* dst = out + gi * ld + j0 + tx * 4;
      *reinterpret_cast<d2_t*>(dst) = d2_t{v[0], v[1]};
      *reinterpret_cast<d2_t*>(dst + 2) = d2_t{v[2], v[3]};
    }
  }
}

template <bool SQUARE>
__global__ __launch_bounds__(256) void ksum_kernel(CovParams p, const double* __restrict__ U, int64_t nu,
                                                   const double* __restrict__ V, int64_t nv,
                                                   const double* __restrict__ noise, double* __restrict__ out,
                                                   int64_t ld, int lower_only) {
  ksum_body<SQUARE>(p, U, nu, V, nv, noise, out, ld, lower_only);
}

// batched square build of sums: problem z uses pdev[z], writes out + z * stride
__global__ __launch_bounds__(256) void ksum_batched_kernel(const CovParams* __restrict__ pdev,
                                                           const double* __restrict__ x, int64_t n,
                                                           const double* __restrict__ noise, double* __restrict__ out,
                                                           int64_t ld, int64_t stride) {
  ksum_body<true>(pdev[blockIdx.z], x, n, x, n, noise, out + (int64_t)blockIdx.z * stride, ld, 2);
}

// batched cross build of sums (kbuild_cross_batched_kernel for GPMI_KERNEL_SUM)
__global__ __launch_bounds__(256) void ksum_cross_batched_kernel(const CovParams* __restrict__ pdev,
                                                                 const double* __restrict__ U, int64_t nu,
                                                                 const double* __restrict__ V, int64_t nv,
                                                                 double* __restrict__ out, int64_t ld, int64_t stride) {
  ksum_body<false>(pdev[blockIdx.z], U, nu, V, nv, nullptr, out + (int64_t)blockIdx.z * stride, ld, 0);
}

}  // namespace

static size_t kb_lds_bytes(int d) { return sizeof(double) * 2 * (size_t)d * KT; }

// dispatch on the covariance function (a template parameter of the kernels).  A KParams is one stationary kernel: a sum
// reaches the builders only as a CovParams (the overloads below), so a KParams whose kind is GPMI_KERNEL_SUM is a sliced
// copy - a bug of the caller.
// The builders' own dispatch: the stationary kernels and GPMI_KERNEL_PER (with_stationary_kernel also instantiates the
// sparse-model, selection and Hessian kernels, which do not take the Periodic kernel).
template <class F>
static bool with_builder_kernel(int kernel, F&& f) {
  if (kernel == GPMI_KERNEL_PER) {
    f(std::integral_constant<int, GPMI_KERNEL_PER>());
    return true;
  }
  return with_stationary_kernel(kernel, f);
}

template <bool SQUARE>
static void launch_kb(dim3 grid, hipStream_t s, const KParams& p, const double* U, int64_t nu, const double* V,
                      int64_t nv, const double* noise, double* out, int64_t ld, int lower_only) {
  [[maybe_unused]] const bool ok = with_builder_kernel(p.kernel, [&](auto K) {
    hipLaunchKernelGGL((kbuild_kernel<SQUARE, decltype(K)::value>), grid, dim3(256), kb_lds_bytes(p.d), s, p, U, nu, V, nv,
                       noise, out, ld, lower_only);
  });
  assert(ok && "a sum of kernels must be passed as a CovParams");  // (make_params admits no other kind)
}

// a CovParams: the fused build of its sum, or the single-kernel build of its base
template <bool SQUARE>
static void launch_kb(dim3 grid, hipStream_t s, const CovParams& p, const double* U, int64_t nu, const double* V,
                      int64_t nv, const double* noise, double* out, int64_t ld, int lower_only) {
  if (p.kernel == GPMI_KERNEL_SUM)
    hipLaunchKernelGGL(ksum_kernel<SQUARE>, grid, dim3(256), kb_lds_bytes(p.d), s, p, U, nu, V, nv, noise, out, ld,
                       lower_only);
  else
    launch_kb<SQUARE>(grid, s, static_cast<const KParams&>(p), U, nu, V, nv, noise, out, ld, lower_only);
}

template <class P>
static void kbuild_square(hipStream_t s, const P& p, const double* x, int64_t n, int64_t np, const double* noise,
                          double* A, int64_t ld, bool lower_only) {
  const unsigned nt = (unsigned)(np / KT);
  dim3 grid = lower_only ? dim3(nt * (nt + 1) / 2) : dim3(nt, nt);
  launch_kb<true>(grid, s, p, x, n, x, n, noise, A, ld, lower_only ? 2 : 0);
}

// The lower tiles in two launches: part 1 = the first `split_cols` columns (all rows), part 2 = everything to the right
// of them.  The fit starts factoring the first outer panel behind part 1 while part 2 is still being built on the
// update stream (api.hip: enqueue_factor_and_forward).
template <class P>
static void kbuild_square_part(hipStream_t s, const P& p, const double* x, int64_t n, int64_t np, const double* noise,
                               double* A, int64_t ld, int part, int split_cols) {
  const unsigned nt = (unsigned)(np / KT), sp = (unsigned)(split_cols / KT);
  if (part == 1) {
    launch_kb<true>(dim3(sp, nt), s, p, x, n, x, n, noise, A, ld, 1);
  } else if (nt > sp) {
    const unsigned m = nt - sp;
    launch_kb<true>(dim3(m * (m + 1) / 2), s, p, x, n, x, n, noise, A, ld, 2 | (int)(sp << 8));
  }
}

template <class P>
static void kbuild_cross(hipStream_t s, const P& p, const double* U, int64_t mu, int64_t mp, const double* V, int64_t n,
                         int64_t np, double* out, int64_t ld) {
  dim3 grid((unsigned)(np / KT), (unsigned)(mp / KT));
  launch_kb<false>(grid, s, p, U, mu, V, n, nullptr, out, ld, 0);
}

void launch_kbuild_square(hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np,
                          const double* noise, double* A, int64_t ld, bool lower_only) {
  kbuild_square(s, p, x, n, np, noise, A, ld, lower_only);
}
void launch_kbuild_square(hipStream_t s, const CovParams& p, const double* x, int64_t n, int64_t np,
                          const double* noise, double* A, int64_t ld, bool lower_only) {
  kbuild_square(s, p, x, n, np, noise, A, ld, lower_only);
}

void launch_kbuild_square_part(hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np,
                               const double* noise, double* A, int64_t ld, int part, int split_cols) {
  kbuild_square_part(s, p, x, n, np, noise, A, ld, part, split_cols);
}
void launch_kbuild_square_part(hipStream_t s, const CovParams& p, const double* x, int64_t n, int64_t np,
                               const double* noise, double* A, int64_t ld, int part, int split_cols) {
  kbuild_square_part(s, p, x, n, np, noise, A, ld, part, split_cols);
}

void launch_kbuild_square_batched(hipStream_t s, int kernel, const KParams* pdev, int batch, const double* x,
                                  int64_t n, int64_t np, const double* noise, double* A, int64_t ld,
                                  int64_t stride, int d, int64_t noise_stride) {
  const unsigned nt = (unsigned)(np / KT);
  dim3 grid(nt * (nt + 1) / 2, 1, (unsigned)batch);  // lower tiles only, one-dimensional (kbuild_body, mode 2)
  [[maybe_unused]] const bool ok = with_builder_kernel(kernel, [&](auto K) {
    hipLaunchKernelGGL(kbuild_batched_kernel<decltype(K)::value>, grid, dim3(256), kb_lds_bytes(d), s, pdev, x, n, noise, A,
                       ld, stride, noise_stride);
  });
  assert(ok && "a batch of sums is an array of CovParams");
}

// a batch of sums (every pdev[z] of kind GPMI_KERNEL_SUM; the data variances are shared)
void launch_kbuild_square_batched(hipStream_t s, const CovParams* pdev, int batch, const double* x, int64_t n,
                                  int64_t np, const double* noise, double* A, int64_t ld, int64_t stride, int d) {
  const unsigned nt = (unsigned)(np / KT);
  dim3 grid(nt * (nt + 1) / 2, 1, (unsigned)batch);
  hipLaunchKernelGGL(ksum_batched_kernel, grid, dim3(256), kb_lds_bytes(d), s, pdev, x, n, noise, A, ld, stride);
}

void launch_kbuild_cross(hipStream_t s, const KParams& p, const double* U, int64_t mu, int64_t mp,
                         const double* V, int64_t n, int64_t np, double* out, int64_t ld) {
  kbuild_cross(s, p, U, mu, mp, V, n, np, out, ld);
}
void launch_kbuild_cross(hipStream_t s, const CovParams& p, const double* U, int64_t mu, int64_t mp,
                         const double* V, int64_t n, int64_t np, double* out, int64_t ld) {
  kbuild_cross(s, p, U, mu, mp, V, n, np, out, ld);
}

// a^2 g in the place of K = a^2 C: kbuild_body with the derivative profile as its covariance function
void launch_kbuild_cross_dprofile(hipStream_t s, const KParams& p, const double* U, int64_t mu, int64_t mp,
                                  const double* V, int64_t n, int64_t np, double* out, int64_t ld) {
  assert(kernel_is_matern(p.kernel) && "derivative-profile rows exist for the Matern kernels only");
  dim3 grid((unsigned)(np / KT), (unsigned)(mp / KT));
  if (p.kernel == GPMI_KERNEL_M32)
    hipLaunchKernelGGL((kbuild_kernel<false, KFUN_M32_G>), grid, dim3(256), kb_lds_bytes(p.d), s, p, U, mu, V, n, nullptr,
                       out, ld, 0);
  else if (p.kernel == GPMI_KERNEL_M52)
    hipLaunchKernelGGL((kbuild_kernel<false, KFUN_M52_G>), grid, dim3(256), kb_lds_bytes(p.d), s, p, U, mu, V, n, nullptr,
                       out, ld, 0);
}

// lockstep batch: K*_z (mp x ld, mu valid rows against the n valid rows of V) for problem z of `batch`, `stride` doubles
// apart; one panel of query points per launch (the caller bounds mp: gpmi_predict_batch)
void launch_kbuild_cross_batched(hipStream_t s, int kernel, const KParams* pdev, int batch, const double* U, int64_t mu,
                                 int64_t mp, const double* V, int64_t n, int64_t np, double* out, int64_t ld,
                                 int64_t stride, int d) {
  dim3 grid((unsigned)(np / KT), (unsigned)(mp / KT), (unsigned)batch);
  [[maybe_unused]] const bool ok = with_builder_kernel(kernel, [&](auto K) {
    hipLaunchKernelGGL(kbuild_cross_batched_kernel<decltype(K)::value>, grid, dim3(256), kb_lds_bytes(d), s, pdev, U, mu, V,
                       n, out, ld, stride);
  });
  assert(ok && "a batch of sums is an array of CovParams");
}
void launch_kbuild_cross_batched(hipStream_t s, const CovParams* pdev, int batch, const double* U, int64_t mu, int64_t mp,
                                 const double* V, int64_t n, int64_t np, double* out, int64_t ld, int64_t stride, int d) {
  dim3 grid((unsigned)(np / KT), (unsigned)(mp / KT), (unsigned)batch);
  hipLaunchKernelGGL(ksum_cross_batched_kernel, grid, dim3(256), kb_lds_bytes(d), s, pdev, U, mu, V, n, out, ld, stride);
}

void launch_add_full(hipStream_t s, double* A, int64_t ld, const double* Y, int64_t n) {
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)n);
  hipLaunchKernelGGL(add_full_kernel, grid, dim3(256), 0, s, A, ld, Y, n);
}
