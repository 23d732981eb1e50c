// Device kernels of the generalised GP (api_generalised.hip, GeneralisedGpRegressor): Laplace's method for a log-concave
// likelihood p(y_i | f_i) on top of the latent GP f = m + K a (Rasmussen & Williams, GPML, Alg. 3.1 / 3.2 / 5.1).
//   ggp_terms_kernel   per point: g = d log p / df, W = -d^2 log p / df^2, sw = sqrt W, d3 = d^3 log p / df^3, b = W (f - m) + g,
//                      and per block the partial sums of log p and a (f - m) and the partial maxima of |f - f_prev| and |f|
//   ggp_totals_kernel  the partials in ascending order, then a fixed tree: the record the host reads once per Newton step
//   ggp_kv_kernel      Y[:, k] = K V[:, k] for 1 .. 4 vectors in one pass over the padded matrix (HBM bound)
//   ggp_blend_kernel   the halved step, a_old + s (a_new - a_old)
// and the few element-wise kernels between them.  No atomics: every sum's order is fixed by np alone.
#include "gpmi_internal.h"
#include "kmath.h"

namespace {

constexpr int GG_THREADS = 256;

// e = exp(-|t|) in (0, 1]: everything logistic below is written in e, so nothing overflows for any finite t
__device__ __forceinline__ double exp_neg_abs(double t) {
  const double x[1] = {-fabs(t)};
  double e[1];
  kmath::exp_neg(x, e);
  return e[0];
}
// softplus(t) = ln(1 + e^t) = max(t, 0) + log1p(e)
__device__ __forceinline__ double softplus_e(double t, double e) {
  const double z[1] = {e};
  double l[1];
  kmath::log1p_pos(z, l);
  return fmax(t, 0.0) + l[0];
}
// sigma(t), sigma (1 - sigma) and 1 - 2 sigma from e, without cancellation in either tail
__device__ __forceinline__ void logistic_parts(double t, double e, double& sig, double& sig1m, double& one_m2sig) {
  const double r = 1.0 / (1.0 + e);
  sig = (t >= 0.0) ? r : e * r;
  sig1m = e * r * r;
  const double h = (1.0 - e) * r;  // |1 - 2 sigma|
  one_m2sig = (t >= 0.0) ? -h : h;
}

// block sum / block maximum over GG_THREADS values in a fixed tree
__device__ __forceinline__ double block_tree(double v, double* sh, bool take_max) {
  const int k = threadIdx.x;
  __syncthreads();
  sh[k] = v;
  __syncthreads();
  for (int h = GG_THREADS / 2; h > 0; h >>= 1) {
    if (k < h) sh[k] = take_max ? fmax(sh[k], sh[k + h]) : sh[k] + sh[k + h];
    __syncthreads();
  }
  return sh[0];
}

// One point per thread.  lik: GPMI_GGP_LOGISTIC / _POISSON / _BINOMIAL; aux: s_i, e_i, n_i; lconst: the part of log p that
// does not depend on f (-ln s; y ln e - lgamma(y + 1); ln C(n, y)), computed once on the host.  fm = f - m = K a.
// Padding rows (i >= n) get g = W = sw = d3 = b = 0: B = I + sw sw^T o K is the identity there.
// part: 4 x nblk - sums of log p, sums of a fm, maxima of |fm - fm_prev| (fm_prev may be null: 0), maxima of |f|.
__global__ __launch_bounds__(GG_THREADS) void ggp_terms_kernel(int lik, const double* __restrict__ y, const double* __restrict__ aux,
                                                               const double* __restrict__ lconst, double offset,
                                                               const double* __restrict__ a, const double* __restrict__ fm,
                                                               const double* __restrict__ fm_prev, int64_t n, int64_t np,
                                                               GgpTerms t, double* __restrict__ part) {
  __shared__ double sh[GG_THREADS];
  const int64_t i = (int64_t)blockIdx.x * GG_THREADS + threadIdx.x;
  double lp = 0.0, af = 0.0, df = 0.0, fa = 0.0;
  double g = 0.0, W = 0.0, d3 = 0.0, b = 0.0;
  if (i < n) {
    const double fmi = fm[i], f = fmi + offset, yi = y[i], ax = aux[i];
    if (lik == GPMI_GGP_LOGISTIC) {
      const double is = 1.0 / ax, z = (yi - f) * is;
      const double e = exp_neg_abs(z);
      double sig, s1, m2;
      logistic_parts(z, e, sig, s1, m2);
      lp = z - 2.0 * softplus_e(z, e) + lconst[i];
      g = -m2 * is;
      W = 2.0 * s1 * is * is;
      d3 = 2.0 * s1 * m2 * is * is * is;
    } else if (lik == GPMI_GGP_POISSON) {
      const double mu = ax * exp(f);
      lp = yi * f - mu + lconst[i];
      g = yi - mu;
      W = mu;
      d3 = -mu;
    } else {  // GPMI_GGP_BINOMIAL
      const double e = exp_neg_abs(f);
      double sig, s1, m2;
      logistic_parts(f, e, sig, s1, m2);
      // y f - n softplus(f) = -(y softplus(-f) + (n - y) softplus(f)): every term of one sign, nothing cancels
      lp = lconst[i] - (yi * softplus_e(-f, e) + (ax - yi) * softplus_e(f, e));
      g = yi - ax * sig;
      W = ax * s1;
      d3 = -ax * s1 * m2;
    }
    b = fma(W, fmi, g);
    af = a[i] * fmi;
    df = fm_prev ? fabs(fmi - fm_prev[i]) : 0.0;
    fa = fabs(f);
  }
  if (i < np) {
    t.g[i] = g;
    t.W[i] = W;
    t.sw[i] = sqrt(W);
    t.d3[i] = d3;
    t.b[i] = b;
  }
  const int64_t nblk = gridDim.x;
  double v = block_tree(lp, sh, false);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
  v = block_tree(af, sh, false);
  if (threadIdx.x == 0) part[nblk + blockIdx.x] = v;
  v = block_tree(df, sh, true);
  if (threadIdx.x == 0) part[2 * nblk + blockIdx.x] = v;
  v = block_tree(fa, sh, true);
  if (threadIdx.x == 0) part[3 * nblk + blockIdx.x] = v;
}

// rec[0] = sum log p, rec[1] = a^T (f - m), rec[2] = max |f - f_prev|, rec[3] = max |f|: thread k takes the partials k,
// k + 256, ... in ascending order, then the tree
__global__ __launch_bounds__(GG_THREADS) void ggp_totals_kernel(const double* __restrict__ part, int64_t nblk, double* __restrict__ rec) {
  __shared__ double sh[GG_THREADS];
  for (int q = 0; q < 4; ++q) {
    const bool mx = q >= 2;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < nblk; k += GG_THREADS) s = mx ? fmax(s, part[q * nblk + k]) : s + part[q * nblk + k];
    const double v = block_tree(s, sh, mx);
    if (threadIdx.x == 0) rec[q] = v;
  }
}

// Y[q][row] = sum_j K[row][j] V[q][j] over the np columns of the padded matrix, NV vectors in one pass.  A wave takes a
// row; lane l adds the columns 2 l, 2 l + 1, 2 l + 128, 2 l + 129, ... in ascending order (one 16-byte load per lane and
// step: a wave reads 1 KiB of the row at a time), then a butterfly over the 64 lanes.  The order depends on np alone, and
// every vector has its own accumulator: the bits are the same whatever NV is.  Grid: np / 4 workgroups of four waves.
template <int NV>
__global__ __launch_bounds__(GG_THREADS) void ggp_kv_kernel(const double* __restrict__ K, int64_t ld, int64_t np, GgpKv a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  if (row >= np) return;
  const double* __restrict__ kr = K + row * ld;
  double acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q] = 0.0;
#pragma unroll 4
  for (int64_t j = 2 * lane; j < np; j += 128) {
    const d2_t k2 = *reinterpret_cast<const d2_t*>(kr + j);
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const d2_t v2 = *reinterpret_cast<const d2_t*>(a.v[q] + j);
      acc[q] = fma(k2[0], v2[0], acc[q]);
      acc[q] = fma(k2[1], v2[1], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double s = acc[q];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) a.y[q][row] = s;
  }
}

// out = lo + s (hi - lo) over cnt values (a and f - m lie side by side: one launch blends both)
__global__ void ggp_blend_kernel(const double* __restrict__ lo, const double* __restrict__ hi, double s, double* __restrict__ out,
                                 int64_t cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) out[i] = fma(s, hi[i] - lo[i], lo[i]);
}

// a+ = b - sw o t  (t = B^-1 (sw o K b))
__global__ void ggp_newton_a_kernel(const double* __restrict__ b, const double* __restrict__ sw, const double* __restrict__ t,
                                    double* __restrict__ a_new, int64_t np) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) a_new[i] = fma(-sw[i], t[i], b[i]);
}

// s2_i = 1/2 (K_ii - ss_i) d3_i with ss_i = |L^-1 (sw o K[:, i])|^2: half the posterior variance of f_i times d^3 log p
__global__ void ggp_s2_kernel(const double* __restrict__ K, int64_t ld, const double* __restrict__ ss, const double* __restrict__ d3,
                              double* __restrict__ s2, int64_t np) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) s2[i] = 0.5 * (K[i * ld + i] - ss[i]) * d3[i];
}

// u = g + 2 (s2 - rt)  (rt = R K s2)
__global__ void ggp_grad_u_kernel(const double* __restrict__ g, const double* __restrict__ s2, const double* __restrict__ rt,
                                  double* __restrict__ u, int64_t np) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < np) u[i] = fma(2.0, s2[i] - rt[i], g[i]);
}

// Q[r][j] *= sc[j] over `rows` rows of np columns, in place (the predict's cross-covariances: any number of rows)
__global__ void ggp_scale_cols_kernel(double* __restrict__ Q, int64_t ld, int64_t np, const double* __restrict__ sc) {
  const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (j >= np) return;
  double* q = Q + (int64_t)blockIdx.y * ld + j;
  const d2_t v = *reinterpret_cast<const d2_t*>(q);
  *reinterpret_cast<d2_t*>(q) = d2_t{v[0] * sc[j], v[1] * sc[j + 1]};
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + GG_THREADS - 1) / GG_THREADS); }

}  // namespace

int64_t ggp_part_doubles(int64_t np) { return 4 * (int64_t)blocks_for(np); }

void launch_ggp_terms(hipStream_t s, int lik, const double* y, const double* aux, const double* lconst, double offset,
                      const double* a, const double* fm, const double* fm_prev, int64_t n, int64_t np, const GgpTerms& t,
                      double* part, double* rec) {
  const unsigned nblk = blocks_for(np);
  hipLaunchKernelGGL(ggp_terms_kernel, dim3(nblk), dim3(GG_THREADS), 0, s, lik, y, aux, lconst, offset, a, fm, fm_prev, n, np, t,
                     part);
  hipLaunchKernelGGL(ggp_totals_kernel, dim3(1), dim3(GG_THREADS), 0, s, part, (int64_t)nblk, rec);
}

void launch_ggp_kv(hipStream_t s, const double* K, int64_t ld, int64_t np, int nv, const GgpKv& a) {
  const dim3 grid((unsigned)(np / 4)), block(GG_THREADS);
  switch (nv) {
    case 1: hipLaunchKernelGGL(ggp_kv_kernel<1>, grid, block, 0, s, K, ld, np, a); break;
    case 2: hipLaunchKernelGGL(ggp_kv_kernel<2>, grid, block, 0, s, K, ld, np, a); break;
    case 3: hipLaunchKernelGGL(ggp_kv_kernel<3>, grid, block, 0, s, K, ld, np, a); break;
    default: hipLaunchKernelGGL(ggp_kv_kernel<4>, grid, block, 0, s, K, ld, np, a); break;
  }
}

void launch_ggp_blend(hipStream_t s, const double* lo, const double* hi, double step, double* out, int64_t cnt) {
  hipLaunchKernelGGL(ggp_blend_kernel, dim3(blocks_for(cnt)), dim3(GG_THREADS), 0, s, lo, hi, step, out, cnt);
}

void launch_ggp_newton_a(hipStream_t s, const double* b, const double* sw, const double* t, double* a_new, int64_t np) {
  hipLaunchKernelGGL(ggp_newton_a_kernel, dim3(blocks_for(np)), dim3(GG_THREADS), 0, s, b, sw, t, a_new, np);
}

void launch_ggp_s2(hipStream_t s, const double* K, int64_t ld, const double* ss, const double* d3, double* s2, int64_t np) {
  hipLaunchKernelGGL(ggp_s2_kernel, dim3(blocks_for(np)), dim3(GG_THREADS), 0, s, K, ld, ss, d3, s2, np);
}

void launch_ggp_grad_u(hipStream_t s, const double* g, const double* s2, const double* rt, double* u, int64_t np) {
  hipLaunchKernelGGL(ggp_grad_u_kernel, dim3(blocks_for(np)), dim3(GG_THREADS), 0, s, g, s2, rt, u, np);
}

void launch_ggp_scale_cols(hipStream_t s, double* Q, int64_t ld, int64_t rows, int64_t np, const double* sc) {
  hipLaunchKernelGGL(ggp_scale_cols_kernel, dim3(blocks_for(np / 2), (unsigned)rows), dim3(GG_THREADS), 0, s, Q, ld, np, sc);
}
