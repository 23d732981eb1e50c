// Kernels of gpmi_predict_batch (api_regression.hip) besides the batched cross-covariance build (kbuild.hip): the store of
// a panel's per-row results and the mixture over the rows.
//
// The T x m means and variances of a call stay on the device until every chunk of rows is through; the mixture then reads
// them once per pass.  Its sums over the rows are pairwise trees over the listed rows IN LIST ORDER: the order of the
// additions is a function of the number of listed rows alone - no atomics, nothing that depends on how the rows were
// chunked or split over the two streams - and equal terms with power-of-two weights add up exactly (four copies of one row
// at weight 1/4 return that row).
#include "gpmi_internal.h"

namespace {

// rows [m0, m0 + rows) of problems t_first + z: mean = K* alpha + prior mean, var = |a^2 - |L^-1 k|^2| (regression.py:210-216),
// NaN for a problem whose factorisation failed
__global__ __launch_bounds__(256) void predict_store_kernel(int64_t t_first, int64_t m0, int64_t rows, int64_t m,
                                                            const double* __restrict__ dot,
                                                            const double* __restrict__ sumsq, int64_t sDot,
                                                            int64_t sSq, const char* __restrict__ params, int64_t pstride,
                                                            const int* __restrict__ info,
                                                            const double* __restrict__ mu_q,
                                                            const double* __restrict__ mu_const,
                                                            double* __restrict__ mean_t, double* __restrict__ var_t) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int64_t z = blockIdx.z, t = t_first + z;
  const int64_t o = t * m + m0 + r;
  const bool ok = info[z] == 0;
  const double nan = __builtin_nan("");
  const double prior = mu_q ? mu_q[o] : mu_const[t];
  mean_t[o] = ok ? dot[z * sDot + r] + prior : nan;
  if (sumsq) {
    const double a2 = reinterpret_cast<const KParams*>(params + z * pstride)->a2;
    var_t[o] = ok ? fabs(a2 - sumsq[z * sSq + r]) : nan;
  }
}

constexpr int MIX_DEPTH = 16;  // partial sums of a pairwise tree over up to 2^16 rows

// pairwise tree over term(0) .. term(G - 1) in order: the partial sum of a completed block of 2^k terms waits on level k
// of the thread's column of `st` until its sibling block is complete
template <class Term>
__device__ inline double tree_sum(int64_t G, double (*st)[256], Term term) {
  const int x = threadIdx.x;
  int sp = 0;
  for (int64_t g = 0; g < G; ++g) {
    double v = term(g);
    for (int64_t k = g + 1; (k & 1) == 0; k >>= 1) v = st[--sp][x] + v;
    st[sp++][x] = v;
  }
  double r = st[--sp][x];
  while (sp > 0) r = st[--sp][x] + r;
  return r;
}

// one thread per point (neighbouring threads read neighbouring points of a row)
__global__ __launch_bounds__(256) void predict_mix_kernel(int64_t G, const int* __restrict__ idx,
                                                          const double* __restrict__ w, int64_t m,
                                                          const double* __restrict__ mean_t,
                                                          const double* __restrict__ var_t,
                                                          double* __restrict__ mix_mean, double* __restrict__ mix_var) {
  __shared__ double st[MIX_DEPTH][256];
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m) return;  // (no barrier below: a thread only touches its own column of st)
  const double mean = tree_sum(G, st, [&](int64_t g) { return w[g] * mean_t[(int64_t)idx[g] * m + q]; });
  mix_mean[q] = mean;
  if (mix_var) {
    mix_var[q] = tree_sum(G, st, [&](int64_t g) {
      const int64_t o = (int64_t)idx[g] * m + q;
      const double dm = mean_t[o] - mean;
      return w[g] * (var_t[o] + dm * dm);
    });
  }
}

}  // namespace

void launch_predict_store(hipStream_t s, int batch, int64_t t_first, int64_t m0, int64_t rows, int64_t m,
                          const double* dot, const double* sumsq, int64_t sDot, int64_t sSq, const void* params,
                          int64_t pstride, const int* info, const double* mu_q, const double* mu_const, double* mean_t,
                          double* var_t) {
  hipLaunchKernelGGL(predict_store_kernel, dim3((unsigned)((rows + 255) / 256), 1, (unsigned)batch), dim3(256), 0, s, t_first,
                     m0, rows, m, dot, sumsq, sDot, sSq, static_cast<const char*>(params), pstride, info, mu_q, mu_const, mean_t,
                     var_t);
}

void launch_predict_mix(hipStream_t s, int64_t G, const int* idx, const double* w, int64_t m, const double* mean_t,
                        const double* var_t, double* mix_mean, double* mix_var) {
  hipLaunchKernelGGL(predict_mix_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, G, idx, w, m, mean_t, var_t,
                     mix_mean, mix_var);
}
