// Joint draws from a Gaussian posterior (include/gpmi.h: gpmi_posterior_draws, gpmi_mvn_draws, gpmi_draws_normals):
// D = mu + Z L^T with L L^T = Sigma + eps I.  New here are the counter-based normal generator and four small kernels (largest
// diagonal entry, + eps I with the padding's identity, zeroing of the factor's upper triangle, + mu); Sigma, the
// factorisation and the product run on the kernels of the regression path (kbuild.hip, solve.hip, potrf.hip, gemm_f64.hip),
// unchanged.  Every reduction has a fixed order and nothing uses atomics: repeated calls are bit-identical, and a draw does
// not depend on the draws it shares a call with.
#include <limits>

#include "api_internal.h"
#include "philox.h"

namespace {

constexpr int DRAWS_NT = 256;

// Z[row][2 p], Z[row][2 p + 1] of draw s_first + row for the pairs p of a panel of `rows_padded` rows (grid.y) and mp
// columns: the normals where row < rows and the column is below m, zeros in the padding.  One 16-byte store per thread.
__global__ __launch_bounds__(DRAWS_NT) void draws_normals_kernel(double* __restrict__ Z, int64_t ld, uint64_t seed,
                                                                 uint64_t s_first, int64_t rows, int64_t m, int64_t mp) {
  const int64_t p = (int64_t)blockIdx.x * DRAWS_NT + threadIdx.x, row = blockIdx.y;
  if (2 * p >= mp) return;
  d2_t z = {0.0, 0.0};
  if (row < rows && 2 * p < m) {
    uint64_t n1, n2;
    draws_uniform_bits(seed, s_first + (uint64_t)row, (uint32_t)p, n1, n2);
    const double r = sqrt(-2.0 * log((double)n1 * DRAWS_2M53));
    double sn, cs;
    sincos(DRAWS_TWO_PI * ((double)n2 * DRAWS_2M53), &sn, &cs);
    z.x = r * cs;
    if (2 * p + 1 < m) z.y = r * sn;
  }
  *reinterpret_cast<d2_t*>(Z + row * ld + 2 * p) = z;
}

// out[0] = the largest of A[i][i], i < m - NaN if one of them is NaN.  One workgroup; a maximum has no rounding, the tree is
// fixed all the same.
__global__ __launch_bounds__(DRAWS_NT) void draws_maxdiag_kernel(const double* __restrict__ A, int64_t ld, int64_t m,
                                                                 double* __restrict__ out) {
  __shared__ double best[DRAWS_NT];
  __shared__ int nan_seen[DRAWS_NT];
  const int t = threadIdx.x;
  double v = -std::numeric_limits<double>::infinity();
  int bad = 0;
  for (int64_t i = t; i < m; i += DRAWS_NT) {
    const double d = A[i * ld + i];
    if (d != d) bad = 1;
    else if (d > v) v = d;
  }
  best[t] = v;
  nan_seen[t] = bad;
  __syncthreads();
  for (int h = DRAWS_NT / 2; h > 0; h >>= 1) {
    if (t < h) {
      if (best[t + h] > best[t]) best[t] = best[t + h];
      nan_seen[t] |= nan_seen[t + h];
    }
    __syncthreads();
  }
  if (t == 0) out[0] = nan_seen[0] ? std::numeric_limits<double>::quiet_NaN() : best[0];
}

// A <- lower(Sigma) + eps I in the first m rows, zeros above the diagonal (the factorisation loads whole diagonal tiles, and
// a caller's matrix has nothing defined in the columns m .. mp - 1); the padded rows m .. mp - 1 become rows of the identity.
__global__ __launch_bounds__(DRAWS_NT) void draws_shift_pad_kernel(double* __restrict__ A, int64_t ld, int64_t m, int64_t mp,
                                                                   double eps) {
  const int64_t j = (int64_t)blockIdx.x * DRAWS_NT + threadIdx.x, i = blockIdx.y;
  if (j >= mp) return;
  if (i >= m) A[i * ld + j] = (i == j) ? 1.0 : 0.0;
  else if (j > i) A[i * ld + j] = 0.0;
  else if (i == j) A[i * ld + j] += eps;
}

// zeros above the diagonal of the mp x mp factor: potrf_lower leaves workspace values inside the diagonal tiles and does
// not touch the tiles above them (include/gpmi.h: gpmi_dev_potrf), and the product reads L as a full matrix
__global__ __launch_bounds__(DRAWS_NT) void draws_zero_upper_kernel(double* __restrict__ A, int64_t ld, int64_t mp) {
  const int64_t j = (int64_t)blockIdx.x * DRAWS_NT + threadIdx.x, i = blockIdx.y;
  if (j < mp && j > i) A[i * ld + j] = 0.0;
}

// D[row][j] += mu[j], row < rows, j < m
__global__ __launch_bounds__(DRAWS_NT) void draws_add_mean_kernel(double* __restrict__ D, int64_t ld, const double* __restrict__ mu,
                                                                  int64_t m) {
  const int64_t j = (int64_t)blockIdx.x * DRAWS_NT + threadIdx.x, row = blockIdx.y;
  if (j < m) D[row * ld + j] += mu[j];
}

unsigned blocks(int64_t n) { return (unsigned)((n + DRAWS_NT - 1) / DRAWS_NT); }

}  // namespace

// what the device entry points share in arguments (declared in api_internal.h: sparse.hip's draws use both)
int draws_check_args(gpmi_ctx* c, int64_t m, double jitter_rel, int64_t n_draws, int64_t first_draw, const double* draws) {
  ARGCHK(c, m >= 1 && m <= GPMI_DRAWS_MAX_M, "draws: m out of range (1 .. 16384 = GPMI_DRAWS_MAX_M points)");
  ARGCHK(c, n_draws >= 1, "draws: n_draws must be at least 1");
  ARGCHK(c, first_draw >= 0 && first_draw <= std::numeric_limits<int64_t>::max() - n_draws, "draws: first_draw must not be negative");
  ARGCHK(c, std::isfinite(jitter_rel) && jitter_rel >= 0.0, "draws: jitter_rel must be finite and not negative");
  ARGCHK(c, draws != nullptr, "draws: draws_host is NULL");
  return GPMI_OK;
}

// From Sigma (mp x ld on the device, lower triangle valid in the first m rows and columns) and mu (m, device) to the
// draws on the host, on the stream of `lane` (whose matrices are not touched: the factorisation borrows its streams and
// events, as gpmi_dev_potrf does).  Sigma is factorised in place.
int draws_tail(gpmi_ctx* c, Lane& lane, double* A, int64_t ld, int64_t m, int64_t mp, const double* mu_dev, double jitter_rel,
               int64_t n_draws, const double* z_host, int64_t seed, int64_t first_draw, double* draws_host, double* eps_host,
               int* info) {
  hipStream_t s = lane.stream;
  const int64_t nt = mp / GPMI_NB;
  const int64_t P = std::min<int64_t>(GPMI_DRAWS_PANEL, round_up(n_draws, GPMI_NB));
  DevBuf<double> invD, small, Z, D;
  if (int rc = invD.alloc_zeroed(c, nt * GPMI_NB * GPMI_NB)) return rc;  // potrf_diag writes the block-lower part only (lane_alloc)
  if (int rc = small.alloc(c, 2)) return rc;  // [0] max diag, [1] the info word
  if (int rc = Z.alloc(c, P * ld)) return rc;
  if (int rc = D.alloc(c, P * ld)) return rc;
  int* info_dev = reinterpret_cast<int*>(small + 1);
  double maxd = 0.0;
  int inf = 0;
  {
    ProfScope ps(c, s, GPMI_PROF_DRAWS_FACTOR, (double)mp * mp * mp / 3.0, 8.0 * mp * mp);
    hipLaunchKernelGGL(draws_maxdiag_kernel, dim3(1), dim3(DRAWS_NT), 0, s, A, ld, m, small);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&maxd, small, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (!(std::isfinite(maxd) && maxd > 0.0)) {
      if (info) *info = 1;
      return GPMI_OK;
    }
    const double eps = jitter_rel * maxd;
    if (eps_host) *eps_host = eps;
    hipLaunchKernelGGL(draws_shift_pad_kernel, dim3(blocks(mp), (unsigned)mp), dim3(DRAWS_NT), 0, s, A, ld, m, mp, eps);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(info_dev, 0, sizeof(int), s));
    potrf_lower(c, lane, A, mp, ld, invD, info_dev);
    hipLaunchKernelGGL(draws_zero_upper_kernel, dim3(blocks(mp), (unsigned)mp), dim3(DRAWS_NT), 0, s, A, ld, mp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&inf, info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  INFOCHK(c, inf);
  if (info) *info = inf;
  if (inf != 0) return GPMI_OK;

  // ring_order_only: a row's sums must not depend on the number of row tiles (gpmi_internal.h: GemmBatch)
  GemmBatch gb;
  gb.ring_order_only = true;
  for (int64_t s0 = 0; s0 < n_draws; s0 += P) {
    const int64_t rows = std::min<int64_t>(P, n_draws - s0), rp = round_up(rows, GPMI_NB);
    {
      ProfScope ps(c, s, GPMI_PROF_DRAWS_NORMALS, 0.0, 8.0 * rp * mp);
      if (z_host) {
        HIPCHK(c, hipMemsetAsync(Z, 0, sizeof(double) * rp * ld, s));
        HIPCHK(c, hipMemcpy2DAsync(Z, sizeof(double) * ld, z_host + s0 * m, sizeof(double) * m, sizeof(double) * m,
                                   (size_t)rows, hipMemcpyHostToDevice, s));
      } else {
        hipLaunchKernelGGL(draws_normals_kernel, dim3(blocks(mp / 2), (unsigned)rp), dim3(DRAWS_NT), 0, s, Z, ld,
                           (uint64_t)seed, (uint64_t)(first_draw + s0), rows, m, mp);
        HIPCHK(c, hipGetLastError());
      }
    }
    {
      ProfScope ps(c, s, GPMI_PROF_DRAWS_PRODUCT, 2.0 * rp * mp * mp, 8.0 * (2.0 * rp * mp + (double)mp * mp));
      launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, D, ld, Z, ld, A, ld, (int)(rp / GPMI_NB), (int)nt,
                     (int)mp, nullptr, gb);
      hipLaunchKernelGGL(draws_add_mean_kernel, dim3(blocks(m), (unsigned)rows), dim3(DRAWS_NT), 0, s, D, ld, mu_dev,
                         m);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpy2DAsync(draws_host + s0 * m, sizeof(double) * m, D, sizeof(double) * ld, sizeof(double) * m,
                               (size_t)rows, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));  // (the next panel overwrites Z and D)
  }
  return GPMI_OK;
}

extern "C" {

int gpmi_posterior_draws(gpmi_ctx* c, const double* pts, int64_t m, double jitter_rel, int64_t n_draws, const double* z_host,
                         int64_t seed, int64_t first_draw, double* mu_out, double* draws_host, double* eps_host, int* info) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = draws_check_args(c, m, jitter_rel, n_draws, first_draw, draws_host)) return rc;
  ARGCHK(c, pts != nullptr, "gpmi_posterior_draws: pts_host is NULL");
  ARGCHK(c, c->fitted && c->fit_params.kernel >= 0 && c->mix_nk == 0,
         "gpmi_posterior_draws needs a successful gpmi_fit (one stationary kernel or a sum); with the model of gpmi_fit_dense / "
         "gpmi_fit_mix pass the posterior's mean and covariance to gpmi_mvn_draws");
  if (int rc = set_device(c)) return rc;
  if (info) *info = 0;
  Lane& L = c->lanes[0];
  hipStream_t s = L.stream;
  const int64_t mp = round_up(m, GPMI_NB), ldq = mp + 32;
  if (int rc = ensure_query_ws(c, mp)) return rc;
  DevBuf<double> Sigma;
  if (int rc = Sigma.alloc(c, mp * ldq)) return rc;
  double* mu_dev = c->pvec;
  {
    // mu and Sigma = K_qq - Q^T Q: the pipeline of gpmi_posterior
    ProfScope ps(c, s, GPMI_PROF_DRAWS_SIGMA, 2.0 * mp * mp * c->np + (double)mp * c->np * c->np, 8.0 * mp * (2.0 * c->np + mp));
    // (an error return leaves at most the kernel build on Sigma in flight: hipFree waits for the device before it releases)
    if (int rc = kernel_posterior_sigma(c, pts, m, mp, nullptr, Sigma, ldq)) return rc;
  }
  if (mu_out) HIPCHK(c, hipMemcpyAsync(mu_out, mu_dev, sizeof(double) * m, hipMemcpyDeviceToHost, s));
  const int rc = draws_tail(c, L, Sigma, ldq, m, mp, mu_dev, jitter_rel, n_draws, z_host, seed, first_draw,
                            draws_host, eps_host, info);
  const hipError_t e = hipStreamSynchronize(s);  // (before Sigma is released, whatever the tail returned)
  if (rc != GPMI_OK) return rc;
  HIPCHK(c, e);
  return GPMI_OK;
}

int gpmi_mvn_draws(gpmi_ctx* c, int64_t m, const double* mean, const double* cov, double jitter_rel, int64_t n_draws,
                   const double* z_host, int64_t seed, int64_t first_draw, double* draws_host, double* eps_host, int* info) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = draws_check_args(c, m, jitter_rel, n_draws, first_draw, draws_host)) return rc;
  ARGCHK(c, mean != nullptr && cov != nullptr, "gpmi_mvn_draws: mean_host or cov_host is NULL");
  if (int rc = set_device(c)) return rc;
  if (info) *info = 0;
  if (c->lanes.empty()) {
    // a bare handle (no data set): a lane of streams and events alone is all the tail needs
    c->lanes.emplace_back();
    if (int rc = lane_streams(c, c->lanes[0])) return rc;
  }
  Lane& L = c->lanes[0];
  hipStream_t s = L.stream;
  const int64_t mp = round_up(m, GPMI_NB), ldq = mp + 32;
  DevBuf<double> Sigma, mu;
  if (int rc = Sigma.alloc(c, mp * ldq)) return rc;
  if (int rc = mu.alloc(c, m)) return rc;
  {
    ProfScope ps(c, s, GPMI_PROF_DRAWS_SIGMA, 0.0, 8.0 * m * m);
    HIPCHK(c, hipMemcpyAsync(mu, mean, sizeof(double) * m, hipMemcpyHostToDevice, s));
    // (the columns m .. mp - 1 of the first m rows lie above the diagonal: draws_shift_pad_kernel zeroes them)
    HIPCHK(c, hipMemcpy2DAsync(Sigma, sizeof(double) * ldq, cov, sizeof(double) * m, sizeof(double) * m, (size_t)m,
                               hipMemcpyHostToDevice, s));
  }
  const int rc = draws_tail(c, L, Sigma, ldq, m, mp, mu, jitter_rel, n_draws, z_host, seed, first_draw,
                            draws_host, eps_host, info);
  const hipError_t e = hipStreamSynchronize(s);
  if (rc != GPMI_OK) return rc;
  HIPCHK(c, e);
  return GPMI_OK;
}

int gpmi_draws_normals(int64_t seed, int64_t first_draw, int64_t n_draws, int64_t m, double* z_host) {
  if (!z_host || m < 1 || n_draws < 1 || first_draw < 0 || first_draw > std::numeric_limits<int64_t>::max() - n_draws)
    return GPMI_ERR_ARG;
  for (int64_t row = 0; row < n_draws; ++row)
    for (int64_t p = 0; 2 * p < m; ++p) {
      uint64_t n1, n2;
      draws_uniform_bits((uint64_t)seed, (uint64_t)(first_draw + row), (uint32_t)p, n1, n2);
      const double r = std::sqrt(-2.0 * std::log((double)n1 * DRAWS_2M53));
      const double a = DRAWS_TWO_PI * ((double)n2 * DRAWS_2M53);
      z_host[row * m + 2 * p] = r * std::cos(a);
      if (2 * p + 1 < m) z_host[row * m + 2 * p + 1] = r * std::sin(a);
    }
  return GPMI_OK;
}

}  // extern "C"
