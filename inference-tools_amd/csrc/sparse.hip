// Variational inducing-point GP regression (include/gpmi.h: gpmi_sgp_*; Titsias 2009) on gfx950.
//
// N data points are summarised by m <= 4096 inducing inputs Z.  With W = diag(1 / sigma_i^2):
//   K_mm + eps I = L L^T,  G = K_mn W K_nm,  H = L^-1 G L^-T,  B = I + H = L_B L_B^T,  c = L_B^-1 L^-1 K_mn W r,
//   F = -1/2 [N ln 2 pi + sum ln sigma_i^2 + 2 sum ln diag(L_B) + r^T W r - c^T c] - 1/2 [a^2 sum w_i - tr H].
// Pass 1 walks x in panels: cross build of the m x P panel of K_mn (kbuild.hip), columns scaled by 1 / sigma_i, G accumulated
// on the fp64 matrix cores (gemm_f64.hip, lower tiles), b = K_mn W r by rows.  The m x m algebra is the lockstep
// factorisation and inverse of the small-problem path (potrf_lower_batched, trsm_identity_batched, batch of one) and
// products with the explicit triangular inverses L^-1, L_B^-1 - B is factorised, never K_mm^-1 G or the N x N matrix.
// Pass 2 (gradient) rebuilds every panel transposed (P x m: rows are data points), forms alpha = W (r - K_nm gamma), the
// weight panel T K_mn (one GEMM) and contracts  sum_ij M1_ij dK(z_i, x_j)/dtheta  in sgp_contract_kernel: the 64 x 64 pair
// tile of the builders (pair_tile.h: both point panels staged in LDS, s and the value and derivative profiles of kfun.h
// recomputed - C is bit for bit the builders' value), one partial per tile and parameter, summed by a second kernel in a
// fixed order.  The K_mm term runs through the same kernel (rows = Z).  sgp_zcontract_kernel (dF/dZ) and sgp_qgrad_kernel
// (below) stand on the same tile and on its column reduction, pair_tile::reduce_columns, with one and two weight arrays.
//   gamma = L^-T L_B^-T c;  beta = K_mm^-1 K_mn alpha = gamma (exactly: (K_mm + G) gamma = b);  S = L^-T B^-1 L^-1;
//   T = L^-T L^-1 - S;  M1 = gamma alpha^T + T K_mn W;  M2 = gamma gamma^T + K_mm^-1 G K_mm^-1 - T;
//   dF/dtheta = sum M1 o dK_mn - 1/2 sum M2 o d(K_mm + eps I) - 1/2 sum w_i da^2/dtheta;
//   dF/d ln s = s^2 sum_i [alpha_i^2 - w_i + w_i^2 (a^2 - k_i^T T k_i)].
// The fitted model (L^-1, L_B^-1, c, gamma kept by gpmi_sgp_fit) answers in O(M m^2): mean and variance (gpmi_sgp_predict), the
// joint posterior mu = U c, Sigma = K_qq - V V^T + U U^T and joint draws through the tail of draws.hip (gpmi_sgp_posterior,
// gpmi_sgp_posterior_draws), and the derivatives of mean and variance by the query point (gpmi_sgp_spatial_derivatives):
// four products per panel for the rows t(q)^T = (L^-T (L_B^-T u - v))^T, then sgp_qgrad_kernel: one profile evaluation
// weighted twice, by gamma and by t(q).
// Every reduction has a fixed order, nothing uses atomics: a call repeated gives the same bits.
// Lockstep batches (gpmi_sgp_bound_batch: T hyper-parameter vectors on one object) run the launches of the two passes with a
// chunk of problems in blockIdx.z, on the same kernels, and wait for the host once per chunk (sgp_batch_chunk, below).
#include <limits>

#include "api_internal.h"
#include "pair_tile.h"

struct gpmi_sgp {
  gpmi_ctx* ctx = nullptr;
  int64_t n = 0, d = 0, m = 0, mp = 0, ld = 0;
  DevBuf<double> x, z, r, nv;  // n x d, m x d, n, n
  DevBuf<double> w, alpha;     // n each: 1 / sigma_i^2, alpha
  bool have_targets = false;
  // mp x ld work matrices (roles in sgp_factor / sgp_gradient) and the inverse diagonal blocks of the two factors
  DevBuf<double> M[9];
  DevBuf<double> invD1, invD2;
  DevBuf<double> vec;   // 4 x mp: b, L^-1 b, c, gamma
  DevBuf<double> red;   // 128 small results
  DevBuf<int> info;     // 2 words
  DevBuf<double> part;  // SGP_RED_BLOCKS x 4 partial sums over the data
  // panels (allocated at first use): three of max(mp (R + 32), R ld) doubles, three vectors of R, the contraction's partials
  DevBuf<double> P[3], pvec, ws;
  int64_t panel_cap = 0;  // rows the five hold
  // the gradient by Z (allocated at first use): the partials per run of data tiles, the mp x d accumulator
  DevBuf<double> zws, zacc;
  // query staging: 1024 x d points, 2 x 1024 results
  DevBuf<double> q_pts, q_out;
  // the derivatives by the query point (allocated at first use): the partials per run of inducing tiles and the two
  // results of a query panel, (mp / 128 + 1) x 2 x 1024 x d doubles
  DevBuf<double> qws;
  // the fit: L^-1, L_B^-1 (mp x ld), c and gamma = L^-T L_B^-T c (mp each), the kernel
  DevBuf<double> fLinv, fLBinv, fc, fgamma;
  KParams fp = {};
  bool fitted = false;
  // lockstep batches (gpmi_sgp_bound_batch): y itself, the range of the noise variances as the host saw them go up (nv is
  // shared with gpmi_sgp_set_targets) and the workspace of `cap` problems side by side, grown on demand
  DevBuf<double> y;
  bool have_obs = false;
  double nv_lo = 0.0, nv_hi = 0.0;
  bool nv_nan = false;
  struct BatchWs {
    int64_t cap = 0, panel = 0;
    bool grad = false;
    DevBuf<double> M[9], invD1, invD2, vec, red, part, P[3], w, r, alpha, ws, white, mu;
    DevBuf<int> info;  // [0, cap): K_mm + eps I, [cap, 2 cap): B
    DevBuf<KParams> params;
  } bw;
};

namespace {

using pair_tile::block_sum;
using pair_tile::KT;
constexpr int SGP_NT = pair_tile::NT;
constexpr int SGP_RED_BLOCKS = 1024;
constexpr int SGP_QPANEL = 1024;
constexpr int64_t SGP_MAX_PANEL = 32768;
// slots of gpmi_sgp::red
constexpr int RED_DATA = 0;   // r^T W r, sum ln sigma^2, sum w, count of non-positive variances
constexpr int RED_MM = 4;     // sum ln diag(L_B), tr H, c^T c
constexpr int RED_NOISE = 8;  // sum_i [alpha_i^2 - w_i + w_i^2 (a^2 - k_i^T T k_i)]
constexpr int RED_GRAD = 16;  // n_theta partial derivatives

// w_i = 1 / (nv_i + white) and, per workgroup, the partial sums [r^T W r, sum ln sigma^2, sum w, bad] over its
// grid-strided share of the data (bad: variances that are not positive and finite; their w is 0).
// The kernels below take a lockstep batch in blockIdx.z: problem z reads and writes its arrays `z * stride` doubles behind
// the pointers (SgpStrides; all 0 for the single evaluation) and, where a scalar differs by problem, takes it from an
// array of one value per problem in the place of the argument (whites, pdev; nullptr: the argument).
__global__ __launch_bounds__(SGP_NT) void sgp_weights_kernel(const double* __restrict__ r, const double* __restrict__ nv,
                                                             double white, const double* __restrict__ whites, int64_t n,
                                                             double* __restrict__ w, double* __restrict__ part, int64_t sN,
                                                             int64_t sPart) {
  __shared__ double red[4];
  const int64_t z = blockIdx.z;
  if (whites) white = whites[z];
  r += z * sN;
  w += z * sN;
  part += z * sPart;
  double rwr = 0.0, lns = 0.0, sw = 0.0, bad = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SGP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * SGP_NT) {
    const double s2 = nv[i] + white;
    const bool ok = s2 > 0.0 && s2 < std::numeric_limits<double>::infinity();
    const double wi = ok ? 1.0 / s2 : 0.0;
    w[i] = wi;
    if (ok) {
      rwr = fma(r[i] * r[i], wi, rwr);
      lns += log(s2);
      sw += wi;
    } else {
      bad += 1.0;
    }
  }
  const double v0 = block_sum(rwr, red), v1 = block_sum(lns, red), v2 = block_sum(sw, red), v3 = block_sum(bad, red);
  if (threadIdx.x == 0) {
    double* o = part + (int64_t)blockIdx.x * 4;
    o[0] = v0;
    o[1] = v1;
    o[2] = v2;
    o[3] = v3;
  }
}

// out[j] (+)= sum_t ws[t][j], t < nrows, in a fixed order: thread-strided partial sums, then a tree (workgroup j)
__global__ __launch_bounds__(SGP_NT) void sgp_colsum_kernel(const double* __restrict__ ws, int64_t nrows, int width,
                                                            double* __restrict__ out, int accumulate, int64_t sWs,
                                                            int64_t sOut) {
  __shared__ double red[4];
  const int j = blockIdx.x;
  ws += (int64_t)blockIdx.z * sWs;
  out += (int64_t)blockIdx.z * sOut;
  double acc = 0.0;
  for (int64_t t = threadIdx.x; t < nrows; t += SGP_NT) acc += ws[t * width + j];
  const double v = block_sum(acc, red);
  if (threadIdx.x == 0) out[j] = accumulate ? out[j] + v : v;
}

// K[i][j] *= sqrt(w[j]), i < rows (grid.y), j < cols
__global__ __launch_bounds__(SGP_NT) void sgp_scale_cols_kernel(double* __restrict__ K, int64_t ld, int64_t cols,
                                                                const double* __restrict__ w, int64_t sK, int64_t sN) {
  const int64_t j = (int64_t)blockIdx.x * SGP_NT + threadIdx.x, i = blockIdx.y, z = blockIdx.z;
  if (j < cols) K[z * sK + i * ld + j] *= sqrt(w[z * sN + j]);
}

// b[i] (+)= sum_j Kw[i][j] r[j] sqrt(w[j]), j < cols; workgroup i
__global__ __launch_bounds__(SGP_NT) void sgp_bvec_kernel(const double* __restrict__ Kw, int64_t ld, int64_t cols,
                                                          const double* __restrict__ r, const double* __restrict__ w,
                                                          double* __restrict__ b, int accumulate, int64_t sK, int64_t sN,
                                                          int64_t sVec) {
  __shared__ double red[4];
  const int64_t i = blockIdx.x, z = blockIdx.z;
  Kw += z * sK;
  r += z * sN;
  w += z * sN;
  b += z * sVec;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < cols; j += SGP_NT) acc = fma(Kw[i * ld + j], r[j] * sqrt(w[j]), acc);
  const double v = block_sum(acc, red);
  if (threadIdx.x == 0) b[i] = accumulate ? b[i] + v : v;
}

// A[i][i] += eps for i < m; = 1 in the padding (the cross build leaves zeros there)
// (pdev: eps = jitter a^2 of problem z)
__global__ void sgp_pad_diag_kernel(double* __restrict__ A, int64_t ld, int64_t m, int64_t mp, double eps, double jitter,
                                    const KParams* __restrict__ pdev, int64_t sMat) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= mp) return;
  if (pdev) eps = __dmul_rn(jitter, pdev[blockIdx.z].a2);  // (rounded on its own, as the host's product is)
  A += (int64_t)blockIdx.z * sMat;
  if (i < m) A[i * ld + i] += eps;
  else A[i * ld + i] = 1.0;
}

// dst = src^T (mp x mp, 64 x 64 tiles through LDS)
__global__ __launch_bounds__(SGP_NT) void sgp_transpose_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                               int64_t ld, int64_t sMat) {
  __shared__ double t[64][65];
  src += (int64_t)blockIdx.z * sMat;
  dst += (int64_t)blockIdx.z * sMat;
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) t[r][tx] = src[((int64_t)ti * 64 + r) * ld + (int64_t)tj * 64 + tx];
  __syncthreads();
  for (int r = ty; r < 64; r += 4) dst[((int64_t)tj * 64 + r) * ld + (int64_t)ti * 64 + tx] = t[tx][r];
}

// B = 1/2 (H + H^T) + I
__global__ __launch_bounds__(SGP_NT) void sgp_sym_b_kernel(const double* __restrict__ H, double* __restrict__ B, int64_t ld,
                                                           int64_t sMat) {
  __shared__ double t[64][65];
  H += (int64_t)blockIdx.z * sMat;
  B += (int64_t)blockIdx.z * sMat;
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) t[r][tx] = H[((int64_t)tj * 64 + r) * ld + (int64_t)ti * 64 + tx];
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int64_t i = (int64_t)ti * 64 + r, j = (int64_t)tj * 64 + tx;
    B[i * ld + j] = 0.5 * (H[i * ld + j] + t[tx][r]) + (i == j ? 1.0 : 0.0);
  }
}

// out = [sum ln LB_ii, sum H_ii, sum c_i^2], i < m; one workgroup
__global__ __launch_bounds__(SGP_NT) void sgp_mm_reduce_kernel(const double* __restrict__ LB, const double* __restrict__ H,
                                                               int64_t ld, int64_t m, const double* __restrict__ c,
                                                               double* __restrict__ out, int64_t sMat, int64_t sVec,
                                                               int64_t sOut) {
  __shared__ double red[4];
  const int64_t z = blockIdx.z;
  LB += z * sMat;
  H += z * sMat;
  c += z * sVec;
  out += z * sOut;
  double a = 0.0, b = 0.0, q = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += SGP_NT) {
    a += log(LB[i * ld + i]);
    b += H[i * ld + i];
    q = fma(c[i], c[i], q);
  }
  const double v0 = block_sum(a, red), v1 = block_sum(b, red), v2 = block_sum(q, red);
  if (threadIdx.x == 0) {
    out[0] = v0;
    out[1] = v1;
    out[2] = v2;
  }
}

// C = A - B (mp rows in grid.y, mp columns)
__global__ __launch_bounds__(SGP_NT) void sgp_sub_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                         double* __restrict__ C, int64_t ld, int64_t mp, int64_t sMat) {
  const int64_t j = (int64_t)blockIdx.x * SGP_NT + threadIdx.x, i = blockIdx.y, o = (int64_t)blockIdx.z * sMat;
  if (j < mp) C[o + i * ld + j] = A[o + i * ld + j] - B[o + i * ld + j];
}

// out[j] = sum_a K[j][a] M[j][a], a < m; workgroup j
__global__ __launch_bounds__(SGP_NT) void sgp_rowdot2_kernel(const double* __restrict__ K, const double* __restrict__ M,
                                                             int64_t ld, int64_t m, double* __restrict__ out, int64_t sK,
                                                             int64_t sVec) {
  __shared__ double red[4];
  const int64_t j = blockIdx.x, z = blockIdx.z;
  K += z * sK;
  M += z * sK;
  out += z * sVec;
  double acc = 0.0;
  for (int64_t a = threadIdx.x; a < m; a += SGP_NT) acc = fma(K[j * ld + a], M[j * ld + a], acc);
  const double v = block_sum(acc, red);
  if (threadIdx.x == 0) out[j] = v;
}

// alpha_j = w_j (r_j - kg_j) and, with q (k_j^T T k_j), the noise-gradient term of the point; j < rows
__global__ __launch_bounds__(SGP_NT) void sgp_alpha_kernel(const double* __restrict__ r, const double* __restrict__ w,
                                                           const double* __restrict__ kg, const double* __restrict__ q,
                                                           double a2, const KParams* __restrict__ pdev, int64_t rows,
                                                           double* __restrict__ alpha, double* __restrict__ term, int64_t sN,
                                                           int64_t sVec) {
  const int64_t j = (int64_t)blockIdx.x * SGP_NT + threadIdx.x, z = blockIdx.z;
  if (j >= rows) return;
  if (pdev) a2 = pdev[z].a2;
  r += z * sN;
  w += z * sN;
  alpha += z * sN;
  kg += z * sVec;
  if (q) q += z * sVec;
  term += z * sVec;
  const double wj = w[j], a = wj * (r[j] - kg[j]);
  alpha[j] = a;
  if (q) term[j] = a * a - wj + wj * wj * (a2 - q[j]);
}

// mean_j = sum_a U[j][a] c[a],  var_j = a2 - |V_j|^2 + |U_j|^2, a < m; workgroup j
__global__ __launch_bounds__(SGP_NT) void sgp_predict_kernel(const double* __restrict__ V, const double* __restrict__ U,
                                                             int64_t ld, int64_t m, const double* __restrict__ c, double a2,
                                                             double* __restrict__ mean, double* __restrict__ var) {
  __shared__ double red[4];
  const int64_t j = blockIdx.x;
  double mu = 0.0, sv = 0.0, su = 0.0;
  for (int64_t a = threadIdx.x; a < m; a += SGP_NT) {
    const double v = V[j * ld + a], u = U[j * ld + a];
    mu = fma(u, c[a], mu);
    sv = fma(v, v, sv);
    su = fma(u, u, su);
  }
  const double t0 = block_sum(mu, red), t1 = block_sum(sv, red), t2 = block_sum(su, red);
  if (threadIdx.x == 0) {
    mean[j] = t0;
    var[j] = a2 - t1 + t2;
  }
}

// The weights of a thread's 4 x 4 block (rows gi0 .., columns gj0 ..) in the two weighted contractions:
//   w_ij = m_scale rs_i Mw[i][j] + uv_scale uvec_i vvec_j   (rs == nullptr: 1);   0, and nothing read, where i >= nu or j >= nv
__device__ __forceinline__ void pair_weights(int64_t gi0, int64_t nu, int64_t gj0, int64_t nv, const double* __restrict__ Mw,
                                             int64_t ld, const double* __restrict__ rs, double m_scale,
                                             const double* __restrict__ uvec, double uv_scale, const double* __restrict__ vvec,
                                             double (&w)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t gi = gi0 + r;
    const bool row_ok = gi < nu;
    const double ui = row_ok ? uv_scale * uvec[gi] : 0.0;
    const double ri = row_ok ? (rs ? m_scale * rs[gi] : m_scale) : 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t gj = gj0 + c;
      w[r][c] = (row_ok && gj < nv) ? fma(ri, Mw[gi * ld + gj], ui * vvec[gj]) : 0.0;
    }
  }
}

// The rectangular weighted gradient contraction: tile (blockIdx.y, blockIdx.x) of (rows of U) x (rows of V) reduces
//   sum_ij w_ij dK(u_i, v_j) / dtheta_k,   w_ij = m_scale rs_i Mw[i][j] + uv_scale uvec_i vvec_j   (rs == nullptr: 1),
// to one partial per parameter at ws[(tile row * gridDim.x + tile column) * n_theta + k]: [ln a, (RQ: ln kappa,) ln l_1..d].
// The pair tile of pair_tile.h: the two 64-point panels staged in LDS (2 x d x 64 doubles of dynamic LDS: 64 KiB at
// d = 64), a 4 x 4 block per thread, s by pair_tile::accumulate_s - the builders' s - then value and derivative profiles
// in two halves of eight elements (kfun.h: kprofiles) and one pass over the dimensions for the length scales.
// square != 0: U and V are the same points (the K_mm term) and the diagonal carries diag_eps: d(K + eps I)_ii / d ln a =
// 2 (a^2 + eps).  Reads Mw only where i < nu and j < nv; VALU-bound (the fp64 exp and the d-term sums).
// BATCHED: a lockstep batch in blockIdx.z - problem z takes its parameters from pdev[z] (p_one is not read), diag_eps =
// jitter a_z^2 (diag_eps carries the relative jitter), and its weights, vectors and partials `z * stride` behind the
// pointers (ContractStrides); U and V are shared.  The tile's arithmetic is the same code either way.
struct ContractStrides {
  int64_t mw, rs, u, v, ws;
};

template <int KERNEL, bool BATCHED>
__global__ __launch_bounds__(SGP_NT) void sgp_contract_kernel(KParams p_one, const KParams* __restrict__ pdev,
                                                              const double* __restrict__ U, int64_t nu,
                                                              const double* __restrict__ V, int64_t nv,
                                                              const double* __restrict__ Mw, int64_t ld,
                                                              const double* __restrict__ rs, const double* __restrict__ uvec,
                                                              const double* __restrict__ vvec, double m_scale,
                                                              double uv_scale, int square, double diag_eps, int n_theta,
                                                              double* __restrict__ ws, ContractStrides st) {
  extern __shared__ double sc_lds[];
  __shared__ double red[4];
  const KParams& p = BATCHED ? pdev[blockIdx.z] : p_one;
  if (BATCHED) {
    const int64_t z = blockIdx.z;
    diag_eps = __dmul_rn(diag_eps, p.a2);  // (rounded on its own, as the host's product is)
    Mw += z * st.mw;
    if (rs) rs += z * st.rs;
    uvec += z * st.u;
    vvec += z * st.v;
    ws += z * st.ws;
  }
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int tid = threadIdx.x, d = p.d;
  double* su = sc_lds;
  double* sv = sc_lds + d * KT;
  const int64_t i0 = (int64_t)ti * KT, j0 = (int64_t)tj * KT;
  pair_tile::stage_panels(su, U, i0, nu, sv, V, j0, nv, d);
  __syncthreads();
  const int ty = pair_tile::thread_row(tid), tx = pair_tile::thread_col(tid);
  double s[4][4], w[4][4];
  pair_tile::accumulate_s(p.inv_l2, d, su, sv, ty, tx, s);
  pair_weights(i0 + ty * 4, nu, j0 + tx * 4, nv, Mw, ld, rs, m_scale, uvec, uv_scale, vvec, w);
  double g_amp = 0.0, g_shape = 0.0;
  // The two halves of eight are written out here, not through pair_tile::for_each_profile: behind the helper, with the
  // element's work in a callback of any shape tried, the Matern32 instantiation took 132 VGPRs (three waves per SIMD)
  // against 114 (four) in this form.
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double s8[8], C8[8], g8[8], h8[8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) s8[4 * r + c] = s[2 * h + r][c];
    kprofiles<KERNEL>(p, s8, C8, g8, h8);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t gi = i0 + ty * 4 + 2 * h + r, gj = j0 + tx * 4 + c;
        const double wv = w[2 * h + r][c];
        double K = p.a2 * C8[4 * r + c];
        if (square && gi == gj) K += diag_eps;
        g_amp = fma(wv, 2.0 * K, g_amp);                            // dK/d ln a = 2 K
        if (KERNEL == GPMI_KERNEL_RQ) g_shape = fma(wv, p.a2 * h8[4 * r + c], g_shape);
        w[2 * h + r][c] = wv * (p.a2 * g8[4 * r + c]);              // times dx_k^2 / l_k^2: dK/d ln l_k
      }
  }
  double* out = ws + ((int64_t)ti * gridDim.x + tj) * n_theta;
  const int off = (KERNEL == GPMI_KERNEL_RQ) ? 2 : 1;
  double v = block_sum(g_amp, red);
  if (tid == 0) out[0] = v;
  if (KERNEL == GPMI_KERNEL_RQ) {
    v = block_sum(g_shape, red);
    if (tid == 0) out[1] = v;
  }
  for (int k = 0; k < d; ++k) {
    const double il2 = p.inv_l2[k];
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double dx = su[k * KT + ty * 4 + r] - sv[k * KT + tx * 4 + c];
        acc = fma(w[r][c], dx * dx * il2, acc);
      }
    v = block_sum(acc, red);
    if (tid == 0) out[off + k] = v;
  }
}

size_t contract_lds_bytes(int d) { return sizeof(double) * 2 * (size_t)d * KT; }

// tiles (ceil(nu_padded / 64) x ceil(nv_padded / 64)) of partials into ws
void launch_contract(hipStream_t s, const KParams& p, const double* U, int64_t nu, int64_t nup, const double* V, int64_t nv,
                     int64_t nvp, const double* Mw, int64_t ld, const double* rs, const double* uvec, const double* vvec,
                     double m_scale, double uv_scale, int square, double diag_eps, int n_theta, double* ws) {
  const dim3 grid((unsigned)(nvp / KT), (unsigned)(nup / KT));
  const size_t lds = contract_lds_bytes(p.d);
  with_stationary_kernel(p.kernel, [&](auto K) {  // (sgp_params admits no other kind)
    hipLaunchKernelGGL((sgp_contract_kernel<decltype(K)::value, false>), grid, dim3(SGP_NT), lds, s, p, nullptr, U, nu, V, nv, Mw,
                       ld, rs, uvec, vvec, m_scale, uv_scale, square, diag_eps, n_theta, ws, ContractStrides{});
  });
}

// the same for the B problems of a lockstep chunk (pdev[z], all of kind `kernel` in d dimensions; jitter_rel: the diagonal
// of the square form carries jitter_rel a_z^2)
void launch_contract_batched(hipStream_t s, int kernel, int d, const KParams* pdev, int B, const double* U, int64_t nu, int64_t nup,
                             const double* V, int64_t nv, int64_t nvp, const double* Mw, int64_t ld, const double* rs,
                             const double* uvec, const double* vvec, double m_scale, double uv_scale, int square,
                             double jitter_rel, int n_theta, double* ws, const ContractStrides& st) {
  const dim3 grid((unsigned)(nvp / KT), (unsigned)(nup / KT), (unsigned)B);
  const size_t lds = contract_lds_bytes(d);
  with_stationary_kernel(kernel, [&](auto K) {
    hipLaunchKernelGGL((sgp_contract_kernel<decltype(K)::value, true>), grid, dim3(SGP_NT), lds, s, KParams{}, pdev, U, nu, V, nv,
                       Mw, ld, rs, uvec, vvec, m_scale, uv_scale, square, jitter_rel, n_theta, ws, st);
  });
}

// A kernel launched with `lds` bytes of dynamic LDS: above 64 KiB a kernel has to opt in first
template <class... KA>
int launch_large_lds(gpmi_ctx* c, hipStream_t s, void (*kernel)(KA...), dim3 grid, size_t lds, std::common_type_t<KA>... args) {
  if (lds > 65536)
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(SGP_NT), lds, s, args...);
  return GPMI_OK;
}

// The contraction by the inducing inputs: for the 64 points v_j of tile blockIdx.x (the inducing inputs differentiated) and
// the run blockIdx.y of `run_tiles` consecutive 64-row tiles of U (the points summed over),
//   zws[(run * nvp + j) * d + k] = scale / l_k^2 * sum_i w_ij a^2 g(s(u_i, v_j)) (v_jk - u_ik),
//   w_ij = rs_i Mw[i][j] + uvec_i vvec_j   (rs == nullptr: 1),
// the operands and the weights of sgp_contract_kernel (pair_weights).  dK(u_i, v_j) / dv_jk = -a^2 g (v_jk - u_ik) / l_k^2.
// The column panel is staged once, the row panel once per tile of the run; s and the profiles are recomputed per tile
// (pair_tile.h), and the weighted differences are summed over the rows by pair_tile::reduce_columns with one weight
// array: four dimensions per barrier into a [d][64] accumulator in LDS.  Tiles are added in ascending order, rows >= nu
// and columns >= nv carry weight 0.  The order of every sum is fixed by the shapes and run_tiles alone.
// Dynamic LDS (pair_tile::column_lds_bytes): (3 d + 32) x 64 doubles - 112 KiB at d = 64, 28 KiB at d = 8.  gfx950
// (kernel-resource-usage; the state is independent of d), SE / RQ / Matern32 / Matern52: 124 / 157 / 127 / 139 VGPRs, no
// AGPRs, scratch 0, no static LDS: 114688 bytes of LDS at d = 64 (one workgroup per CU there, five at d = 8).
constexpr int ZRUN_MAX = 16;

template <int KERNEL>
__global__ __launch_bounds__(SGP_NT) void sgp_zcontract_kernel(KParams p, const double* __restrict__ U, int64_t nu,
                                                               const double* __restrict__ V, int64_t nv, int64_t nvp,
                                                               const double* __restrict__ Mw, int64_t ld,
                                                               const double* __restrict__ rs, const double* __restrict__ uvec,
                                                               const double* __restrict__ vvec, double scale, int run_tiles,
                                                               double* __restrict__ zws) {
  extern __shared__ double sz_lds[];
  const int tj = blockIdx.x, run = blockIdx.y;
  const int tid = threadIdx.x, d = p.d;
  double* sv = sz_lds;
  double* su = sv + d * KT;
  double* const acc[1] = {su + d * KT};
  double* red = acc[0] + d * KT;
  const int64_t j0 = (int64_t)tj * KT;
  pair_tile::for_each_coordinate(d, [&](int idx, int pt, int k) {
    pair_tile::stage_coordinate(sv, V, j0, nv, d, pt, k);
    acc[0][idx] = 0.0;
  });
  const int ty = pair_tile::thread_row(tid), tx = pair_tile::thread_col(tid);
  int chunk = 0;
  for (int t = 0; t < run_tiles; ++t) {
    const int64_t i0 = ((int64_t)run * run_tiles + t) * KT;
    if (i0 >= nu) break;
    __syncthreads();  // (the previous tile's readers of su)
    pair_tile::stage_panel(su, U, i0, nu, d);
    __syncthreads();
    double s[4][4], w[1][4][4];
    pair_tile::accumulate_s(p.inv_l2, d, su, sv, ty, tx, s);
    pair_weights(i0 + ty * 4, nu, j0 + tx * 4, nv, Mw, ld, rs, 1.0, uvec, 1.0, vvec, w[0]);
    pair_tile::for_each_profile<KERNEL, true>(p, s, [&](int r, int c, double, double g, double) { w[0][r][c] *= p.a2 * g; });
    pair_tile::reduce_columns<1>(su, sv, d, ty, tx, w, 1, acc, red, chunk);
  }
  __syncthreads();
  pair_tile::write_columns<1>(p.inv_l2, d, acc, 1, {scale}, (int64_t)run * nvp + j0, {zws});
}

// zacc[e] (+)= sum_run zws[run * count + e], runs in ascending order; e < count
__global__ __launch_bounds__(SGP_NT) void sgp_zsum_kernel(const double* __restrict__ zws, int nruns, int64_t count,
                                                          double* __restrict__ zacc, int accumulate) {
  const int64_t e = (int64_t)blockIdx.x * SGP_NT + threadIdx.x;
  if (e >= count) return;
  double v = 0.0;
  for (int r = 0; r < nruns; ++r) v += zws[(int64_t)r * count + e];
  zacc[e] = accumulate ? zacc[e] + v : v;
}

// tiles of U per workgroup: ZRUN_MAX, halved (not below 2) while the grid stays under 512 workgroups - a function of the
// two padded shapes alone
int zrun_tiles(int64_t nup, int64_t nvp) {
  int r = ZRUN_MAX;
  while (r > 2 && (nvp / KT) * ((nup / KT + r - 1) / r) < 512) r >>= 1;
  return r;
}

int zruns(int64_t nup, int64_t nvp) {
  const int r = zrun_tiles(nup, nvp);
  return (int)((nup / KT + r - 1) / r);
}

// zacc (nvp x d) (+)= the contraction over the rows of U; zws holds zruns(nup, nvp) x nvp x d doubles
int launch_zcontract(gpmi_ctx* c, hipStream_t s, const KParams& p, const double* U, int64_t nu, int64_t nup, const double* V,
                     int64_t nv, int64_t nvp, const double* Mw, int64_t ld, const double* rs, const double* uvec,
                     const double* vvec, double scale, double* zws, double* zacc, int accumulate) {
  const int run_tiles = zrun_tiles(nup, nvp), nruns = zruns(nup, nvp);
  const dim3 grid((unsigned)(nvp / KT), (unsigned)nruns);
  int rc = GPMI_OK;
  with_stationary_kernel(p.kernel, [&](auto K) {  // (sgp_params admits no other kind)
    rc = launch_large_lds(c, s, sgp_zcontract_kernel<decltype(K)::value>, grid, pair_tile::column_lds_bytes(p.d, 1), p, U, nu, V,
                          nv, nvp, Mw, ld, rs, uvec, vvec, scale, run_tiles, zws);
  });
  if (rc) return rc;
  const int64_t count = nvp * p.d;
  hipLaunchKernelGGL(sgp_zsum_kernel, dim3((unsigned)((count + SGP_NT - 1) / SGP_NT)), dim3(SGP_NT), 0, s, zws, nruns, count,
                     zacc, accumulate);
  HIPCHK(c, hipGetLastError());
  return GPMI_OK;
}

// The derivatives of the predictive mean and variance by the query point: for the 64 query points q_j of tile blockIdx.x and
// the run blockIdx.y of QRUN_TILES consecutive 64-row tiles of the inducing inputs z_a,
//   ws_mean[(run * nqp + j) * d + k] = -1 / l_k^2 * sum_a gamma_a  a^2 g(s(z_a, q_j)) (q_jk - z_ak),
//   ws_var [(run * nqp + j) * d + k] = -2 / l_k^2 * sum_a Tq[j][a] a^2 g(s(z_a, q_j)) (q_jk - z_ak)      (want_var != 0),
// with gamma = L^-T L_B^-T c (mean(q) = k_m(q)^T gamma) and the rows Tq[j] = t(q_j)^T = (L^-T (L_B^-T u(q_j) - v(q_j)))^T
// (var(q) = a^2 + k_m(q)^T t(q)) as the products leave them, query-major.  d k(q, z_a) / d q_k = -a^2 g (q_k - z_ak) / l_k^2:
// nothing is divided by a distance, a query point that is an inducing input gets an exact zero from it.
// The query panel is staged once, a tile of inducing inputs once per tile of the run; s and the profiles are recomputed
// per tile (pair_tile.h); the profile a^2 g is formed once and weighted twice, and pair_tile::reduce_columns sums the
// weighted differences with two weight arrays into two [d][64] accumulators in LDS: two dimensions of both outputs per
// barrier, or four of the mean alone - a slot's sum does not depend on which of the two forms ran.  Tiles are added in
// ascending order; rows >= m and columns >= nq carry weight 0.
// The order of every sum of column j is fixed by m alone: it does not depend on nq or on where q_j stands in the call.
// Dynamic LDS (pair_tile::column_lds_bytes): (4 d + 32) x 64 doubles - 147456 bytes (144 KiB of the CU's 160) at d = 64,
// one workgroup per CU there; 32 KiB at d = 8.  gfx950 (kernel-resource-usage; the state is independent of d), SE / RQ /
// Matern32 / Matern52: 128 / 170 / 128 / 128 VGPRs, no AGPRs, scratch 0, no static LDS.  VALU-bound (the fp64 exp), as
// the Z pass.
constexpr int QRUN_TILES = 2;

template <int KERNEL>
__global__ __launch_bounds__(SGP_NT) void sgp_qgrad_kernel(KParams p, const double* __restrict__ Z, int64_t m,
                                                           const double* __restrict__ Q, int64_t nq, int64_t nqp,
                                                           const double* __restrict__ gamma, const double* __restrict__ Tq,
                                                           int64_t ld, int want_var, double* __restrict__ ws_mean,
                                                           double* __restrict__ ws_var) {
  extern __shared__ double sq_lds[];
  const int tj = blockIdx.x, run = blockIdx.y;
  const int tid = threadIdx.x, d = p.d;
  double* sv = sq_lds;            // the query points
  double* su = sv + d * KT;       // a tile of inducing inputs
  double* const acc[2] = {su + d * KT, su + 2 * d * KT};  // the mean's, the variance's
  double* red = acc[1] + d * KT;
  const int64_t j0 = (int64_t)tj * KT;
  pair_tile::for_each_coordinate(d, [&](int idx, int pt, int k) {
    pair_tile::stage_coordinate(sv, Q, j0, nq, d, pt, k);
    acc[0][idx] = 0.0;
    acc[1][idx] = 0.0;
  });
  const int ty = pair_tile::thread_row(tid), tx = pair_tile::thread_col(tid);
  const int nw = want_var ? 2 : 1;
  int chunk = 0;
  for (int t = 0; t < QRUN_TILES; ++t) {
    const int64_t i0 = ((int64_t)run * QRUN_TILES + t) * KT;
    if (i0 >= m) break;
    __syncthreads();  // (the previous tile's readers of su)
    pair_tile::stage_panel(su, Z, i0, m, d);
    __syncthreads();
    double w[2][4][4];  // w[0]: s, then the profile times gamma; w[1]: the profile times t(q)
    pair_tile::accumulate_s(p.inv_l2, d, su, sv, ty, tx, w[0]);
    double ga[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ga[r] = (i0 + ty * 4 + r < m) ? gamma[i0 + ty * 4 + r] : 0.0;
    pair_tile::for_each_profile<KERNEL, true>(p, w[0], [&](int r, int c, double, double g, double) {
      const int64_t gi = i0 + ty * 4 + r, gj = j0 + tx * 4 + c;
      const bool ok = gi < m && gj < nq;
      const double pg = ok ? p.a2 * g : 0.0;
      w[0][r][c] = pg * ga[r];
      w[1][r][c] = (want_var && ok) ? pg * Tq[gj * ld + gi] : 0.0;
    });
    pair_tile::reduce_columns<2>(su, sv, d, ty, tx, w, nw, acc, red, chunk);
  }
  __syncthreads();
  pair_tile::write_columns<2>(p.inv_l2, d, acc, nw, {-1.0, -2.0}, (int64_t)run * nqp + j0, {ws_mean, ws_var});
}

// runs of inducing tiles per query tile: a function of m alone
int qruns(int64_t mp) { return (int)((mp / KT + QRUN_TILES - 1) / QRUN_TILES); }

// out_mean, out_var (nqp x d each; out_var only if want_var) = the derivatives at the nq points Q; ws_mean and ws_var hold
// qruns(mp) x nqp x d doubles each
int launch_qgrad(gpmi_ctx* c, hipStream_t s, const KParams& p, const double* Z, int64_t m, int64_t mp, const double* Q, int64_t nq,
                 int64_t nqp, const double* gamma, const double* Tq, int64_t ld, bool want_var, double* ws_mean, double* ws_var,
                 double* out_mean, double* out_var) {
  const int nruns = qruns(mp);
  const dim3 grid((unsigned)(nqp / KT), (unsigned)nruns);
  int rc = GPMI_OK;
  with_stationary_kernel(p.kernel, [&](auto K) {  // (sgp_params admits no other kind)
    rc = launch_large_lds(c, s, sgp_qgrad_kernel<decltype(K)::value>, grid, pair_tile::column_lds_bytes(p.d, 2), p, Z, m, Q, nq,
                          nqp, gamma, Tq, ld, want_var ? 1 : 0, ws_mean, ws_var);
  });
  if (rc) return rc;
  const int64_t count = nqp * p.d;
  const dim3 sgrid((unsigned)((count + SGP_NT - 1) / SGP_NT));
  hipLaunchKernelGGL(sgp_zsum_kernel, sgrid, dim3(SGP_NT), 0, s, ws_mean, nruns, count, out_mean, 0);
  if (want_var) hipLaunchKernelGGL(sgp_zsum_kernel, sgrid, dim3(SGP_NT), 0, s, ws_var, nruns, count, out_var, 0);
  HIPCHK(c, hipGetLastError());
  return GPMI_OK;
}

unsigned blocks(int64_t n) { return (unsigned)((n + SGP_NT - 1) / SGP_NT); }

// workgroups of sgp_weights_kernel: one element per thread up to SGP_RED_BLOCKS workgroups, a grid-stride loop beyond
unsigned weights_blocks(int64_t n) { return (unsigned)std::min<int64_t>(SGP_RED_BLOCKS, (n + SGP_NT - 1) / SGP_NT); }

// the ranges gpmi_sgp_create, sgp_params and gpmi_sgp_schedule share
bool sgp_n_ok(int64_t n) { return n >= 2 && n <= ((int64_t)1 << 30); }
bool sgp_m_ok(int64_t m) { return m >= 1 && m <= GPMI_SGP_MAX_M; }
bool sgp_panel_ok(int64_t panel_rows) { return panel_rows >= 0 && panel_rows <= SGP_MAX_PANEL; }

bool sgp_live(gpmi_ctx* c, gpmi_sgp* g) {
  return std::find(c->sgp_live.begin(), c->sgp_live.end(), g) != c->sgp_live.end();
}

int sgp_params(gpmi_sgp* g, int kernel, const double* theta, int n_theta, double white, double jitter, int64_t panel_rows,
               KParams& p) {
  gpmi_ctx* c = g->ctx;
  ARGCHK(c, g->have_targets, "gpmi_sgp: gpmi_sgp_set_targets has not been called");
  ARGCHK(c, kernel != GPMI_KERNEL_SUM && kernel_is_stationary(kernel),
         "gpmi_sgp: the kernel must be GPMI_KERNEL_SE, _RQ, _M32 or _M52");
  const int off = kernel_theta_offset(kernel);
  ARGCHK(c, theta != nullptr, "gpmi_sgp: theta is NULL");
  ARGCHK(c, n_theta == g->d + off, "gpmi_sgp: n_theta does not match the kernel and the data dimension");
  for (int k = 0; k < n_theta; ++k) ARGCHK(c, std::isfinite(theta[k]), "gpmi_sgp: theta must be finite");
  ARGCHK(c, std::isfinite(white) && white >= 0.0, "gpmi_sgp: white_var must be finite and not negative");
  ARGCHK(c, std::isfinite(jitter) && jitter >= 0.0, "gpmi_sgp: jitter_rel must be finite and not negative");
  ARGCHK(c, sgp_panel_ok(panel_rows), "gpmi_sgp: panel_rows out of range (0 .. 32768)");
  std::memset(&p, 0, sizeof(p));
  p.kernel = kernel;
  p.d = (int)g->d;
  const double a = std::exp(theta[0]);
  p.a2 = a * a;
  p.kappa = (kernel == GPMI_KERNEL_RQ) ? std::exp(theta[1]) : 1.0;
  for (int k = 0; k < p.d; ++k) {
    const double l = std::exp(theta[off + k]);
    p.inv_l2[k] = 1.0 / (l * l);
  }
  return GPMI_OK;
}

// rows of x per panel of the two passes: the caller's panel_rows (0: GPMI_SGP_PANEL) in whole tiles, at most all of x
int64_t sgp_panel_rows(int64_t n, int64_t panel_rows) {
  return std::min<int64_t>(round_up(panel_rows > 0 ? panel_rows : GPMI_SGP_PANEL, GPMI_NB), round_up(n, GPMI_NB));
}
int64_t sgp_panel_rows(const gpmi_sgp* g, int64_t panel_rows) { return sgp_panel_rows(g->n, panel_rows); }

// panels for R rows (a multiple of 128)
int sgp_ensure_panels(gpmi_sgp* g, int64_t R) {
  gpmi_ctx* c = g->ctx;
  if (R <= g->panel_cap) return GPMI_OK;
  g->panel_cap = 0;
  for (DevBuf<double>* q : {&g->P[0], &g->P[1], &g->P[2], &g->pvec, &g->ws}) q->release();
  const int64_t each = std::max(g->mp * (R + 32), R * g->ld);
  for (int k = 0; k < 3; ++k)
    if (int rc = g->P[k].alloc(c, each)) return rc;
  if (int rc = g->pvec.alloc(c, 3 * R)) return rc;
  const int64_t tiles = (std::max(R, g->mp) / KT) * (g->mp / KT);
  if (int rc = g->ws.alloc(c, tiles * (GPMI_MAX_D + 2))) return rc;
  g->panel_cap = R;
  return GPMI_OK;
}

// the workspace of the Z pass for panels of R rows
int sgp_ensure_zws(gpmi_sgp* g, int64_t R) {
  gpmi_ctx* c = g->ctx;
  if (!g->zacc)
    if (int rc = g->zacc.alloc(c, g->mp * g->d)) return rc;
  return g->zws.reserve(c, (int64_t)std::max(zruns(R, g->mp), zruns(g->mp, g->mp)) * g->mp * g->d);
}

// names of the work matrices: G, A (K_mm -> L; later T), LiT (L^-T), Linv, W1 (L^-1 G; later L^-T L_B^-T), W2 (H; later S,
// then K_mm^-1 G K_mm^-1), LB (B -> L_B; later K_mm^-1 G, then the K_mm weights), W3 (L_B^-T; later K_mm^-1), LBinv
enum { MG = 0, MA, MLIT, MLINV, MW1, MW2, MLB, MW3, MLBINV };

void nt_square(hipStream_t s, double* C, const double* A, const double* B, int64_t mp, int64_t ld) {
  const int nt = (int)(mp / GPMI_NB);
  launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, C, ld, A, ld, B, ld, nt, nt, (int)mp);  // C = A B^T
}

// dst <- (factor at A)^-1, through its transpose in `scratch`
void inverse_factor(hipStream_t s, const double* A, const double* invD, double* scratch, double* dst, int64_t mp, int64_t ld) {
  trsm_identity_batched(s, A, mp, ld, invD, scratch, BatchShape());
  hipLaunchKernelGGL(sgp_transpose_kernel, dim3((unsigned)(mp / KT), (unsigned)(mp / KT)), dim3(SGP_NT), 0, s, scratch, dst, ld, 0);
}

int read_info(gpmi_sgp* g, int slot, int& inf) {
  gpmi_ctx* c = g->ctx;
  HIPCHK(c, hipMemcpyAsync(&inf, g->info + slot, sizeof(int), hipMemcpyDeviceToHost, c->sgp_stream));
  HIPCHK(c, hipStreamSynchronize(c->sgp_stream));
  return GPMI_OK;
}

// Pass 1 and the m x m algebra.  info = 0: M[MLINV], M[MLBINV], M[MLIT], M[MW3] (L_B^-T), vec (b, L^-1 b, c) and *F are valid.
int sgp_factor(gpmi_sgp* g, const KParams& p, double white, double jitter, int64_t panel_rows, double* F, double* sum_w,
               int* info) {
  gpmi_ctx* c = g->ctx;
  hipStream_t s = c->sgp_stream;
  const int64_t n = g->n, m = g->m, mp = g->mp, ld = g->ld, d = g->d;
  const int nt = (int)(mp / GPMI_NB);
  const int64_t P = sgp_panel_rows(g, panel_rows);
  const int64_t ldp = P + 32;
  if (int rc = sgp_ensure_panels(g, P)) return rc;
  double *G = g->M[MG], *A = g->M[MA], *LiT = g->M[MLIT], *Linv = g->M[MLINV], *W1 = g->M[MW1], *W2 = g->M[MW2],
         *LB = g->M[MLB], *W3 = g->M[MW3], *LBinv = g->M[MLBINV];
  double *b = g->vec, *v1 = g->vec + mp, *cc = g->vec + 2 * mp;
  double hred[4] = {};
  {
    const unsigned nblk = weights_blocks(n);
    hipLaunchKernelGGL(sgp_weights_kernel, dim3(nblk), dim3(SGP_NT), 0, s, g->r, g->nv, white, nullptr, n, g->w, g->part, 0, 0);
    hipLaunchKernelGGL(sgp_colsum_kernel, dim3(4), dim3(SGP_NT), 0, s, g->part, (int64_t)nblk, 4, g->red + RED_DATA, 0, 0, 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hred, g->red + RED_DATA, sizeof(hred), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    ARGCHK(c, hred[3] == 0.0, "gpmi_sgp: noise_var_i + white_var must be positive and finite for every data point");
  }
  HIPCHK(c, hipMemsetAsync(G, 0, sizeof(double) * mp * ld, s));
  HIPCHK(c, hipMemsetAsync(g->vec, 0, sizeof(double) * 4 * mp, s));
  for (int64_t j0 = 0; j0 < n; j0 += P) {
    const int64_t rows = std::min<int64_t>(P, n - j0);
    double* Kp = g->P[0];
    {
      ProfScope ps(c, s, GPMI_PROF_SGP_BUILD, 0.0, 8.0 * mp * P);
      launch_kbuild_cross(s, p, g->z, m, mp, g->x + j0 * d, rows, P, Kp, ldp);  // (zeros in rows >= m and columns >= rows)
      hipLaunchKernelGGL(sgp_scale_cols_kernel, dim3(blocks(rows), (unsigned)m), dim3(SGP_NT), 0, s, Kp, ldp, rows, g->w + j0, 0, 0);
      hipLaunchKernelGGL(sgp_bvec_kernel, dim3((unsigned)m), dim3(SGP_NT), 0, s, Kp, ldp, rows, g->r + j0, g->w + j0, b,
                         j0 > 0 ? 1 : 0, 0, 0, 0);
    }
    {
      ProfScope ps(c, s, GPMI_PROF_SGP_GRAM, (double)P * mp * (mp + GPMI_NB), 8.0 * (mp * P + 0.5 * mp * mp));
      launch_gemm_nt(s, TILES_LOWER, OP_SUB, G, ld, Kp, ldp, Kp, ldp, nt, nt, (int)P);  // G holds -G until the sweep is over
    }
    HIPCHK(c, hipGetLastError());
  }
  int inf = 0;
  {
    ProfScope ps(c, s, GPMI_PROF_SGP_FACTOR, 2.0 * mp * mp * mp / 3.0 + 8.0 * mp * mp * mp, 8.0 * 12.0 * mp * mp);
    launch_mirror_lower(s, G, ld, mp);
    launch_negate(s, G, mp * ld);
    launch_kbuild_cross(s, p, g->z, m, mp, g->z, m, mp, A, ld);
    hipLaunchKernelGGL(sgp_pad_diag_kernel, dim3(blocks(mp)), dim3(SGP_NT), 0, s, A, ld, m, mp, jitter * p.a2, 0.0, nullptr, 0);
    HIPCHK(c, hipMemsetAsync(g->info, 0, 2 * sizeof(int), s));
    potrf_lower_batched(c, s, A, mp, ld, g->invD1, g->info, BatchShape());
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = read_info(g, 0, inf)) return rc;
  if (inf != 0) {
    *info = inf;
    return GPMI_OK;
  }
  {
    ProfScope ps(c, s, GPMI_PROF_SGP_FACTOR, 0.0, 0.0);
    inverse_factor(s, A, g->invD1, LiT, Linv, mp, ld);
    nt_square(s, W1, Linv, G, mp, ld);   // L^-1 G   (G symmetric)
    nt_square(s, W2, W1, Linv, mp, ld);  // H = L^-1 G L^-T
    hipLaunchKernelGGL(sgp_sym_b_kernel, dim3((unsigned)(mp / KT), (unsigned)(mp / KT)), dim3(SGP_NT), 0, s, W2, LB, ld, 0);
    potrf_lower_batched(c, s, LB, mp, ld, g->invD2, g->info + 1, BatchShape());
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = read_info(g, 1, inf)) return rc;
  if (inf != 0) {
    *info = (int)m + inf;
    return GPMI_OK;
  }
  double hmm[3] = {};
  {
    ProfScope ps(c, s, GPMI_PROF_SGP_FACTOR, 0.0, 0.0);
    inverse_factor(s, LB, g->invD2, W3, LBinv, mp, ld);
    launch_rows_dot(s, Linv, ld, mp, mp, b, v1);
    launch_rows_dot(s, LBinv, ld, mp, mp, v1, cc);
    hipLaunchKernelGGL(sgp_mm_reduce_kernel, dim3(1), dim3(SGP_NT), 0, s, LB, W2, ld, m, cc, g->red + RED_MM, 0, 0, 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hmm, g->red + RED_MM, sizeof(hmm), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  const double LN_2PI = 1.8378770664093454836;
  *F = -0.5 * ((double)n * LN_2PI + hred[1] + 2.0 * hmm[0] + hred[0] - hmm[2]) - 0.5 * (p.a2 * hred[2] - hmm[1]);
  *sum_w = hred[2];
  *info = 0;
  return GPMI_OK;
}

// The gradient behind a successful sgp_factor (same parameters): grad (n_theta + 1) if not NULL, alpha into g->alpha.
// want_z (needs grad): dF/dZ into g->zacc (m x d in its first rows) from the operands of every contraction, behind it.
int sgp_gradient(gpmi_sgp* g, const KParams& p, int n_theta, double white, double jitter, int64_t panel_rows, double sum_w,
                 double* grad, bool want_z = false) {
  gpmi_ctx* c = g->ctx;
  hipStream_t s = c->sgp_stream;
  const int64_t n = g->n, m = g->m, mp = g->mp, ld = g->ld, d = g->d;
  const int nt = (int)(mp / GPMI_NB);
  const int64_t P = sgp_panel_rows(g, panel_rows);
  double *G = g->M[MG], *T = g->M[MA], *LiT = g->M[MLIT], *RT = g->M[MW1], *W2 = g->M[MW2], *LB = g->M[MLB], *Kinv = g->M[MW3],
         *LBinv = g->M[MLBINV];
  double *cc = g->vec + 2 * mp, *gamma = g->vec + 3 * mp;
  double *kg = g->pvec, *q = g->pvec + P, *term = g->pvec + 2 * P;
  if (want_z)
    if (int rc = sgp_ensure_zws(g, P)) return rc;
  ProfScope ps(c, s, GPMI_PROF_SGP_GRAD, 0.0, 0.0);
  nt_square(s, RT, LiT, LBinv, mp, ld);  // L^-T L_B^-T
  launch_rows_dot(s, RT, ld, mp, mp, cc, gamma);
  if (grad) {
    nt_square(s, W2, RT, RT, mp, ld);      // S = L^-T B^-1 L^-1
    nt_square(s, Kinv, LiT, LiT, mp, ld);  // L^-T L^-1
    hipLaunchKernelGGL(sgp_sub_kernel, dim3(blocks(mp), (unsigned)mp), dim3(SGP_NT), 0, s, Kinv, W2, T, ld, mp, 0);
    nt_square(s, LB, Kinv, G, mp, ld);     // K_mm^-1 G
    nt_square(s, W2, LB, Kinv, mp, ld);    // K_mm^-1 G K_mm^-1
    hipLaunchKernelGGL(sgp_sub_kernel, dim3(blocks(mp), (unsigned)mp), dim3(SGP_NT), 0, s, W2, T, LB, ld, mp,
                       0);  // M2 - gamma gamma^T
  }
  HIPCHK(c, hipGetLastError());
  for (int64_t j0 = 0; j0 < n; j0 += P) {
    const int64_t rows = std::min<int64_t>(P, n - j0);
    double *KTp = g->P[0], *Mp = g->P[1];
    launch_kbuild_cross(s, p, g->x + j0 * d, rows, P, g->z, m, mp, KTp, ld);  // P x mp: row j = k_m(x_j)
    launch_rows_dot(s, KTp, ld, P, mp, gamma, kg);
    if (grad) {
      launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, Mp, ld, KTp, ld, T, ld, (int)(P / GPMI_NB), nt, (int)mp);  // rows k_j^T T
      hipLaunchKernelGGL(sgp_rowdot2_kernel, dim3((unsigned)rows), dim3(SGP_NT), 0, s, KTp, Mp, ld, m, q, 0, 0);
    }
    hipLaunchKernelGGL(sgp_alpha_kernel, dim3(blocks(rows)), dim3(SGP_NT), 0, s, g->r + j0, g->w + j0, kg,
                       grad ? q : (const double*)nullptr, p.a2, nullptr, rows, g->alpha + j0, term, 0, 0);
    if (grad) {
      hipLaunchKernelGGL(sgp_colsum_kernel, dim3(1), dim3(SGP_NT), 0, s, term, rows, 1, g->red + RED_NOISE, j0 > 0 ? 1 : 0, 0, 0);
      launch_contract(s, p, g->x + j0 * d, rows, P, g->z, m, mp, Mp, ld, g->w + j0, g->alpha + j0, gamma, 1.0, 1.0, 0, 0.0,
                      n_theta, g->ws);
      hipLaunchKernelGGL(sgp_colsum_kernel, dim3((unsigned)n_theta), dim3(SGP_NT), 0, s, g->ws, (P / KT) * (mp / KT), n_theta,
                         g->red + RED_GRAD, j0 > 0 ? 1 : 0, 0, 0);
      if (want_z)  // -sum_j M1_ij a^2 g (z_ik - x_jk) / l_k^2
        if (int rc = launch_zcontract(c, s, p, g->x + j0 * d, rows, P, g->z, m, mp, Mp, ld, g->w + j0, g->alpha + j0, gamma,
                                      -1.0, g->zws, g->zacc, j0 > 0 ? 1 : 0))
          return rc;
    }
    HIPCHK(c, hipGetLastError());
  }
  if (!grad) return GPMI_OK;
  // the K_mm term: weights -1/2 M2 = -1/2 (gamma gamma^T + LB), rows and columns are Z
  launch_contract(s, p, g->z, m, mp, g->z, m, mp, LB, ld, nullptr, gamma, gamma, -0.5, -0.5, 1, jitter * p.a2, n_theta, g->ws);
  hipLaunchKernelGGL(sgp_colsum_kernel, dim3((unsigned)n_theta), dim3(SGP_NT), 0, s, g->ws, (mp / KT) * (mp / KT), n_theta,
                     g->red + RED_GRAD, 1, 0, 0);
  if (want_z)  // +sum_j M2_ij a^2 g (z_ik - z_jk) / l_k^2: z_i is in row i and column i of K_mm, M2 symmetric - no 1/2
    if (int rc = launch_zcontract(c, s, p, g->z, m, mp, g->z, m, mp, LB, ld, nullptr, gamma, gamma, 1.0, g->zws, g->zacc, 1))
      return rc;
  HIPCHK(c, hipGetLastError());
  double hg[GPMI_MAX_D + 2] = {}, hnoise = 0.0;
  HIPCHK(c, hipMemcpyAsync(hg, g->red + RED_GRAD, sizeof(double) * n_theta, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(&hnoise, g->red + RED_NOISE, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (int k = 0; k < n_theta; ++k) grad[k] = hg[k];
  grad[0] -= p.a2 * sum_w;  // -1/2 sum w_i da^2 / d ln a
  grad[n_theta] = white > 0.0 ? white * hnoise : 0.0;
  return GPMI_OK;
}

// the noise variances go up: their range as the host sees it (gpmi_sgp_bound_batch checks noise_var_i + white_var with it)
int sgp_upload_noise(gpmi_sgp* g, const double* noise_var) {
  gpmi_ctx* c = g->ctx;
  g->nv_lo = g->nv_hi = 0.0;
  g->nv_nan = false;
  if (!noise_var) {
    ZERO_SYNC(c, g->nv, sizeof(double) * g->n);
    return GPMI_OK;
  }
  HIPCHK(c, hipMemcpy(g->nv, noise_var, sizeof(double) * g->n, hipMemcpyHostToDevice));
  g->nv_lo = std::numeric_limits<double>::infinity();
  g->nv_hi = -g->nv_lo;
  for (int64_t i = 0; i < g->n; ++i) {
    g->nv_nan = g->nv_nan || std::isnan(noise_var[i]);
    g->nv_lo = std::min(g->nv_lo, noise_var[i]);
    g->nv_hi = std::max(g->nv_hi, noise_var[i]);
  }
  return GPMI_OK;
}

// c->err = who + what
int sgp_arg_error(gpmi_ctx* c, const char* who, const char* what) {
  c->err = std::string(who) + what;
  return GPMI_ERR_ARG;
}

// What the evaluations of the bound (gpmi_sgp_bound, gpmi_sgp_bound_zgrad, gpmi_sgp_fit: `who` in the messages) open with:
// the checks of the object and the results (want_z: grad_z is one of them), the kernel parameters, pass 1 and the m x m
// algebra.  *info != 0 behind GPMI_OK: a factorisation failed and nothing else is valid.
int sgp_begin(gpmi_sgp* g, const char* who, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
              int64_t panel_rows, const double* F, int* info, bool want_z, const double* grad_z, KParams& p, double& f,
              double& sum_w) {
  gpmi_ctx* c = g->ctx;
  if (!sgp_live(c, g)) return sgp_arg_error(c, who, ": not a live object of this handle");
  if (!F || !info) return sgp_arg_error(c, who, ": F and info must be non-NULL");
  if (want_z && !grad_z) return sgp_arg_error(c, who, ": grad_z is NULL");
  if (int rc = sgp_params(g, kernel, theta, n_theta, white_var, jitter_rel, panel_rows, p)) return rc;
  if (int rc = set_device(c)) return rc;
  int inf = 0;
  if (int rc = sgp_factor(g, p, white_var, jitter_rel, panel_rows, &f, &sum_w, &inf)) return rc;
  *info = inf;
  return GPMI_OK;
}

// gpmi_sgp_bound (want_z false, grad_z unused) and gpmi_sgp_bound_zgrad (want_z: the gradient always runs, dF/dZ to grad_z)
int sgp_bound(gpmi_sgp* g, const char* who, bool want_z, int kernel, const double* theta, int n_theta, double white_var,
              double jitter_rel, int64_t panel_rows, double* F, double* grad, double* grad_z, double* alpha_host, int* info) {
  KParams p;
  double f = 0.0, sum_w = 0.0;
  if (int rc = sgp_begin(g, who, kernel, theta, n_theta, white_var, jitter_rel, panel_rows, F, info, want_z, grad_z, p, f, sum_w))
    return rc;
  if (*info != 0) return GPMI_OK;
  gpmi_ctx* c = g->ctx;
  if (want_z || grad || alpha_host) {
    double gbuf[GPMI_MAX_D + 3];
    if (int rc = sgp_gradient(g, p, n_theta, white_var, jitter_rel, panel_rows, sum_w, (want_z || grad) ? gbuf : nullptr, want_z))
      return rc;
    if (alpha_host) HIPCHK(c, hipMemcpyAsync(alpha_host, g->alpha, sizeof(double) * g->n, hipMemcpyDeviceToHost, c->sgp_stream));
    if (want_z) HIPCHK(c, hipMemcpyAsync(grad_z, g->zacc, sizeof(double) * g->m * g->d, hipMemcpyDeviceToHost, c->sgp_stream));
    HIPCHK(c, hipStreamSynchronize(c->sgp_stream));
    if (grad) std::memcpy(grad, gbuf, sizeof(double) * (n_theta + 1));
  }
  *F = f;
  return GPMI_OK;
}

// What the queries of a fitted model open with (`who` in the messages).  bounded: mq <= GPMI_DRAWS_MAX_M, the calls that
// hold an mq x mq covariance.  proceed == false behind GPMI_OK: mq == 0, the call has nothing to do.
int sgp_query_args(gpmi_sgp* g, const char* who, int64_t mq, bool bounded, bool& proceed) {
  gpmi_ctx* c = g->ctx;
  proceed = false;
  if (!sgp_live(c, g)) return sgp_arg_error(c, who, ": not a live object of this handle");
  if (!g->fitted) return sgp_arg_error(c, who, " needs a successful gpmi_sgp_fit");
  if (bounded) {
    if (mq < 0 || mq > GPMI_DRAWS_MAX_M) return sgp_arg_error(c, who, ": mq out of range (0 .. 16384 = GPMI_DRAWS_MAX_M points)");
  } else if (mq < 0) {
    return sgp_arg_error(c, who, ": mq must not be negative");
  }
  proceed = mq > 0;
  return GPMI_OK;
}

// The query panel of the fitted model: K_qm of the `rows` points at pts_dev (rp rows: whole tiles) into Kq, then the rows
// v^T = (L^-1 k_q)^T into V and u^T = (L_B^-1 v)^T into U.  Kq may be U.
void sgp_query_panel(gpmi_sgp* g, hipStream_t s, const double* pts_dev, int64_t rows, int64_t rp, double* Kq, double* V,
                     double* U, const GemmBatch& gb = GemmBatch()) {
  const int64_t mp = g->mp, ld = g->ld;
  const int nt = (int)(mp / GPMI_NB), ntr = (int)(rp / GPMI_NB);
  launch_kbuild_cross(s, g->fp, pts_dev, rows, rp, g->z, g->m, mp, Kq, ld);
  launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, V, ld, Kq, ld, g->fLinv, ld, ntr, nt, (int)mp, nullptr, gb);
  launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, U, ld, V, ld, g->fLBinv, ld, ntr, nt, (int)mp, nullptr, gb);
}

// The device buffers of a posterior call at mq points: the points, V and U (two matrices of mpq x ld(m)), mu and, if asked
// for, Sigma (mpq x ldq).  (An error return may leave work on these in flight: hipFree waits for the device before it
// releases.)
struct PosteriorBufs {
  DevBuf<double> P, VU, mu, Sigma;
  int64_t mpq = 0, ldq = 0;
  int alloc(gpmi_sgp* g, int64_t mq, bool want_sigma) {
    gpmi_ctx* c = g->ctx;
    mpq = round_up(mq, GPMI_NB);
    ldq = mpq + 32;
    if (int rc = P.alloc(c, mpq * g->d)) return rc;
    if (int rc = VU.alloc(c, 2 * mpq * g->ld)) return rc;
    if (int rc = mu.alloc(c, mpq)) return rc;
    return want_sigma ? Sigma.alloc(c, mpq * ldq) : GPMI_OK;
  }
};

// mu (mq) and Sigma (lower tiles; the mean alone if b holds no Sigma) of the latent function at the mq points of the host,
// enqueued on the sparse stream
int sgp_posterior_sigma(gpmi_sgp* g, const double* pts, int64_t mq, PosteriorBufs& b) {
  gpmi_ctx* c = g->ctx;
  hipStream_t s = c->sgp_stream;
  const int64_t mp = g->mp, ld = g->ld, mpq = b.mpq, ldq = b.ldq;
  const int ntq = (int)(mpq / GPMI_NB);
  double *pts_dev = b.P, *V = b.VU, *U = V + mpq * ld, *Sigma = b.Sigma;
  HIPCHK(c, hipMemcpyAsync(pts_dev, pts, sizeof(double) * mq * g->d, hipMemcpyHostToDevice, s));
  sgp_query_panel(g, s, pts_dev, mq, mpq, U, V, U);  // (K_qm in the place U takes)
  launch_rows_dot(s, U, ld, mpq, mp, g->fc, b.mu);
  if (Sigma) {
    // Sigma = K_qq - V V^T + U U^T on the lower tiles; the product only subtracts, so the sign is turned in between
    launch_kbuild_cross(s, g->fp, pts_dev, mq, mpq, pts_dev, mq, mpq, Sigma, ldq);
    launch_gemm_nt(s, TILES_LOWER, OP_SUB, Sigma, ldq, V, ld, V, ld, ntq, ntq, (int)mp);
    launch_negate(s, Sigma, mpq * ldq);
    launch_gemm_nt(s, TILES_LOWER, OP_SUB, Sigma, ldq, U, ld, U, ld, ntq, ntq, (int)mp);
    launch_negate(s, Sigma, mpq * ldq);
  }
  HIPCHK(c, hipGetLastError());
  return GPMI_OK;
}


// ---- lockstep batches: T hyper-parameter vectors on one object (gpmi_sgp_bound_batch) ---------------------------------
// The launches of sgp_factor and sgp_gradient with a chunk of B problems in blockIdx.z of every one of them, on the batch
// workspace (gpmi_sgp::bw: B copies of the object's work arrays side by side).  The host is waited for once per chunk:
// a problem whose factorisation fails carries what it holds through the later launches - no index depends on a value -
// and is reported through its two info words.

constexpr int64_t SGP_BATCH_MAX = 1024;  // problems per chunk at most (blockIdx.z, and the tiles of one GEMM launch)
constexpr int RED_SALPHA = 12;           // sum_i alpha_i
constexpr int SGP_RED = 128;             // doubles of a problem's small results (gpmi_sgp::red)

// r_z = y - mu_const[z], or (mu_const == nullptr) y - r_z with the problem's mean function in r_z's place
__global__ __launch_bounds__(SGP_NT) void sgp_residual_kernel(const double* __restrict__ y, const double* __restrict__ mu_const,
                                                              int64_t n, double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * SGP_NT + threadIdx.x, z = blockIdx.z;
  if (i >= n) return;
  r[z * n + i] = y[i] - (mu_const ? mu_const[z] : r[z * n + i]);
}

// per workgroup the partial sum of its grid-strided share of v_z (n values; sgp_colsum_kernel adds the partials)
__global__ __launch_bounds__(SGP_NT) void sgp_vecsum_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ part,
                                                            int64_t sPart) {
  __shared__ double red[4];
  const int64_t z = blockIdx.z;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SGP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * SGP_NT) acc += v[z * n + i];
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) part[z * sPart + blockIdx.x] = t;
}

// The shape of a batch call: a function of its arguments alone (gpmi_sgp_batch_schedule reports it, gpmi_sgp_bound_batch
// runs it).  Doubles per problem, with mp = m_pad, ld = mp + 32, P the panel rows, S = 4 mp + 3 P:
//   9 mp ld (work matrices) + 2 mp 128 (inverse diagonal blocks) + S (vectors) + 128 (results) + 4096 (partial sums)
//   + 3 max(mp (P + 32), P ld) (panels) + 2 n (w, r) + 2 (white_var, mu_const);  with the gradient  + n (alpha)
//   + (max(P, mp) / 64) (mp / 64) (d + 2) (the contraction's partials);  and sizeof(KParams) + 8 bytes (parameters, info).
struct SgpBatchPlan {
  int64_t chunk, nchunks, bytes_per, P, panels, mp, ld, each, S, ws_each;
};

SgpBatchPlan sgp_batch_plan(int64_t n, int64_t m, int64_t d, int64_t panel_rows, int64_t T, bool want_grad, int64_t max_chunk,
                            int64_t budget_bytes) {
  SgpBatchPlan pl;
  pl.P = sgp_panel_rows(n, panel_rows);
  pl.mp = round_up(m, GPMI_NB);
  pl.ld = pl.mp + 32;
  pl.panels = (n + pl.P - 1) / pl.P;
  pl.each = std::max(pl.mp * (pl.P + 32), pl.P * pl.ld);
  pl.S = 4 * pl.mp + 3 * pl.P;
  pl.ws_each = (std::max(pl.P, pl.mp) / KT) * (pl.mp / KT) * (d + 2);
  int64_t doubles = 9 * pl.mp * pl.ld + 2 * pl.mp * GPMI_NB + pl.S + SGP_RED + 4 * SGP_RED_BLOCKS + 3 * pl.each + 2 * n + 2;
  if (want_grad) doubles += n + pl.ws_each;
  pl.bytes_per = 8 * doubles + (int64_t)sizeof(KParams) + 2 * (int64_t)sizeof(int);
  if (budget_bytes <= 0) budget_bytes = batch_budget_bytes();
  int64_t chunk = std::min<int64_t>(T, SGP_BATCH_MAX);
  if (max_chunk > 0) chunk = std::min(chunk, max_chunk);
  chunk = std::min(chunk, budget_bytes / pl.bytes_per);
  pl.chunk = std::max<int64_t>(chunk, 1);
  pl.nchunks = (T + pl.chunk - 1) / pl.chunk;
  return pl;
}

// the batch workspace for `B` problems of plan pl (with the gradient's part if want_grad): kept while it is large enough
int sgp_ensure_batch(gpmi_sgp* g, const SgpBatchPlan& pl, int64_t B, bool want_grad) {
  gpmi_ctx* c = g->ctx;
  gpmi_sgp::BatchWs& w = g->bw;
  if (B <= w.cap && pl.P <= w.panel && (w.grad || !want_grad)) return GPMI_OK;
  B = std::max(B, w.cap);
  want_grad = want_grad || w.grad;
  const int64_t P = std::max(pl.P, w.panel);
  const int64_t each = std::max(g->mp * (P + 32), P * g->ld);
  w = gpmi_sgp::BatchWs();
  const int64_t mp = g->mp, ld = g->ld, n = g->n;
  for (DevBuf<double>& q : w.M)
    if (int rc = q.alloc(c, B * mp * ld)) return rc;
  // (the zeros above the block-lower parts stay from here: gpmi_sgp_create)
  if (int rc = w.invD1.alloc_zeroed(c, B * mp * GPMI_NB)) return rc;
  if (int rc = w.invD2.alloc_zeroed(c, B * mp * GPMI_NB)) return rc;
  if (int rc = w.vec.alloc(c, B * (4 * mp + 3 * P))) return rc;
  if (int rc = w.red.alloc(c, B * SGP_RED)) return rc;
  if (int rc = w.part.alloc(c, B * 4 * SGP_RED_BLOCKS)) return rc;
  for (DevBuf<double>& q : w.P)
    if (int rc = q.alloc(c, B * each)) return rc;
  if (int rc = w.w.alloc(c, B * n)) return rc;
  if (int rc = w.r.alloc(c, B * n)) return rc;
  if (int rc = w.white.alloc(c, B)) return rc;
  if (int rc = w.mu.alloc(c, B)) return rc;
  if (int rc = w.info.alloc(c, 2 * B)) return rc;
  if (int rc = w.params.alloc(c, B)) return rc;
  if (want_grad) {
    if (int rc = w.alpha.alloc(c, B * n)) return rc;
    if (int rc = w.ws.alloc(c, B * (std::max(P, mp) / KT) * (mp / KT) * (g->d + 2))) return rc;
  }
  w.cap = B;
  w.panel = P;
  w.grad = want_grad;
  return GPMI_OK;
}

// what a chunk brings back for each of its problems
struct SgpBatchOut {
  double* F;
  double* grad;       // (n_theta + 1) per problem, or null
  double* sum_alpha;  // or null
  double* alpha;      // n per problem, or null
  int* info;
};

// One chunk: problems [0, B) with the parameters ps, white variances and means (mu_const: B values, or mus: B x n) of the
// host.  second: the gradient pass runs (grad, sum_alpha or alpha is wanted); want_grad: all of it, else alpha alone.
int sgp_batch_chunk(gpmi_sgp* g, const SgpBatchPlan& pl, int kernel, int64_t B, const KParams* ps, const double* white,
                    const double* mu_const, const double* mus, double jitter, int n_theta, bool second, bool want_grad,
                    const SgpBatchOut& out) {
  gpmi_ctx* c = g->ctx;
  hipStream_t s = c->sgp_stream;
  gpmi_sgp::BatchWs& w = g->bw;
  const int64_t n = g->n, m = g->m, mp = g->mp, ld = g->ld, d = g->d;
  const int nt = (int)(mp / GPMI_NB), nb = (int)B;
  const int64_t P = pl.P, ldp = P + 32, nd = mp * GPMI_NB;
  // the strides of the workspace as it was allocated (cap and panel may be larger than this call's)
  const int64_t sMat = mp * ld, sVec = 4 * mp + 3 * w.panel, sPanel = std::max(mp * (w.panel + 32), w.panel * ld);
  const int64_t sPart = 4 * SGP_RED_BLOCKS, sWs = (std::max(w.panel, mp) / KT) * (mp / KT) * (d + 2);
  double *G = w.M[MG], *A = w.M[MA], *LiT = w.M[MLIT], *Linv = w.M[MLINV], *W1 = w.M[MW1], *W2 = w.M[MW2], *LB = w.M[MLB],
         *W3 = w.M[MW3], *LBinv = w.M[MLBINV];
  double *b = w.vec, *v1 = b + mp, *cc = b + 2 * mp, *gamma = b + 3 * mp, *kg = b + 4 * mp, *q = kg + w.panel, *term = q + w.panel;
  const KParams* pdev = w.params;
  int *info1 = w.info, *info2 = w.info + w.cap;
  BatchShape bs;
  bs.count = nb;
  bs.sMat = sMat;
  bs.sInv = nd;
  bs.sVec = sVec;
  GemmBatch sq;  // products of the m x m matrices; ring_order_only: a value must not depend on the problems it shares a launch with
  sq.count = nb;
  sq.sC = sq.sA = sq.sB = sMat;
  sq.ring_order_only = true;
  auto nt_square_b = [&](double* C, const double* X, const double* Y) {
    launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, C, ld, X, ld, Y, ld, nt, nt, (int)mp, nullptr, sq);
  };
  auto inverse_factor_b = [&](const double* fac, const double* invD, double* scratch, double* dst) {
    trsm_identity_batched(s, fac, mp, ld, invD, scratch, bs);
    hipLaunchKernelGGL(sgp_transpose_kernel, dim3((unsigned)(mp / KT), (unsigned)(mp / KT), (unsigned)nb), dim3(SGP_NT), 0, s, scratch,
                       dst, ld, sMat);
  };
  const dim3 tiles_mm((unsigned)(mp / KT), (unsigned)(mp / KT), (unsigned)nb);

  HIPCHK(c, hipMemcpyAsync(w.params.get(), ps, sizeof(KParams) * B, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(w.white.get(), white, sizeof(double) * B, hipMemcpyHostToDevice, s));
  if (mu_const) HIPCHK(c, hipMemcpyAsync(w.mu.get(), mu_const, sizeof(double) * B, hipMemcpyHostToDevice, s));
  else HIPCHK(c, hipMemcpyAsync(w.r.get(), mus, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(sgp_residual_kernel, dim3(blocks(n), 1, (unsigned)nb), dim3(SGP_NT), 0, s, g->y, mu_const ? w.mu.get() : nullptr,
                     n, w.r.get());
  const unsigned nblk = weights_blocks(n);
  hipLaunchKernelGGL(sgp_weights_kernel, dim3(nblk, 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.r, g->nv, 0.0, w.white, n, w.w, w.part, n,
                     sPart);
  hipLaunchKernelGGL(sgp_colsum_kernel, dim3(4, 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.part, (int64_t)nblk, 4, w.red + RED_DATA, 0,
                     sPart, (int64_t)SGP_RED);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(G, 0, sizeof(double) * B * sMat, s));
  HIPCHK(c, hipMemsetAsync(w.vec.get(), 0, sizeof(double) * B * sVec, s));
  HIPCHK(c, hipMemsetAsync(w.info.get(), 0, sizeof(int) * 2 * w.cap, s));
  for (int64_t j0 = 0; j0 < n; j0 += P) {
    const int64_t rows = std::min<int64_t>(P, n - j0);
    double* Kp = w.P[0];
    {
      ProfScope ps_(c, s, GPMI_PROF_SGP_BUILD, 0.0, 8.0 * B * mp * P);
      launch_kbuild_cross_batched(s, kernel, pdev, nb, g->z, m, mp, g->x + j0 * d, rows, P, Kp, ldp, sPanel, (int)d);
      hipLaunchKernelGGL(sgp_scale_cols_kernel, dim3(blocks(rows), (unsigned)m, (unsigned)nb), dim3(SGP_NT), 0, s, Kp, ldp, rows,
                         w.w + j0, sPanel, n);
      hipLaunchKernelGGL(sgp_bvec_kernel, dim3((unsigned)m, 1, (unsigned)nb), dim3(SGP_NT), 0, s, Kp, ldp, rows, w.r + j0, w.w + j0, b,
                         j0 > 0 ? 1 : 0, sPanel, n, sVec);
    }
    {
      ProfScope ps_(c, s, GPMI_PROF_SGP_GRAM, (double)B * P * mp * (mp + GPMI_NB), 8.0 * B * (mp * P + 0.5 * mp * mp));
      GemmBatch gb;
      gb.count = nb;
      gb.sC = sMat;
      gb.sA = gb.sB = sPanel;
      gb.ring_order_only = true;
      launch_gemm_nt(s, TILES_LOWER, OP_SUB, G, ld, Kp, ldp, Kp, ldp, nt, nt, (int)P, nullptr, gb);  // -G until the sweep is over
    }
    HIPCHK(c, hipGetLastError());
  }
  {
    ProfScope ps_(c, s, GPMI_PROF_SGP_FACTOR, B * (2.0 * mp * mp * mp / 3.0 + 8.0 * mp * mp * mp), 8.0 * 12.0 * B * mp * mp);
    launch_mirror_lower(s, G, ld, mp, nb, sMat);
    launch_negate(s, G, B * sMat);
    launch_kbuild_cross_batched(s, kernel, pdev, nb, g->z, m, mp, g->z, m, mp, A, ld, sMat, (int)d);
    hipLaunchKernelGGL(sgp_pad_diag_kernel, dim3(blocks(mp), 1, (unsigned)nb), dim3(SGP_NT), 0, s, A, ld, m, mp, 0.0, jitter, pdev,
                       sMat);
    potrf_lower_batched(c, s, A, mp, ld, w.invD1, info1, bs);
    inverse_factor_b(A, w.invD1, LiT, Linv);
    nt_square_b(W1, Linv, G);   // L^-1 G   (G symmetric)
    nt_square_b(W2, W1, Linv);  // H = L^-1 G L^-T
    hipLaunchKernelGGL(sgp_sym_b_kernel, tiles_mm, dim3(SGP_NT), 0, s, W2, LB, ld, sMat);
    potrf_lower_batched(c, s, LB, mp, ld, w.invD2, info2, bs);
    inverse_factor_b(LB, w.invD2, W3, LBinv);
    launch_rows_dot(s, Linv, ld, mp, mp, b, v1, nb, sMat, sVec);
    launch_rows_dot(s, LBinv, ld, mp, mp, v1, cc, nb, sMat, sVec);
    hipLaunchKernelGGL(sgp_mm_reduce_kernel, dim3(1, 1, (unsigned)nb), dim3(SGP_NT), 0, s, LB, W2, ld, m, cc, w.red + RED_MM, sMat,
                       sVec, (int64_t)SGP_RED);
    HIPCHK(c, hipGetLastError());
  }
  if (second) {
    ProfScope ps_(c, s, GPMI_PROF_SGP_GRAD, 0.0, 0.0);
    double *T = A, *RT = W1, *Kinv = W3;
    nt_square_b(RT, LiT, LBinv);  // L^-T L_B^-T
    launch_rows_dot(s, RT, ld, mp, mp, cc, gamma, nb, sMat, sVec);
    if (want_grad) {
      const dim3 rows_mm(blocks(mp), (unsigned)mp, (unsigned)nb);
      nt_square_b(W2, RT, RT);      // S = L^-T B^-1 L^-1
      nt_square_b(Kinv, LiT, LiT);  // L^-T L^-1
      hipLaunchKernelGGL(sgp_sub_kernel, rows_mm, dim3(SGP_NT), 0, s, Kinv, W2, T, ld, mp, sMat);
      nt_square_b(LB, Kinv, G);     // K_mm^-1 G
      nt_square_b(W2, LB, Kinv);    // K_mm^-1 G K_mm^-1
      hipLaunchKernelGGL(sgp_sub_kernel, rows_mm, dim3(SGP_NT), 0, s, W2, T, LB, ld, mp, sMat);  // M2 - gamma gamma^T
    }
    HIPCHK(c, hipGetLastError());
    for (int64_t j0 = 0; j0 < n; j0 += P) {
      const int64_t rows = std::min<int64_t>(P, n - j0);
      double *KTp = w.P[0], *Mp = w.P[1];
      launch_kbuild_cross_batched(s, kernel, pdev, nb, g->x + j0 * d, rows, P, g->z, m, mp, KTp, ld, sPanel, (int)d);
      launch_rows_dot(s, KTp, ld, P, mp, gamma, kg, nb, sPanel, sVec);
      if (want_grad) {
        GemmBatch gb;
        gb.count = nb;
        gb.sC = gb.sA = sPanel;
        gb.sB = sMat;
        gb.ring_order_only = true;
        launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, Mp, ld, KTp, ld, T, ld, (int)(P / GPMI_NB), nt, (int)mp, nullptr, gb);
        hipLaunchKernelGGL(sgp_rowdot2_kernel, dim3((unsigned)rows, 1, (unsigned)nb), dim3(SGP_NT), 0, s, KTp, Mp, ld, m, q, sPanel,
                           sVec);
      }
      hipLaunchKernelGGL(sgp_alpha_kernel, dim3(blocks(rows), 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.r + j0, w.w + j0, kg,
                         want_grad ? q : (const double*)nullptr, 0.0, pdev, rows, w.alpha + j0, term, n, sVec);
      if (want_grad) {
        hipLaunchKernelGGL(sgp_colsum_kernel, dim3(1, 1, (unsigned)nb), dim3(SGP_NT), 0, s, term, rows, 1, w.red + RED_NOISE,
                           j0 > 0 ? 1 : 0, sVec, (int64_t)SGP_RED);
        launch_contract_batched(s, kernel, (int)d, pdev, nb, g->x + j0 * d, rows, P, g->z, m, mp, Mp, ld, w.w + j0, w.alpha + j0,
                                gamma, 1.0, 1.0, 0, 0.0, n_theta, w.ws, ContractStrides{sPanel, n, n, sVec, sWs});
        hipLaunchKernelGGL(sgp_colsum_kernel, dim3((unsigned)n_theta, 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.ws, (P / KT) * (mp / KT),
                           n_theta, w.red + RED_GRAD, j0 > 0 ? 1 : 0, sWs, (int64_t)SGP_RED);
      }
      HIPCHK(c, hipGetLastError());
    }
    if (want_grad) {
      // the K_mm term: weights -1/2 M2 = -1/2 (gamma gamma^T + LB), rows and columns are Z
      launch_contract_batched(s, kernel, (int)d, pdev, nb, g->z, m, mp, g->z, m, mp, LB, ld, nullptr, gamma, gamma, -0.5, -0.5, 1,
                              jitter, n_theta, w.ws, ContractStrides{sMat, 0, sVec, sVec, sWs});
      hipLaunchKernelGGL(sgp_colsum_kernel, dim3((unsigned)n_theta, 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.ws, (mp / KT) * (mp / KT),
                         n_theta, w.red + RED_GRAD, 1, sWs, (int64_t)SGP_RED);
    }
    if (out.sum_alpha) {
      hipLaunchKernelGGL(sgp_vecsum_kernel, dim3(nblk, 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.alpha.get(), n, w.part.get(), sPart);
      hipLaunchKernelGGL(sgp_colsum_kernel, dim3(1, 1, (unsigned)nb), dim3(SGP_NT), 0, s, w.part, (int64_t)nblk, 1, w.red + RED_SALPHA,
                         0, sPart, (int64_t)SGP_RED);
    }
    HIPCHK(c, hipGetLastError());
  }
  // the one wait of the chunk: results, info and, if asked for, alpha
  std::vector<double> hred((size_t)(B * SGP_RED));
  std::vector<int> hinfo((size_t)(2 * B));
  HIPCHK(c, hipMemcpyAsync(hred.data(), w.red.get(), sizeof(double) * B * SGP_RED, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(hinfo.data(), info1, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(hinfo.data() + B, info2, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  if (out.alpha) HIPCHK(c, hipMemcpyAsync(out.alpha, w.alpha.get(), sizeof(double) * B * n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const double LN_2PI = 1.8378770664093454836;
  for (int64_t t = 0; t < B; ++t) {
    const double* r = hred.data() + t * SGP_RED;
    out.info[t] = hinfo[t] != 0 ? hinfo[t] : (hinfo[B + t] != 0 ? (int)m + hinfo[B + t] : 0);
    const double a2 = ps[t].a2;
    out.F[t] = -0.5 * ((double)n * LN_2PI + r[RED_DATA + 1] + 2.0 * r[RED_MM] + r[RED_DATA] - r[RED_MM + 2]) -
               0.5 * (a2 * r[RED_DATA + 2] - r[RED_MM + 1]);
    if (out.grad) {
      double* gr = out.grad + t * (n_theta + 1);
      for (int k = 0; k < n_theta; ++k) gr[k] = r[RED_GRAD + k];
      gr[0] -= a2 * r[RED_DATA + 2];  // -1/2 sum w_i da^2 / d ln a
      gr[n_theta] = white[t] > 0.0 ? white[t] * r[RED_NOISE] : 0.0;
    }
    if (out.sum_alpha) out.sum_alpha[t] = r[RED_SALPHA];
  }
  return GPMI_OK;
}

}  // namespace

void sgp_release_all(gpmi_ctx* c) {
  if (c->sgp_stream) (void)hipStreamSynchronize(c->sgp_stream);
  for (gpmi_sgp* g : c->sgp_live) delete g;
  c->sgp_live.clear();
  if (c->sgp_stream) (void)hipStreamDestroy(c->sgp_stream);
  c->sgp_stream = nullptr;
}

extern "C" {

int gpmi_sgp_schedule(int64_t n, int64_t m, int64_t panel_rows, int64_t out[6]) {
  if (!out || !sgp_n_ok(n) || !sgp_m_ok(m) || !sgp_panel_ok(panel_rows)) return GPMI_ERR_ARG;
  const int64_t P = sgp_panel_rows(n, panel_rows), mp = round_up(m, GPMI_NB);
  out[0] = P;
  out[1] = mp;
  out[2] = zrun_tiles(P, mp);   // launch_zcontract of a data panel: rows = the panel, columns = Z
  out[3] = zrun_tiles(mp, mp);  // and of the K_mm term
  out[4] = weights_blocks(n);
  out[5] = (n + P - 1) / P;
  return GPMI_OK;
}

int gpmi_sgp_create(gpmi_ctx* c, int64_t n, int64_t d, const double* x, int64_t m, const double* z, gpmi_sgp** out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, out != nullptr, "gpmi_sgp_create: out is NULL");
  *out = nullptr;
  ARGCHK(c, x != nullptr && z != nullptr, "gpmi_sgp_create: x_host and z_host must be non-NULL");
  ARGCHK(c, sgp_n_ok(n), "gpmi_sgp_create: n out of range (2 .. 2^30)");
  ARGCHK(c, d >= 1 && d <= GPMI_MAX_D, "gpmi_sgp_create: d out of range (1 .. 64)");
  ARGCHK(c, sgp_m_ok(m), "gpmi_sgp_create: m out of range (1 .. 4096 = GPMI_SGP_MAX_M inducing points)");
  if (int rc = set_device(c)) return rc;
  if (!c->sgp_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->sgp_stream, hipStreamNonBlocking));
  gpmi_sgp* g = new gpmi_sgp();
  g->ctx = c;
  g->n = n;
  g->d = d;
  g->m = m;
  g->mp = round_up(m, GPMI_NB);
  g->ld = g->mp + 32;  // rows 256-byte aligned, off a power-of-two pitch
  const int64_t mp = g->mp, ld = g->ld, nd = mp / GPMI_NB * GPMI_NB * GPMI_NB;
  int rc = g->x.alloc(c, n * d);
  if (!rc) rc = g->z.alloc(c, mp * d);
  for (DevBuf<double>* q : {&g->r, &g->nv, &g->w, &g->alpha})
    if (!rc) rc = q->alloc(c, n);
  for (DevBuf<double>& q : g->M)
    if (!rc) rc = q.alloc(c, mp * ld);
  for (DevBuf<double>* q : {&g->fLinv, &g->fLBinv})
    if (!rc) rc = q->alloc(c, mp * ld);
  if (!rc) rc = g->fc.alloc(c, mp);
  if (!rc) rc = g->fgamma.alloc(c, mp);
  if (!rc) rc = g->invD1.alloc(c, nd);
  if (!rc) rc = g->invD2.alloc(c, nd);
  if (!rc) rc = g->vec.alloc(c, 4 * mp);
  if (!rc) rc = g->red.alloc(c, 128);
  if (!rc) rc = g->info.alloc(c, 2);
  if (!rc) rc = g->part.alloc(c, SGP_RED_BLOCKS * 4);
  if (!rc) rc = g->q_pts.alloc(c, SGP_QPANEL * d);
  if (!rc) rc = g->q_out.alloc(c, 2 * SGP_QPANEL);
  if (rc) {
    c->err = "gpmi_sgp_create: " + c->err;
    delete g;
    return rc;
  }
  // potrf_diag writes the block-lower part of an inverse only: the zeros above stay from here (api.hip: lane_alloc, ZERO_SYNC)
  hipError_t e = hipMemset(g->invD1, 0, sizeof(double) * nd);
  if (e == hipSuccess) e = hipMemset(g->invD2, 0, sizeof(double) * nd);
  if (e == hipSuccess) e = hipMemset(g->z, 0, sizeof(double) * mp * d);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipMemcpy(g->x, x, sizeof(double) * n * d, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(g->z, z, sizeof(double) * m * d, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    c->err = std::string("gpmi_sgp_create: ") + hipGetErrorString(e);
    delete g;
    return e == hipErrorOutOfMemory ? GPMI_ERR_NOMEM : GPMI_ERR_HIP;
  }
  c->sgp_live.push_back(g);
  *out = g;
  return GPMI_OK;
}

int gpmi_sgp_destroy(gpmi_sgp* g) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  auto it = std::find(c->sgp_live.begin(), c->sgp_live.end(), g);
  ARGCHK(c, it != c->sgp_live.end(), "gpmi_sgp_destroy: not a live object of this handle");
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->sgp_stream));
  c->sgp_live.erase(it);
  delete g;
  return GPMI_OK;
}

int gpmi_sgp_set_targets(gpmi_sgp* g, const double* r, const double* noise_var) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  ARGCHK(c, sgp_live(c, g), "gpmi_sgp_set_targets: not a live object of this handle");
  ARGCHK(c, r != nullptr, "gpmi_sgp_set_targets: r_host is NULL");
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->sgp_stream));
  HIPCHK(c, hipMemcpy(g->r, r, sizeof(double) * g->n, hipMemcpyHostToDevice));
  if (int rc = sgp_upload_noise(g, noise_var)) return rc;
  g->have_targets = true;
  return GPMI_OK;
}

int gpmi_sgp_set_observations(gpmi_sgp* g, const double* y, const double* noise_var) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  ARGCHK(c, sgp_live(c, g), "gpmi_sgp_set_observations: not a live object of this handle");
  ARGCHK(c, y != nullptr, "gpmi_sgp_set_observations: y_host is NULL");
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->sgp_stream));
  if (!g->y)
    if (int rc = g->y.alloc(c, g->n)) return rc;
  HIPCHK(c, hipMemcpy(g->y, y, sizeof(double) * g->n, hipMemcpyHostToDevice));
  if (int rc = sgp_upload_noise(g, noise_var)) return rc;
  g->have_obs = true;
  return GPMI_OK;
}

int gpmi_sgp_batch_schedule(int64_t n, int64_t m, int64_t d, int64_t panel_rows, int64_t T, int want_grad, int64_t max_chunk,
                            int64_t budget_bytes, int64_t out[6]) {
  if (!out || !sgp_n_ok(n) || !sgp_m_ok(m) || d < 1 || d > GPMI_MAX_D || !sgp_panel_ok(panel_rows) || T < 0 || max_chunk < 0 ||
      budget_bytes < 0)
    return GPMI_ERR_ARG;
  const SgpBatchPlan pl = sgp_batch_plan(n, m, d, panel_rows, T, want_grad != 0, max_chunk, budget_bytes);
  out[0] = pl.chunk;
  out[1] = pl.nchunks;
  out[2] = pl.bytes_per;
  out[3] = pl.P;
  out[4] = pl.panels;
  out[5] = pl.mp;
  return GPMI_OK;
}

int gpmi_sgp_bound_batch(gpmi_sgp* g, int kernel, int64_t T, const double* thetas, int n_theta, const double* white_var,
                         const double* mu_const, const double* mus, double jitter_rel, int64_t panel_rows, int64_t max_chunk,
                         double* F, double* grad, double* sum_alpha, double* alpha_host, int* info) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  const char* who = "gpmi_sgp_bound_batch";
  if (!sgp_live(c, g)) return sgp_arg_error(c, who, ": not a live object of this handle");
  if (T < 0) return sgp_arg_error(c, who, ": T must not be negative");
  if (T == 0) return GPMI_OK;
  ARGCHK(c, g->have_obs, "gpmi_sgp_bound_batch: gpmi_sgp_set_observations has not been called");
  ARGCHK(c, thetas && white_var && F && info, "gpmi_sgp_bound_batch: thetas, white_var_host, F and info must be non-NULL");
  ARGCHK(c, (mu_const != nullptr) != (mus != nullptr),
         "gpmi_sgp_bound_batch: exactly one of mu_const_host and mus_host must be given");
  ARGCHK(c, max_chunk >= 0, "gpmi_sgp_bound_batch: max_chunk must not be negative");
  ARGCHK(c, kernel != GPMI_KERNEL_SUM && kernel_is_stationary(kernel),
         "gpmi_sgp: the kernel must be GPMI_KERNEL_SE, _RQ, _M32 or _M52");
  const int off = kernel_theta_offset(kernel);
  ARGCHK(c, n_theta == g->d + off, "gpmi_sgp: n_theta does not match the kernel and the data dimension");
  ARGCHK(c, std::isfinite(jitter_rel) && jitter_rel >= 0.0, "gpmi_sgp: jitter_rel must be finite and not negative");
  ARGCHK(c, sgp_panel_ok(panel_rows), "gpmi_sgp: panel_rows out of range (0 .. 32768)");
  std::vector<KParams> ps((size_t)T);
  for (int64_t t = 0; t < T; ++t) {
    const double* theta = thetas + t * n_theta;
    for (int k = 0; k < n_theta; ++k) ARGCHK(c, std::isfinite(theta[k]), "gpmi_sgp: theta must be finite");
    const double wv = white_var[t];
    ARGCHK(c, std::isfinite(wv) && wv >= 0.0, "gpmi_sgp: white_var must be finite and not negative");
    // every noise_var_i + white_var positive and finite: the sum is monotone in noise_var_i, so its range decides
    ARGCHK(c, !g->nv_nan && g->nv_lo + wv > 0.0 && g->nv_hi + wv < std::numeric_limits<double>::infinity(),
           "gpmi_sgp: noise_var_i + white_var must be positive and finite for every data point");
    if (mu_const) ARGCHK(c, std::isfinite(mu_const[t]), "gpmi_sgp_bound_batch: mu_const_host must be finite");
    KParams& p = ps[(size_t)t];
    std::memset(&p, 0, sizeof(p));  // (the parameters as sgp_params forms them)
    p.kernel = kernel;
    p.d = (int)g->d;
    const double a = std::exp(theta[0]);
    p.a2 = a * a;
    p.kappa = (kernel == GPMI_KERNEL_RQ) ? std::exp(theta[1]) : 1.0;
    for (int k = 0; k < p.d; ++k) {
      const double l = std::exp(theta[off + k]);
      p.inv_l2[k] = 1.0 / (l * l);
    }
  }
  if (int rc = set_device(c)) return rc;
  const bool second = grad || sum_alpha || alpha_host;
  const SgpBatchPlan pl = sgp_batch_plan(g->n, g->m, g->d, panel_rows, T, second, max_chunk, 0);
  if (int rc = sgp_ensure_batch(g, pl, pl.chunk, second)) return rc;
  for (int64_t t0 = 0; t0 < T; t0 += pl.chunk) {
    const int64_t B = std::min(pl.chunk, T - t0);
    const SgpBatchOut out{F + t0, grad ? grad + t0 * (n_theta + 1) : nullptr, sum_alpha ? sum_alpha + t0 : nullptr,
                          alpha_host ? alpha_host + t0 * g->n : nullptr, info + t0};
    if (int rc = sgp_batch_chunk(g, pl, kernel, B, ps.data() + t0, white_var + t0, mu_const ? mu_const + t0 : nullptr,
                                 mus ? mus + t0 * g->n : nullptr, jitter_rel, n_theta, second, grad != nullptr, out))
      return rc;
  }
  return GPMI_OK;
}

int gpmi_sgp_set_inducing(gpmi_sgp* g, const double* z) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  ARGCHK(c, sgp_live(c, g), "gpmi_sgp_set_inducing: not a live object of this handle");
  ARGCHK(c, z != nullptr, "gpmi_sgp_set_inducing: z_host is NULL");
  for (int64_t i = 0; i < g->m * g->d; ++i) ARGCHK(c, std::isfinite(z[i]), "gpmi_sgp_set_inducing: z_host must be finite");
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->sgp_stream));
  HIPCHK(c, hipMemcpy(g->z, z, sizeof(double) * g->m * g->d, hipMemcpyHostToDevice));  // (the padding rows stay zero)
  g->fitted = false;
  return GPMI_OK;
}

int gpmi_sgp_bound_zgrad(gpmi_sgp* g, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
                         int64_t panel_rows, double* F, double* grad, double* grad_z, double* alpha_host, int* info) {
  if (!g) return GPMI_ERR_ARG;
  return sgp_bound(g, "gpmi_sgp_bound_zgrad", true, kernel, theta, n_theta, white_var, jitter_rel, panel_rows, F, grad, grad_z,
                   alpha_host, info);
}

int gpmi_sgp_bound(gpmi_sgp* g, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
                   int64_t panel_rows, double* F, double* grad, double* alpha_host, int* info) {
  if (!g) return GPMI_ERR_ARG;
  return sgp_bound(g, "gpmi_sgp_bound", false, kernel, theta, n_theta, white_var, jitter_rel, panel_rows, F, grad, nullptr,
                   alpha_host, info);
}

int gpmi_sgp_fit(gpmi_sgp* g, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
                 int64_t panel_rows, double* F, int* info) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  KParams p;
  double f = 0.0, sum_w = 0.0;
  if (int rc = sgp_begin(g, "gpmi_sgp_fit", kernel, theta, n_theta, white_var, jitter_rel, panel_rows, F, info, false, nullptr, p, f,
                         sum_w))
    return rc;
  if (*info != 0) return GPMI_OK;
  hipStream_t s = c->sgp_stream;
  launch_copy_rows(s, g->M[MLINV], g->ld, g->fLinv, g->ld, g->mp, g->mp);
  launch_copy_rows(s, g->M[MLBINV], g->ld, g->fLBinv, g->ld, g->mp, g->mp);
  launch_copy(s, g->vec + 2 * g->mp, g->fc, g->mp);
  // gamma = L^-T (L_B^-T c) from the two transposes sgp_factor left (the gradient path, which forms it too, did not run)
  launch_rows_dot(s, g->M[MW3], g->ld, g->mp, g->mp, g->fc, g->vec + 3 * g->mp);
  launch_rows_dot(s, g->M[MLIT], g->ld, g->mp, g->mp, g->vec + 3 * g->mp, g->fgamma);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(s));
  g->fp = p;
  g->fitted = true;
  *F = f;
  return GPMI_OK;
}

int gpmi_sgp_predict(gpmi_sgp* g, const double* pts, int64_t mq, double* mean, double* var) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  bool proceed;
  if (int rc = sgp_query_args(g, "gpmi_sgp_predict", mq, false, proceed)) return rc;
  if (!proceed) return GPMI_OK;
  ARGCHK(c, pts != nullptr && mean != nullptr, "gpmi_sgp_predict: pts_host and mean_host must be non-NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = sgp_ensure_panels(g, SGP_QPANEL)) return rc;
  hipStream_t s = c->sgp_stream;
  const int64_t d = g->d;
  for (int64_t q0 = 0; q0 < mq; q0 += SGP_QPANEL) {
    const int64_t rows = std::min<int64_t>(SGP_QPANEL, mq - q0), rp = round_up(rows, GPMI_NB);
    double *Kq = g->P[0], *V = g->P[1], *U = g->P[2];
    HIPCHK(c, hipMemcpyAsync(g->q_pts, pts + q0 * d, sizeof(double) * rows * d, hipMemcpyHostToDevice, s));
    sgp_query_panel(g, s, g->q_pts, rows, rp, Kq, V, U);
    hipLaunchKernelGGL(sgp_predict_kernel, dim3((unsigned)rows), dim3(SGP_NT), 0, s, V, U, g->ld, g->m, g->fc, g->fp.a2, g->q_out,
                       g->q_out + SGP_QPANEL);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(mean + q0, g->q_out, sizeof(double) * rows, hipMemcpyDeviceToHost, s));
    if (var) HIPCHK(c, hipMemcpyAsync(var + q0, g->q_out + SGP_QPANEL, sizeof(double) * rows, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));  // (the next panel overwrites the staging)
  }
  return GPMI_OK;
}

int gpmi_sgp_spatial_derivatives(gpmi_sgp* g, const double* pts, int64_t mq, double* dmean, double* dvar) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  bool proceed;
  if (int rc = sgp_query_args(g, "gpmi_sgp_spatial_derivatives", mq, false, proceed)) return rc;
  if (!proceed) return GPMI_OK;
  ARGCHK(c, pts != nullptr && dmean != nullptr, "gpmi_sgp_spatial_derivatives: pts_host and dmean_host must be non-NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = sgp_ensure_panels(g, SGP_QPANEL)) return rc;
  const int64_t m = g->m, mp = g->mp, ld = g->ld, d = g->d;
  const int64_t per = (int64_t)SGP_QPANEL * d;  // one result, or one run's partials, of a panel
  if (!g->qws)
    if (int rc = g->qws.alloc(c, 2 * (qruns(mp) + 1) * per)) return rc;
  double *ws_mean = g->qws, *ws_var = ws_mean + qruns(mp) * per, *out_mean = ws_var + qruns(mp) * per, *out_var = out_mean + per;
  hipStream_t s = c->sgp_stream;
  const int nt = (int)(mp / GPMI_NB);
  // ring_order_only: a row of a product must not depend on the number of row tiles (gpmi_internal.h: GemmBatch)
  GemmBatch gb;
  gb.ring_order_only = true;
  for (int64_t q0 = 0; q0 < mq; q0 += SGP_QPANEL) {
    const int64_t rows = std::min<int64_t>(SGP_QPANEL, mq - q0), rp = round_up(rows, GPMI_NB), nqp = round_up(rows, KT);
    const int ntr = (int)(rp / GPMI_NB);
    double *Kq = g->P[0], *V = g->P[1], *U = g->P[2], *W = g->P[0], *D = g->P[2], *Tq = g->P[1];
    HIPCHK(c, hipMemcpyAsync(g->q_pts, pts + q0 * d, sizeof(double) * rows * d, hipMemcpyHostToDevice, s));
    if (dvar) {
      // (profile classes: the products under GPMI_PROF_SGP_GRAM, the fused kernel under GPMI_PROF_SGP_GRAD)
      ProfScope ps(c, s, GPMI_PROF_SGP_GRAM, 8.0 * rp * mp * mp, 8.0 * 6.0 * rp * mp);
      sgp_query_panel(g, s, g->q_pts, rows, rp, Kq, V, U, gb);
      // the same two inverses the other way round (B k-major: no transposes are stored): rows (L_B^-T u)^T, then t^T
      launch_gemm(s, TILES_RECT, OP_ASSIGN, true, 0, W, ld, U, ld, g->fLBinv, ld, ntr, nt, (int)mp, nullptr, gb);
      hipLaunchKernelGGL(sgp_sub_kernel, dim3(blocks(mp), (unsigned)rp), dim3(SGP_NT), 0, s, W, V, D, ld, mp, 0);
      launch_gemm(s, TILES_RECT, OP_ASSIGN, true, 0, Tq, ld, D, ld, g->fLinv, ld, ntr, nt, (int)mp, nullptr, gb);
      HIPCHK(c, hipGetLastError());
    }
    {
      ProfScope ps(c, s, GPMI_PROF_SGP_GRAD, 0.0, 0.0);
      if (int rc = launch_qgrad(c, s, g->fp, g->z, m, mp, g->q_pts, rows, nqp, g->fgamma, Tq, ld, dvar != nullptr, ws_mean, ws_var,
                                out_mean, out_var))
        return rc;
    }
    HIPCHK(c, hipMemcpyAsync(dmean + q0 * d, out_mean, sizeof(double) * rows * d, hipMemcpyDeviceToHost, s));
    if (dvar) HIPCHK(c, hipMemcpyAsync(dvar + q0 * d, out_var, sizeof(double) * rows * d, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));  // (the next panel overwrites the staging)
  }
  return GPMI_OK;
}

int gpmi_sgp_posterior(gpmi_sgp* g, const double* pts, int64_t mq, double* mean, double* cov) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  bool proceed;
  if (int rc = sgp_query_args(g, "gpmi_sgp_posterior", mq, true, proceed)) return rc;
  if (!proceed) return GPMI_OK;
  ARGCHK(c, pts != nullptr && mean != nullptr, "gpmi_sgp_posterior: pts_host and mean_host must be non-NULL");
  if (int rc = set_device(c)) return rc;
  hipStream_t s = c->sgp_stream;
  PosteriorBufs b;
  if (int rc = b.alloc(g, mq, cov != nullptr)) return rc;
  int rc = sgp_posterior_sigma(g, pts, mq, b);
  hipError_t e = hipSuccess;
  if (rc == GPMI_OK) {
    e = hipMemcpyAsync(mean, b.mu, sizeof(double) * mq, hipMemcpyDeviceToHost, s);
    if (cov && e == hipSuccess) {
      launch_mirror_lower(s, b.Sigma, b.ldq, b.mpq);
      e = hipMemcpy2DAsync(cov, sizeof(double) * mq, b.Sigma, sizeof(double) * b.ldq, sizeof(double) * mq, (size_t)mq,
                           hipMemcpyDeviceToHost, s);
    }
  }
  const hipError_t e2 = hipStreamSynchronize(s);  // (before the buffers are released, whatever happened)
  if (rc != GPMI_OK) return rc;
  HIPCHK(c, e);
  HIPCHK(c, e2);
  return GPMI_OK;
}

int gpmi_sgp_posterior_draws(gpmi_sgp* g, const double* pts, int64_t mq, double jitter_rel, int64_t n_draws, const double* z_host,
                             int64_t seed, int64_t first_draw, double* mean, double* draws_host, double* eps_host, int* info) {
  if (!g) return GPMI_ERR_ARG;
  gpmi_ctx* c = g->ctx;
  bool proceed;
  if (int rc = sgp_query_args(g, "gpmi_sgp_posterior_draws", mq, true, proceed)) return rc;
  if (!proceed) return GPMI_OK;
  if (int rc = draws_check_args(c, mq, jitter_rel, n_draws, first_draw, draws_host)) return rc;
  ARGCHK(c, pts != nullptr, "gpmi_sgp_posterior_draws: pts_host is NULL");
  if (int rc = set_device(c)) return rc;
  if (info) *info = 0;
  if (c->lanes.empty()) {
    // a handle that only ever served sparse models: a lane of streams and events alone is all the tail needs (gpmi_mvn_draws)
    c->lanes.emplace_back();
    if (int rc = lane_streams(c, c->lanes[0])) return rc;
  }
  Lane& L = c->lanes[0];
  PosteriorBufs b;
  if (int rc = b.alloc(g, mq, true)) return rc;
  const int64_t mpq = b.mpq, ldq = b.ldq;
  int rc;
  {
    ProfScope ps(c, c->sgp_stream, GPMI_PROF_DRAWS_SIGMA, 4.0 * mpq * g->mp * g->mp + 2.0 * mpq * mpq * g->mp,
                 8.0 * mpq * (2.0 * g->mp + mpq));
    rc = sgp_posterior_sigma(g, pts, mq, b);
  }
  hipError_t e = hipSuccess;
  if (rc == GPMI_OK && mean) e = hipMemcpyAsync(mean, b.mu, sizeof(double) * mq, hipMemcpyDeviceToHost, c->sgp_stream);
  // the tail runs on the lane's stream: Sigma and mu are complete before it reads them
  const hipError_t e1 = hipStreamSynchronize(c->sgp_stream);
  if (rc == GPMI_OK && e == hipSuccess && e1 == hipSuccess)
    rc = draws_tail(c, L, b.Sigma, ldq, mq, mpq, b.mu, jitter_rel, n_draws, z_host, seed, first_draw,
                    draws_host, eps_host, info);
  const hipError_t e2 = hipStreamSynchronize(L.stream);  // (before Sigma is released, whatever the tail returned)
  if (rc != GPMI_OK) return rc;
  HIPCHK(c, e);
  HIPCHK(c, e1);
  HIPCHK(c, e2);
  return GPMI_OK;
}

}  // extern "C"
