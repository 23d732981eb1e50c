// C-ABI of libgpmi (include/gpmi.h): many targets at one set of inputs (gpmi_mt_*, MultiTargetGpRegressor).  T target
// vectors share x, the data errors and the hyper-parameters, so K, its factor, K^-1 and the predictive variance are
// computed once; per target there are only the O(N^2) solves.  The residuals live on the device as ROWS (mt_Tp x ld, zero
// in the padding: the layout of the many-right-hand-side solves of solve.hip), V^T = R^T L^-T and A^T = V^T L^-1 are one
// trsm_rows_forward and one trsm_rows_backward, the predictive means one launch_gemm_nt per chunk of query points.
// The fit runs on lane 0 with gpmi_fit's own stages (same L, same inverse blocks: the variance half of the predict is
// predict_rows as it stands); the evaluations at other hyper-parameters run on lane 1 and leave the fit alone.
// New device code: the tiled transposed copy, the per-point sum of squares over the targets, the fixed-order sum of the
// per-target terms.  No atomics; every sum's order is fixed by (n, T).
#include "api_internal.h"

namespace {

// out[c][r] = in[r][c] * scale / div[c] over the first out_rows x out_cols elements of `out` (gridDim.y x gridDim.x tiles
// of 64 x 64 cover them), zero where (r, c) is outside the in_rows x in_cols valid part of `in`.  div == nullptr: no
// division.  Both sides move whole 512-byte row pieces; the tile turns in LDS (rows padded by one double: the column
// read is conflict-free).
__global__ __launch_bounds__(256) void mt_transpose_kernel(const double* __restrict__ in, int64_t ldin, int64_t in_rows,
                                                           int64_t in_cols, double* __restrict__ out, int64_t ldout,
                                                           int64_t out_rows, int64_t out_cols, double scale,
                                                           const double* __restrict__ div) {
  __shared__ double t[64][65];
  const int bi = blockIdx.x, bj = blockIdx.y;  // tile of input rows, tile of input columns
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int64_t ir = (int64_t)bi * 64 + r, ic = (int64_t)bj * 64 + tx;
    t[r][tx] = (ir < in_rows && ic < in_cols) ? in[ir * ldin + ic] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int64_t orow = (int64_t)bj * 64 + r, ocol = (int64_t)bi * 64 + tx;
    if (orow >= out_rows || ocol >= out_cols) continue;
    double v = t[tx][r] * scale;
    if (div && orow < in_cols) v /= div[orow];
    out[orow * ldout + ocol] = v;
  }
}

// a2[i] = sum_t At[t][i]^2 over the T target rows, for 64 points per workgroup: wave w adds the rows t = w, w + 4, ... in
// order (each a 512-byte row piece), the four partial sums are added as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(256) void mt_colsumsq_kernel(const double* __restrict__ At, int64_t ld, int64_t T,
                                                          double* __restrict__ a2) {
  __shared__ double part[4][64];
  const int tx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + tx;
  const double* col = At + i;
  double s = 0.0;
#pragma unroll 8
  for (int64_t t = w; t < T; t += 4) {
    const double a = col[t * ld];
    s = fma(a, a, s);
  }
  part[w][tx] = s;
  __syncthreads();
  if (w == 0) a2[i] = (part[0][tx] + part[1][tx]) + (part[2][tx] + part[3][tx]);
}

// out[0] = sum of v[0 .. T): thread k adds v[k], v[k + 256], ... in order, then a binary tree over the 256 partial sums
__global__ __launch_bounds__(256) void mt_total_kernel(const double* __restrict__ v, int64_t T, double* __restrict__ out) {
  __shared__ double part[256];
  const int k = threadIdx.x;
  double s = 0.0;
  for (int64_t t = k; t < T; t += 256) s += v[t];
  part[k] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (k < h) part[k] += part[k + h];
    __syncthreads();
  }
  if (k == 0) out[0] = part[0];
}

// `in` (in_rows x in_cols valid) transposed into the out_rows x out_cols elements of `out`: the padded extent of a device
// operand (zeros beyond the valid part), or the dense in_cols x in_rows array a caller downloads (ldout = in_rows)
void launch_mt_transpose(hipStream_t s, const double* in, int64_t ldin, int64_t in_rows, int64_t in_cols, double* out,
                         int64_t ldout, int64_t out_rows, int64_t out_cols, double scale, const double* div) {
  hipLaunchKernelGGL(mt_transpose_kernel, dim3((unsigned)((out_cols + 63) / 64), (unsigned)((out_rows + 63) / 64)), dim3(256), 0,
                     s, in, ldin, in_rows, in_cols, out, ldout, out_rows, out_cols, scale, div);
}

// A^T (mt_Tp x ld) as the dense n x T array of a caller: into mtAn, then one contiguous copy to `host`
int mt_download_transposed(gpmi_ctx* c, hipStream_t s, const double* At, const double* div, double* host) {
  launch_mt_transpose(s, At, c->ld, c->mt_T, c->n, c->mtAn, c->mt_T, c->n, c->mt_T, 1.0, div);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(host, c->mtAn, sizeof(double) * c->n * c->mt_T, hipMemcpyDeviceToHost, s));
  return GPMI_OK;
}

double* mt_ss(gpmi_ctx* c) { return c->mtVec; }                      // |V_t|^2, mt_Tp of them
double* mt_total(gpmi_ctx* c) { return c->mtVec + c->mt_Tp; }        // their sum
double* mt_a2(gpmi_ctx* c) { return c->mtVec + c->mt_Tp + 8; }       // sum_t A_it^2, np of them

int mt_check(gpmi_ctx* c, const char* who) {
  if (c->mt_T < 1) {
    c->err = std::string(who) + ": gpmi_mt_set_targets has not been called for this data set";
    return GPMI_ERR_ARG;
  }
  return GPMI_OK;
}

int mt_check_fit(gpmi_ctx* c, const char* who) {
  if (int rc = mt_check(c, who)) return rc;
  if (!(c->fitted && c->mt_fitted)) {
    c->err = std::string(who) + " needs a successful gpmi_mt_fit";
    return GPMI_ERR_ARG;
  }
  return GPMI_OK;
}

// dst <- R^T L^-T (V^T, in place through the scratch panel), |V_t|^2 and their sum; with `backward` dst <- V^T L^-1 = A^T.
// L: the lane whose A holds the factor; s: its stream, ordered behind the factorisation.  dst and c->trsm_panel (mt_Tp
// rows) are allocated by the caller.
int mt_row_solves(gpmi_ctx* c, Lane& L, hipStream_t s, double* dst, bool backward) {
  if (int rc = ensure_inv2(c, L, s)) return rc;
  launch_copy(s, c->mtR, dst, c->mt_Tp * c->ld);
  trsm_rows_forward(c, s, L.A, c->np, c->ld, L.inv2, dst, c->mt_Tp, false, nullptr, c->trsm_panel);
  launch_rows_sumsq(s, dst, c->ld, c->mt_Tp, c->np, 0.0, mt_ss(c), 1, 0, 0, -1.0);  // (-(0 - sum): the sum itself)
  hipLaunchKernelGGL(mt_total_kernel, dim3(1), dim3(256), 0, s, mt_ss(c), c->mt_T, mt_total(c));
  if (backward) trsm_rows_backward(c, s, L.A, c->np, c->ld, L.invD, dst, c->mt_Tp, L.inv2, c->trsm_panel);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_mtVec, c->mtVec, sizeof(double) * (c->mt_Tp + 1), hipMemcpyDeviceToHost, s));
  return GPMI_OK;
}

// lml_t = -1/2 |V_t|^2 - sum ln L_ii, lml = -1/2 |V|_F^2 - T sum ln L_ii from the pinned mirror, behind the sync;
// -1e50 for a matrix that did not factorise
void mt_values(const gpmi_ctx* c, double logdet, int inf, double* lml_t, double* lml) {
  const double* h = c->h_mtVec;
  if (lml_t)
    for (int64_t t = 0; t < c->mt_T; ++t) lml_t[t] = (inf == 0) ? -0.5 * h[t] - logdet : -1e50;
  if (lml) *lml = (inf == 0) ? -0.5 * h[c->mt_Tp] - (double)c->mt_T * logdet : -1e50;
}

// what every evaluation reserves before it enqueues anything: the row buffer it solves in and the solves' scratch panel
int mt_reserve(gpmi_ctx* c, DevBuf<double>& rows, int64_t panel_rows) {
  if (int rc = rows.reserve(c, c->mt_Tp * c->ld)) return rc;
  return ensure_trsm_panel(c, panel_rows);
}

}  // namespace

extern "C" {

int gpmi_mt_set_targets(gpmi_ctx* c, const double* r_host, int64_t T) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, r_host != nullptr, "r_host is NULL");
  ARGCHK(c, T >= 1 && T <= GPMI_MT_MAX_T, "gpmi_mt_set_targets: T out of range (1 .. GPMI_MT_MAX_T)");
  if (int rc = set_device(c)) return rc;
  if (int rc = gpmi_sync(c)) return rc;  // (nothing of an earlier target matrix is in flight when its buffers go)
  static_cast<MultiBufs&>(*c) = MultiBufs();
  const int64_t Tp = round_up(T, GPMI_NB), ldt = Tp + 32;
  if (int rc = c->mtR.alloc(c, Tp * c->ld)) return rc;
  if (int rc = c->mtAn.alloc(c, c->np * ldt)) return rc;
  if (int rc = c->mtVec.alloc(c, Tp + 8 + c->np)) return rc;
  if (int rc = c->h_mtVec.alloc(c, Tp + 8 + c->np)) return rc;
  if (int rc = c->mtZero.alloc_zeroed(c, c->np)) return rc;
  // the caller's n x T array into the transposed copies' buffer, turned into rows on the device
  hipStream_t s = c->lanes[0].stream;
  HIPCHK(c, hipMemcpyAsync(c->mtAn, r_host, sizeof(double) * c->n * T, hipMemcpyHostToDevice, s));
  launch_mt_transpose(s, c->mtAn, T, c->n, T, c->mtR, c->ld, Tp, c->np, 1.0, nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(s));
  c->mt_T = T;
  c->mt_Tp = Tp;
  c->mt_ldt = ldt;
  return GPMI_OK;
}

int gpmi_mt_fit(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag, double* lml_t, double* lml,
                int* info) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check(c, "gpmi_mt_fit")) return rc;
  CovParams p;
  NO_PERIODIC(c, kernel);
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  if (int rc = set_device(c)) return rc;
  if (int rc = mt_reserve(c, c->mtA, c->mt_Tp)) return rc;
  const std::vector<double> mu(c->n, 0.0);  // the offsets are in the residuals; the handle's own y takes no part
  const LaneEval ev(c, 0);
  c->fitted = false;
  // gpmi_fit's stages: L in lane 0, the predict's inverse blocks beside the two sweeps
  if (int rc = lane_stages(ev, LaneBuild::kernels(p), LN_BACKWARD | LN_FIT_SCHEDULE, mu.data())) return rc;
  if (int rc = mt_row_solves(c, ev.L(), ev.stream(), c->mtA, true)) return rc;
  int inf = 0;
  double logdet = 0.0;
  if (int rc = lane_collect(ev, LC_LOGDET, 0, {}, &logdet, &inf)) return rc;
  mt_values(c, logdet, inf, lml_t, lml);
  if (info) *info = inf;
  c->fit_params = p;
  c->fitted = c->mt_fitted = (inf == 0);
  return GPMI_OK;
}

int gpmi_mt_lml(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag, double* lml_t, double* lml,
                int* info) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check(c, "gpmi_mt_lml")) return rc;
  CovParams p;
  NO_PERIODIC(c, kernel);
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, lml_t || lml, "lml_t and lml are both NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = mt_reserve(c, c->mtW, c->mt_Tp)) return rc;
  const std::vector<double> mu(c->n, 0.0);
  const LaneEval ev(c, 1);
  if (int rc = lane_stages(ev, LaneBuild::kernels(p), 0, mu.data())) return rc;
  if (int rc = mt_row_solves(c, ev.L(), ev.stream(), c->mtW, false)) return rc;
  int inf = 0;
  double logdet = 0.0;
  if (int rc = lane_collect(ev, LC_LOGDET, 0, {}, &logdet, &inf)) return rc;
  mt_values(c, logdet, inf, lml_t, lml);
  if (info) *info = inf;
  return GPMI_OK;
}

int gpmi_mt_lml_grad(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag, double* lml, double* grad,
                     int* info) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check(c, "gpmi_mt_lml_grad")) return rc;
  CovParams p;
  NO_PERIODIC(c, kernel);
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, lml && grad, "lml / grad is NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = mt_reserve(c, c->mtW, c->mt_Tp > c->np ? c->mt_Tp : c->np)) return rc;  // (np rows: the inverse factor's)
  const std::vector<double> mu(c->n, 0.0);
  const LaneEval ev(c, 1);
  const int nt = (int)(c->np / GPMI_NB);
  // A^T needs L, which the SYRK overwrites with K^-1: the row solves go between the factorisation and the inverse
  if (int rc = lane_forward(ev, LaneBuild::kernels(p), LN_INVERSE | LN_SYRK, mu.data(), n_theta)) return rc;
  Lane& L = ev.L();  // (only now: lane_forward creates lane 1 on its first use, and the lanes move when their vector grows)
  hipStream_t s = ev.stream();
  if (int rc = mt_row_solves(c, L, s, c->mtW, true)) return rc;
  if (int rc = lane_solves(ev, LN_INVERSE | LN_SYRK)) return rc;
  // K^-1 - A~ A~^T with A~ = A / sqrt(T) on the lower tiles: the contraction with u = v = 0 then returns
  // -1/2 sum (K^-1 - A~ A~^T) o dK, 1 / T of the gradient - ONE pass over K^-1 for all the targets
  launch_mt_transpose(s, c->mtW, c->ld, c->mt_T, c->n, c->mtAn, c->mt_ldt, c->np, c->mt_Tp, 1.0 / std::sqrt((double)c->mt_T),
                      nullptr);
  const double tiles = 0.5 * nt * (nt + 1);  // (timed as the trailing updates are: in-kernel stamps, class GPMI_PROF_SYRK)
  launch_gemm_nt(s, TILES_LOWER, OP_SUB, L.A, c->ld, c->mtAn, c->mt_ldt, c->mtAn, c->mt_ldt, nt, nt, (int)c->mt_Tp,
                 prof_stamp_slot(c, tiles * 2.0 * GPMI_NB * GPMI_NB * c->mt_Tp, tiles * 16.0 * GPMI_NB * GPMI_NB));
  launch_lml_grad(s, p, n_theta, c->x, c->n, c->np, L.A, c->ld, c->mtZero, c->mtZero, ev.partial(false), ev.gout());
  int inf = 0;
  double logdet = 0.0;
  if (int rc = lane_collect(ev, LC_LOGDET, n_theta + 1, {}, &logdet, &inf)) return rc;
  mt_values(c, logdet, inf, nullptr, lml);
  for (int j = 0; j <= n_theta; ++j) grad[j] = (double)c->mt_T * ev.h_gout()[j];
  if (info) *info = inf;
  return GPMI_OK;
}

int gpmi_mt_loo_terms(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag, double* a2_host,
                      double* ikdiag_host, int* info) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check(c, "gpmi_mt_loo_terms")) return rc;
  CovParams p;
  NO_PERIODIC(c, kernel);
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, a2_host && ikdiag_host, "a2_host / ikdiag_host is NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = mt_reserve(c, c->mtW, c->mt_Tp > c->np ? c->mt_Tp : c->np)) return rc;
  const std::vector<double> mu(c->n, 0.0);
  const LaneEval ev(c, 1);
  if (int rc = lane_forward(ev, LaneBuild::kernels(p), LN_INVERSE, mu.data())) return rc;
  hipStream_t s = ev.stream();  // (of a lane that lane_forward may just have created)
  if (int rc = mt_row_solves(c, ev.L(), s, c->mtW, true)) return rc;
  if (int rc = lane_solves(ev, LN_INVERSE)) return rc;
  // diag(K^-1)_i = squared norm of row i of L^-T (lane_loo_terms); sum_t A_it^2 down the columns of A^T
  launch_rows_sumsq(s, ev.L().B2, c->ld, c->np, c->np, 0.0, ev.slot2(), 1, 0, 0, -1.0);
  hipLaunchKernelGGL(mt_colsumsq_kernel, dim3((unsigned)(c->np / 64)), dim3(256), 0, s, c->mtW, c->ld, c->mt_T, mt_a2(c));
  return lane_collect(ev, 0, 0, {{a2_host, mt_a2(c)}, {ikdiag_host, ev.slot2()}}, nullptr, info);
}

int gpmi_mt_alpha(gpmi_ctx* c, double* alpha_host) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check_fit(c, "gpmi_mt_alpha")) return rc;
  ARGCHK(c, alpha_host != nullptr, "alpha_host is NULL");
  if (int rc = set_device(c)) return rc;
  hipStream_t s = c->lanes[0].stream;
  if (int rc = mt_download_transposed(c, s, c->mtA, nullptr, alpha_host)) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  return GPMI_OK;
}

int gpmi_mt_predict(gpmi_ctx* c, const double* pts, int64_t m, double* mean_host, double* var_host) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check_fit(c, "gpmi_mt_predict")) return rc;
  ARGCHK(c, pts && m > 0 && mean_host, "pts / mean_host is NULL or m <= 0");
  if (int rc = set_device(c)) return rc;
  // (predict_rows: 2048 points at a time) the product's padded rows, and behind them the dense rows the caller gets
  if (int rc = c->mtMean.reserve(c, 2048 * (c->mt_ldt + c->mt_T))) return rc;
  double* dense = c->mtMean + 2048 * c->mt_ldt;
  hipStream_t s = c->lanes[0].stream;
  const CovParams& p = c->fit_params;
  const int64_t T = c->mt_T;
  auto fill = [&](int64_t m0, int64_t mc, int64_t mp) -> int {
    HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * c->d, sizeof(double) * mc * c->d, hipMemcpyHostToDevice, s));
    {
      ProfScope ps(c, s, GPMI_PROF_KBUILD, 0.0, 8.0 * mp * c->np);
      launch_kbuild_cross(s, p, c->pts, mc, mp, c->x, c->n, c->np, c->Q, c->ld);
    }
    // the chunk's means: K* A, read before the variance's solve consumes K*
    {
      ProfScope ps(c, s, GPMI_PROF_TRSM, 2.0 * mp * c->np * c->mt_Tp, 8.0 * (mp + c->mt_Tp) * c->np);
      launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, c->mtMean, c->mt_ldt, c->Q, c->ld, c->mtA, c->ld, (int)(mp / GPMI_NB),
                     (int)(c->mt_Tp / GPMI_NB), (int)c->np);
    }
    launch_copy_rows(s, c->mtMean, c->mt_ldt, dense, T, T, mc);
    HIPCHK(c, hipMemcpyAsync(mean_host + m0 * T, dense, sizeof(double) * mc * T, hipMemcpyDeviceToHost, s));
    return GPMI_OK;
  };
  return predict_rows(c, m, fill, p.a2, nullptr, var_host);  // K_qq[0,0] = a^2, as gpmi_predict
}

int gpmi_mt_loo(gpmi_ctx* c, double* resid_loo_host, double* ikdiag_host) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = mt_check_fit(c, "gpmi_mt_loo")) return rc;
  ARGCHK(c, resid_loo_host && ikdiag_host, "resid_loo_host / ikdiag_host is NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_lanes(c, 2)) return rc;
  Lane& F = c->lanes[0];
  Lane& L = c->lanes[1];
  hipStream_t s = L.stream;
  if (int rc = ensure_second_matrix(c, L)) return rc;
  HIPCHK(c, hipStreamSynchronize(F.stream));
  // as gpmi_loo_diag: L^-T of the fit's factor into lane 1's second matrix, its squared row norms; then A_it / (K^-1)_ii
  if (int rc = enqueue_inverse_factor(c, L, F)) return rc;
  launch_rows_sumsq(s, L.B2, c->ld, c->np, c->np, 0.0, L.vec, 1, 0, 0, -1.0);
  if (int rc = mt_download_transposed(c, s, c->mtA, L.vec, resid_loo_host)) return rc;
  HIPCHK(c, hipMemcpyAsync(ikdiag_host, L.vec, sizeof(double) * c->n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return GPMI_OK;
}

}  // extern "C"
