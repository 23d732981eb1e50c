// C-ABI of libgpmi (include/gpmi.h): Gaussian processes with a non-Gaussian, log-concave likelihood by Laplace's method
// (gpmi_ggp_*, GeneralisedGpRegressor).  The latent f = m + K a is observed through p(y_i | f_i); the mode of
// psi(a) = -1/2 a^T (f - m) + sum log p is Newton's iteration (GPML Alg. 3.1) over the pieces the Gaussian models are made
// of: the kernel build for K, B = I + sw sw^T o K by launch_scale_add / launch_add_diag_vec, potrf_lower, the two
// triangular sweeps, and for the gradient the many-right-hand-side solve, L^-T, the SYRK and launch_lml_grad's contraction
// with (u, v, iK) = (g + 2 w, g, R).  New device code (generalised.hip): the likelihood terms with their fixed-order sums,
// the K V product, the step blend.  The fit runs on lane 0 and leaves L, g (in the handle's alpha) and sw for the
// predict; evaluations at other hyper-parameters run on lane 1 and leave the fit alone.  The host reads one record of four
// doubles and the info word per Newton step (and per halving); everything else stays on the device.
#include "api_internal.h"

namespace {

// the work vectors of a lane (np each, GGP_NVEC of them); a / fm, their proposals and their blends lie side by side
enum GgpVecs {
  GV_A = 0, GV_FM, GV_A_NEW, GV_FM_NEW, GV_A_TRY, GV_FM_TRY,
  GV_G, GV_W, GV_SW, GV_D3, GV_B,
  GV_T1, GV_T2, GV_T3, GV_T4,  // K b (later the squared row norms), sw o K b (later R K s2), the two sweeps' solutions
  GV_S2, GV_KS2, GV_U,
  GV_COUNT
};
static_assert(GV_COUNT == GGP_NVEC, "GGP_NVEC (gpmi_internal.h) is the number of work vectors");

struct GgpRun {
  double logq = -1e50, psi = 0.0;
  int iters = 0, halvings = 0, info = 0;
};

struct GgpLane {
  gpmi_ctx* c;
  int lane;
  GgpLane(gpmi_ctx* ctx, int index) : c(ctx), lane(index) {}
  Lane& L() const { return c->lanes[(size_t)lane]; }
  double* K() const { return c->ggK[lane]; }
  double* vec(int k) const { return c->ggVec[lane] + (int64_t)k * c->np; }
  double* part() const { return c->ggPart[lane]; }
  double* rec() const { return c->ggRec[lane]; }
  GgpTerms terms() const { return {vec(GV_G), vec(GV_W), vec(GV_SW), vec(GV_D3), vec(GV_B)}; }
};

int ggp_check(gpmi_ctx* c, const char* who) {
  if (c->n <= 0 || c->ggp_lik < 0) {
    c->err = std::string(who) + ": gpmi_ggp_set_observations has not been called for this data set";
    return GPMI_ERR_ARG;
  }
  return GPMI_OK;
}

int ggp_check_fit(gpmi_ctx* c, const char* who) {
  if (int rc = ggp_check(c, who)) return rc;
  if (!c->ggp_fitted) {
    c->err = std::string(who) + " needs a successful gpmi_ggp_fit";
    return GPMI_ERR_ARG;
  }
  return GPMI_OK;
}

// the arguments every evaluation shares, before any device call
int ggp_eval_args(gpmi_ctx* c, const char* who, int kernel, const double* theta, int n_theta, double tol, int max_iter,
                  const double* logq, const int* out_iters, const int* info, CovParams& p) {
  if (int rc = ggp_check(c, who)) return rc;
  NO_PERIODIC(c, kernel);
  if (int rc = make_params(c, kernel, theta, n_theta, 0.0, p)) return rc;
  ARGCHK(c, tol > 0.0 && tol < 1.0, "tol must lie in (0, 1)");
  ARGCHK(c, max_iter >= 1, "max_iter must be at least 1");
  ARGCHK(c, logq && out_iters && info, "logq / out_iters / info is NULL");
  return GPMI_OK;
}

// the lane and its generalised-GP buffers
int ggp_reserve(gpmi_ctx* c, int lane) {
  if (int rc = ensure_lanes(c, (size_t)lane + 1)) return rc;
  if (int rc = c->ggK[lane].reserve(c, c->np * c->ld)) return rc;
  if (int rc = c->ggVec[lane].reserve(c, (int64_t)GGP_NVEC * c->np)) return rc;
  if (int rc = c->ggPart[lane].reserve(c, ggp_part_doubles(c->np))) return rc;
  if (int rc = c->ggRec[lane].reserve(c, 8)) return rc;
  return c->h_ggRec.reserve(c, 8);
}

// latent K (both triangles, the builders' jitter, identity in the padding) into the lane's K
void ggp_build_k(const GgpLane& g, const CovParams& p) {
  gpmi_ctx* c = g.c;
  hipStream_t s = g.L().stream;
  ProfScope ps(c, s, GPMI_PROF_KBUILD, 0.0, 8.0 * c->np * c->np);
  launch_kbuild_square(s, p, c->x, c->n, c->np, c->ggZero, g.K(), c->ld, false);
}

// the likelihood terms at (a, fm) and the record; fm_prev: what max |f - f_prev| is taken against (may be null)
void ggp_terms(const GgpLane& g, const double* a, const double* fm, const double* fm_prev) {
  gpmi_ctx* c = g.c;
  hipStream_t s = g.L().stream;
  ProfScope ps(c, s, GPMI_PROF_GGP_TERMS, 0.0, 8.0 * 11 * c->np);
  launch_ggp_terms(s, c->ggp_lik, c->ggY, c->ggAux, c->ggConst, c->ggp_offset, a, fm, fm_prev, c->n, c->np, g.terms(), g.part(),
                   g.rec());
}

void ggp_kv(const GgpLane& g, const double* M, int nv, const GgpKv& a) {
  gpmi_ctx* c = g.c;
  hipStream_t s = g.L().stream;
  ProfScope ps(c, s, GPMI_PROF_GGP_KV, 2.0 * nv * c->np * c->np, 8.0 * c->np * c->np);
  launch_ggp_kv(s, M, c->ld, c->np, nv, a);
}
void ggp_kv1(const GgpLane& g, const double* M, const double* v, double* y) {
  GgpKv a{};
  a.v[0] = v;
  a.y[0] = y;
  ggp_kv(g, M, 1, a);
}

// B = I + sw sw^T o K into the lane's matrix, then its factor L (and the inverse diagonal blocks)
int ggp_factor(const GgpLane& g) {
  gpmi_ctx* c = g.c;
  Lane& L = g.L();
  hipStream_t s = L.stream;
  L.inv2_valid = false;
  L.identity_ready = false;
  L.early = Lane::EarlyWork();  // (nothing of ours rides beside the factorisation)
  HIPCHK(c, hipMemsetAsync(L.info, 0, sizeof(int), s));
  {
    ProfScope ps(c, s, GPMI_PROF_GGP_BFORM, 0.0, 16.0 * c->np * c->np);
    launch_scale_add(s, L.A, c->ld, g.K(), c->ld, g.vec(GV_SW), g.vec(GV_SW), c->np, c->np, false);
    launch_add_diag_vec(s, L.A, c->ld, c->ggZero, 1.0, c->np);
  }
  potrf_lower(c, L, L.A, c->np, c->ld, L.invD, L.info, true);
  HIPCHK(c, hipGetLastError());
  return GPMI_OK;
}

// the record and the info word of the lane, behind everything enqueued so far
int ggp_read(const GgpLane& g, double* rec4, int* info) {
  gpmi_ctx* c = g.c;
  Lane& L = g.L();
  hipStream_t s = L.stream;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_ggRec, g.rec(), 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(L.h_info, L.info, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (int k = 0; k < 4; ++k) rec4[k] = c->h_ggRec[k];
  *info = L.h_info[0];
  INFOCHK(c, *info);
  return GPMI_OK;
}

inline double ggp_psi(const double* rec4) { return -0.5 * rec4[1] + rec4[0]; }

// Newton's iteration from a = 0 on the lane, then the factor of B at the final f and log q.  On return with run.info == 0
// the lane holds: L in its matrix, K, a / fm = f - m, and g, W, sw, d3 at the final f.
int ggp_newton(const GgpLane& g, const CovParams& p, double tol, int max_iter, GgpRun& run) {
  gpmi_ctx* c = g.c;
  Lane& L = g.L();
  hipStream_t s = L.stream;
  const int64_t np = c->np;
  if (g.lane == 0) c->fitted = c->mt_fitted = c->ggp_fitted = false;  // lane 0 gets another factor
  potrf_pair_quiesce(L);
  ggp_build_k(g, p);
  HIPCHK(c, hipMemsetAsync(g.vec(GV_A), 0, sizeof(double) * 2 * np, s));
  HIPCHK(c, hipMemsetAsync(L.info, 0, sizeof(int), s));
  ggp_terms(g, g.vec(GV_A), g.vec(GV_FM), nullptr);
  double rec[4];
  int inf = 0;
  if (int rc = ggp_read(g, rec, &inf)) return rc;
  double psi = ggp_psi(rec);
  bool converged = false;
  run = GgpRun();
  if (!std::isfinite(psi)) {
    run.info = -1;
    return GPMI_OK;
  }
  for (int it = 1; it <= max_iter && !converged; ++it) {
    if (int rc = ggp_factor(g)) return rc;
    // a+ = b - sw o B^-1 (sw o K b), f+ - m = K a+
    ggp_kv1(g, g.K(), g.vec(GV_B), g.vec(GV_T1));
    launch_vec_mul(s, g.vec(GV_SW), g.vec(GV_T1), g.vec(GV_T2), np);
    trsv_forward(c, s, L.A, np, c->ld, L.invD, g.vec(GV_T2), g.vec(GV_T3), L.info);
    trsv_backward(c, s, L.A, np, c->ld, L.invD, g.vec(GV_T3), g.vec(GV_T4), L.info);
    launch_ggp_newton_a(s, g.vec(GV_B), g.vec(GV_SW), g.vec(GV_T4), g.vec(GV_A_NEW), np);
    ggp_kv1(g, g.K(), g.vec(GV_A_NEW), g.vec(GV_FM_NEW));
    // the terms at the proposal: psi(a+), and - if it is accepted - the next step's g, W, sw, b
    ggp_terms(g, g.vec(GV_A_NEW), g.vec(GV_FM_NEW), g.vec(GV_FM));
    if (int rc = ggp_read(g, rec, &inf)) return rc;
    run.iters = it;
    if (inf != 0) {
      run.info = inf;
      return GPMI_OK;
    }
    double psi_new = ggp_psi(rec), step = 1.0;
    int h = 0;
    const double* accepted = g.vec(GV_A_NEW);
    while (!(psi_new >= psi - 1e-12 * std::fabs(psi)) && h < 10) {
      ++h;
      step *= 0.5;
      launch_ggp_blend(s, g.vec(GV_A), g.vec(GV_A_NEW), step, g.vec(GV_A_TRY), 2 * np);
      ggp_terms(g, g.vec(GV_A_TRY), g.vec(GV_FM_TRY), g.vec(GV_FM));
      if (int rc = ggp_read(g, rec, &inf)) return rc;
      psi_new = ggp_psi(rec);
      accepted = g.vec(GV_A_TRY);
    }
    run.halvings += h;
    if (!std::isfinite(psi_new)) {
      run.info = -1;
      return GPMI_OK;
    }
    launch_copy(s, accepted, g.vec(GV_A), 2 * np);
    psi = psi_new;
    converged = rec[2] <= tol * (1.0 + rec[3]);
  }
  run.psi = psi;
  if (!converged) {
    run.info = -1;
    return GPMI_OK;
  }
  // g, W, sw, d3 are those of the final f (the last terms were taken at the accepted point): L at the final f
  if (int rc = ggp_factor(g)) return rc;
  launch_lml_reduce(s, g.vec(GV_T3), L.A, c->ld, np, L.red);
  HIPCHK(c, hipMemcpyAsync(L.h_red, L.red, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (int rc = ggp_read(g, rec, &inf)) return rc;
  run.info = inf;
  if (inf == 0) run.logq = psi - L.h_red[1];
  return GPMI_OK;
}

void ggp_report(const GgpRun& run, double* logq, int* out_iters, int* info) {
  *logq = (run.info == 0) ? run.logq : -1e50;
  out_iters[0] = run.iters;
  out_iters[1] = run.halvings;
  *info = run.info;
}

}  // namespace

extern "C" {

int gpmi_ggp_set_observations(gpmi_ctx* c, int likelihood, const double* y, const double* aux, double offset) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, likelihood == GPMI_GGP_LOGISTIC || likelihood == GPMI_GGP_POISSON || likelihood == GPMI_GGP_BINOMIAL,
         "gpmi_ggp_set_observations: unknown likelihood id");
  ARGCHK(c, y && aux, "y / aux is NULL");
  ARGCHK(c, std::isfinite(offset), "gpmi_ggp_set_observations: the offset is not finite");
  const int64_t n = c->n;
  // y, aux and the f-independent part of log p, one after another in one host array
  std::vector<double> h((size_t)(3 * n));
  for (int64_t i = 0; i < n; ++i) {
    const double yi = y[i], ax = aux[i];
    ARGCHK(c, std::isfinite(yi) && std::isfinite(ax), "gpmi_ggp_set_observations: y / aux holds a value that is not finite");
    double lc = 0.0;
    if (likelihood == GPMI_GGP_LOGISTIC) {
      ARGCHK(c, ax > 0.0, "gpmi_ggp_set_observations: the logistic scales (aux) must be positive");
      lc = -std::log(ax);
    } else if (likelihood == GPMI_GGP_POISSON) {
      ARGCHK(c, ax > 0.0, "gpmi_ggp_set_observations: the Poisson exposures (aux) must be positive");
      ARGCHK(c, yi >= 0.0 && yi == std::floor(yi), "gpmi_ggp_set_observations: Poisson counts (y) must be integers >= 0");
      lc = yi * std::log(ax) - std::lgamma(yi + 1.0);
    } else {
      ARGCHK(c, ax >= 1.0 && ax == std::floor(ax), "gpmi_ggp_set_observations: the binomial trials (aux) must be integers >= 1");
      ARGCHK(c, yi >= 0.0 && yi <= ax && yi == std::floor(yi),
             "gpmi_ggp_set_observations: binomial successes (y) must be integers in 0 .. trials");
      lc = std::lgamma(ax + 1.0) - std::lgamma(yi + 1.0) - std::lgamma(ax - yi + 1.0);
    }
    h[(size_t)i] = yi;
    h[(size_t)(n + i)] = ax;
    h[(size_t)(2 * n + i)] = lc;
  }
  if (int rc = set_device(c)) return rc;
  if (int rc = gpmi_sync(c)) return rc;  // (nothing of earlier observations is in flight when their buffers go)
  c->ggp_fitted = false;
  c->ggp_lik = -1;
  if (int rc = c->ggY.alloc_zeroed(c, c->np)) return rc;
  if (int rc = c->ggAux.alloc_zeroed(c, c->np)) return rc;
  if (int rc = c->ggConst.alloc_zeroed(c, c->np)) return rc;
  if (int rc = c->ggZero.alloc_zeroed(c, c->np)) return rc;
  HIPCHK(c, hipMemcpy(c->ggY, h.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->ggAux, h.data() + n, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->ggConst, h.data() + 2 * n, sizeof(double) * n, hipMemcpyHostToDevice));
  c->ggp_lik = likelihood;
  c->ggp_offset = offset;
  return GPMI_OK;
}

int gpmi_ggp_fit(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double tol, int max_iter, double* logq,
                 int* out_iters, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = ggp_eval_args(c, "gpmi_ggp_fit", kernel, theta, n_theta, tol, max_iter, logq, out_iters, info, p)) return rc;
  if (int rc = set_device(c)) return rc;
  if (int rc = ggp_reserve(c, 0)) return rc;
  const GgpLane g(c, 0);
  GgpRun run;
  if (int rc = ggp_newton(g, p, tol, max_iter, run)) return rc;
  ggp_report(run, logq, out_iters, info);
  if (run.info != 0) return GPMI_OK;
  // the predict's mean is k(q)^T g: g where the Gaussian fit keeps its alpha
  hipStream_t s = g.L().stream;
  launch_copy(s, g.vec(GV_G), c->alpha, c->np);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(s));
  c->fit_params = p;
  c->ggp_fitted = true;
  return GPMI_OK;
}

int gpmi_ggp_logq(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double tol, int max_iter, double* logq,
                  int* out_iters, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = ggp_eval_args(c, "gpmi_ggp_logq", kernel, theta, n_theta, tol, max_iter, logq, out_iters, info, p)) return rc;
  if (int rc = set_device(c)) return rc;
  if (int rc = ggp_reserve(c, 1)) return rc;
  GgpRun run;
  if (int rc = ggp_newton(GgpLane(c, 1), p, tol, max_iter, run)) return rc;
  ggp_report(run, logq, out_iters, info);
  return GPMI_OK;
}

int gpmi_ggp_logq_grad(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double tol, int max_iter, double* logq,
                       double* grad, int* out_iters, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = ggp_eval_args(c, "gpmi_ggp_logq_grad", kernel, theta, n_theta, tol, max_iter, logq, out_iters, info, p))
    return rc;
  ARGCHK(c, grad != nullptr, "grad is NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = ggp_reserve(c, 1)) return rc;
  const GgpLane g(c, 1);
  {
    Lane& L0 = g.L();
    if (int rc = ensure_second_matrix(c, L0)) return rc;
    if (int rc = L0.gws.reserve(c, grad_ws_doubles(c->np, n_theta))) return rc;
    if (int rc = ensure_trsm_panel(c, c->np)) return rc;
  }
  GgpRun run;
  if (int rc = ggp_newton(g, p, tol, max_iter, run)) return rc;
  ggp_report(run, logq, out_iters, info);
  if (run.info != 0) return GPMI_OK;
  Lane& L = g.L();
  hipStream_t s = L.stream;
  const int64_t np = c->np;
  const int nt = (int)(np / GPMI_NB);
  double* gout = L.red + 16;
  {
    ProfScope ps(c, s, GPMI_PROF_GGP_GRAD, 0.0, 0.0);
    // post = diag K - diag(K R K), diag(K R K)_i = |L^-1 (sw o K[:, i])|^2: the rows of K, columns scaled by sw, solved in
    // place in the second matrix while the lane's matrix still holds L
    if (int rc = ensure_inv2(c, L, s)) return rc;
    launch_scale_columns(s, g.K(), g.vec(GV_SW), L.B2, c->ld, np);
    trsm_rows_forward(c, s, L.A, np, c->ld, L.inv2, L.B2, np, false, nullptr, c->trsm_panel);
    launch_rows_sumsq(s, L.B2, c->ld, np, np, 0.0, g.vec(GV_T1), 1, 0, 0, -1.0);  // (-(0 - sum): the sum itself)
    launch_ggp_s2(s, g.K(), c->ld, g.vec(GV_T1), g.vec(GV_D3), g.vec(GV_S2), np);
    // B^-1 = L^-T L^-1 over L (lower tiles, mirrored), R = sw sw^T o B^-1 into the second matrix
    if (int rc = enqueue_inverse_factor(c, L, L)) return rc;
    launch_gemm(s, TILES_LOWER, OP_ASSIGN, false, 1, L.A, c->ld, L.B2, c->ld, L.B2, c->ld, nt, nt, (int)np);
    L.inv2_valid = false;  // (the lane's matrix no longer holds the factor)
    launch_mirror_lower(s, L.A, c->ld, np);
    launch_scale_add(s, L.B2, c->ld, L.A, c->ld, g.vec(GV_SW), g.vec(GV_SW), np, np, false);
    // w = s2 - R (K s2), u = g + 2 w
    ggp_kv1(g, g.K(), g.vec(GV_S2), g.vec(GV_KS2));
    ggp_kv1(g, L.B2, g.vec(GV_KS2), g.vec(GV_T2));
    launch_ggp_grad_u(s, g.vec(GV_G), g.vec(GV_S2), g.vec(GV_T2), g.vec(GV_U), np);
    launch_lml_grad(s, p, n_theta, c->x, c->n, np, L.B2, c->ld, g.vec(GV_U), g.vec(GV_G), L.gws, gout);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(L.h_red + 16, gout, sizeof(double) * n_theta, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(L.h_info, L.info, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  INFOCHK(c, L.h_info[0]);
  for (int j = 0; j < n_theta; ++j) grad[j] = L.h_red[16 + j];
  return GPMI_OK;
}

int gpmi_ggp_mode(gpmi_ctx* c, double* f_host, double* g_host) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = ggp_check_fit(c, "gpmi_ggp_mode")) return rc;
  ARGCHK(c, f_host && g_host, "f_host / g_host is NULL");
  if (int rc = set_device(c)) return rc;
  const GgpLane g(c, 0);
  hipStream_t s = g.L().stream;
  HIPCHK(c, hipMemcpyAsync(f_host, g.vec(GV_FM), sizeof(double) * c->n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(g_host, c->alpha, sizeof(double) * c->n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (int64_t i = 0; i < c->n; ++i) f_host[i] += c->ggp_offset;
  return GPMI_OK;
}

int gpmi_ggp_predict(gpmi_ctx* c, const double* pts, int64_t m, double* mean_host, double* var_host) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = ggp_check_fit(c, "gpmi_ggp_predict")) return rc;
  ARGCHK(c, pts && m > 0 && mean_host, "pts / mean_host is NULL or m <= 0");
  if (int rc = set_device(c)) return rc;
  if (int rc = c->ggMean.reserve(c, 2048)) return rc;
  const GgpLane g(c, 0);
  hipStream_t s = g.L().stream;
  const CovParams& p = c->fit_params;
  auto fill = [&](int64_t m0, int64_t mc, int64_t mp) -> int {
    HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * c->d, sizeof(double) * mc * c->d, hipMemcpyHostToDevice, s));
    {
      ProfScope ps(c, s, GPMI_PROF_KBUILD, 0.0, 8.0 * mp * c->np);
      launch_kbuild_cross(s, p, c->pts, mc, mp, c->x, c->n, c->np, c->Q, c->ld);
    }
    // the chunk's means from the unscaled cross-covariances, k(q)^T g; then their columns times sw for the variance
    launch_rows_dot(s, c->Q, c->ld, mp, c->np, c->alpha, c->ggMean);
    HIPCHK(c, hipMemcpyAsync(mean_host + m0, c->ggMean, sizeof(double) * mc, hipMemcpyDeviceToHost, s));
    launch_ggp_scale_cols(s, c->Q, c->ld, mp, c->np, g.vec(GV_SW));
    return GPMI_OK;
  };
  if (int rc = predict_rows(c, m, fill, p.a2, nullptr, var_host)) return rc;
  if (!var_host) HIPCHK(c, hipStreamSynchronize(s));
  for (int64_t q = 0; q < m; ++q) mean_host[q] += c->ggp_offset;
  return GPMI_OK;
}

int gpmi_ggp_kv(gpmi_ctx* c, int kernel, const double* theta, int n_theta, const double* V_host, int nv, double* Y_host,
                int reps, float* ms) {
  if (!c) return GPMI_ERR_ARG;
  if (int rc = ggp_check(c, "gpmi_ggp_kv")) return rc;
  CovParams p;
  NO_PERIODIC(c, kernel);
  if (int rc = make_params(c, kernel, theta, n_theta, 0.0, p)) return rc;
  ARGCHK(c, V_host && Y_host, "V_host / Y_host is NULL");
  ARGCHK(c, nv >= 1 && nv <= 4 && reps >= 1, "gpmi_ggp_kv: nv outside 1 .. 4 or reps < 1");
  if (int rc = set_device(c)) return rc;
  if (int rc = ggp_reserve(c, 1)) return rc;
  const GgpLane g(c, 1);
  hipStream_t s = g.L().stream;
  const int64_t np = c->np;
  ggp_build_k(g, p);
  HIPCHK(c, hipMemsetAsync(g.vec(0), 0, sizeof(double) * 8 * np, s));
  GgpKv a{};
  for (int q = 0; q < nv; ++q) {
    HIPCHK(c, hipMemcpyAsync(g.vec(q), V_host + (int64_t)q * c->n, sizeof(double) * c->n, hipMemcpyHostToDevice, s));
    a.v[q] = g.vec(q);
    a.y[q] = g.vec(4 + q);
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ms) {
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipEventRecord(e0, s));
  }
  for (int r = 0; r < reps; ++r) ggp_kv(g, g.K(), nv, a);
  if (ms) HIPCHK(c, hipEventRecord(e1, s));
  HIPCHK(c, hipGetLastError());
  for (int q = 0; q < nv; ++q)
    HIPCHK(c, hipMemcpyAsync(Y_host + (int64_t)q * c->n, g.vec(4 + q), sizeof(double) * c->n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (ms) {
    HIPCHK(c, hipEventElapsedTime(ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return GPMI_OK;
}

}  // extern "C"
