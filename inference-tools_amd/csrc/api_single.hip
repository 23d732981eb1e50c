// What the single-evaluation entry points of api_regression.hip, api_mix.hip and api_dense.hip share (one problem on one
// lane, any size): the stages from the upload of the prior mean to K^-1, the leave-one-out middle part, and the copies,
// sync and info check at the end.  Host code only.  The views and the fitted lane's query pipelines (predict_rows,
// posterior_sigma) are in api_internal.h.
#include "api_internal.h"

// A <- B2 B2^T, lower tiles (kskip: launch_gemm)
static void lane_syrk(gpmi_ctx* c, Lane& L, int kskip) {
  const int nt = (int)(c->np / GPMI_NB);
  launch_gemm(L.stream, TILES_LOWER, OP_ASSIGN, false, kskip, L.A, c->ld, L.B2, c->ld, L.B2, c->ld, nt, nt, (int)c->np);
}

int lane_prepare(const LaneEval& ev, unsigned steps, int n_theta) {
  gpmi_ctx* c = ev.c;
  if (int rc = ensure_lanes(c, (size_t)ev.lane + 1)) return rc;
  Lane& L = ev.L();
  if (steps & LN_INVERSE)
    if (int rc = ensure_second_matrix(c, L)) return rc;
  const int64_t want = (n_theta >= 0 ? grad_ws_doubles(c->np, n_theta) : 0) + ((steps & LN_LOO) ? 4 * c->np : 0);
  return L.gws.reserve(c, want);
}

int lane_forward(const LaneEval& ev, const LaneBuild& b, unsigned steps, const double* mu_host, int n_theta) {
  gpmi_ctx* c = ev.c;
  if (int rc = lane_prepare(ev, steps, n_theta)) return rc;
  Lane& L = ev.L();
  const bool fit = (steps & LN_FIT_SCHEDULE) != 0;
  if (ev.lane == 0) c->mt_fitted = c->ggp_fitted = false;  // lane 0 gets another factor: gpmi_mt_fit says so again if it is the caller
  HIPCHK(c, hipMemcpyAsync(ev.mu(), mu_host, sizeof(double) * c->n, hipMemcpyHostToDevice, L.stream));
  if (b.dense) {
    if (int rc = upload_dense_matrix(c, L, b.dense)) return rc;
    if (int rc = enqueue_dense_factor_and_forward(c, L, ev.mu(), 0)) return rc;
  } else {
    // the kernel build writes the identity L^-T is solved from beside the factorisation; the fit's backward sweep finds
    // its sentinel in alpha() already (enqueue_factor_and_forward: early_identity, backward_out)
    double* ident = (b.p && (steps & LN_INVERSE)) ? L.B2 : nullptr;
    if (int rc = enqueue_factor_and_forward(c, L, b.p ? *b.p : CovParams(b.mix->p[0]), ev.mu(), 0.0, 0, true, b.mix, fit,
                                            fit ? ev.alpha() : nullptr, ident))
      return rc;
  }
  if (ev.times) ev.times->forward = std::chrono::steady_clock::now();
  return GPMI_OK;
}

int lane_solves(const LaneEval& ev, unsigned steps) {
  gpmi_ctx* c = ev.c;
  Lane& L = ev.L();
  hipStream_t s = L.stream;
  const bool fit = (steps & LN_FIT_SCHEDULE) != 0;
  if (steps & LN_BACKWARD) trsv_backward(c, s, L.A, c->np, c->ld, L.invD, ev.v(), ev.alpha(), L.info, BatchShape(), fit);
  if (fit && L.inv2_valid) HIPCHK(c, hipStreamWaitEvent(s, L.ev_main, 0));  // (the inverse blocks built beside the sweeps)
  if (steps & LN_INVERSE)
    if (int rc = enqueue_inverse_factor(c, L, L)) return rc;
  // K^-1 = L^-T L^-1 (regression.py:556-557) by the k-skipped SYRK, lower tiles, overwriting L
  if (steps & LN_SYRK) lane_syrk(c, L, 1);
  if (steps & LN_MIRROR) launch_mirror_lower(s, L.A, c->ld, c->np);
  return GPMI_OK;
}

void lane_loo_middle(const LaneEval& ev, bool want_p, bool want_M, bool mirror_M) {
  gpmi_ctx* c = ev.c;
  Lane& L = ev.L();
  hipStream_t s = L.stream;
  // diag(K^-1)_a = squared norm of row a of L^-T (regression.py:503); rows_sumsq returns base - sum
  launch_rows_sumsq(s, L.B2, c->ld, c->np, c->np, 0.0, ev.loo_diag());
  launch_negate(s, ev.loo_diag(), c->np);
  if (!want_p && !want_M) return;
  lane_syrk(c, L, 1);  // K^-1 in full (both triangles)
  launch_mirror_lower(s, L.A, c->ld, c->np);
  launch_loo_vectors(s, ev.alpha(), ev.loo_diag(), ev.loo_c1(), ev.loo_sc2(), c->n, c->np);
  // p = K^-1 c1  (regression.py:512-513, 518-519 folded: c1^T K^-1 dK_j alpha = p^T dK_j alpha)
  launch_rows_dot(s, L.A, c->ld, c->np, c->np, ev.loo_c1(), ev.loo_p());
  if (!want_M) return;
  // M = K^-1 diag(c2) K^-1 = G G^T with G = K^-1 diag(sqrt c2); lower tiles, overwriting K^-1
  launch_scale_columns(s, L.A, ev.loo_sc2(), L.B2, c->ld, c->np);
  lane_syrk(c, L, 0);
  if (mirror_M) launch_mirror_lower(s, L.A, c->ld, c->np);
}

int lane_loo_terms(const LaneEval& ev, const LaneBuild& b, const double* mu_host, double* alpha_out, double* ikdiag, int* info) {
  gpmi_ctx* c = ev.c;
  if (int rc = lane_stages(ev, b, LN_BACKWARD | LN_INVERSE, mu_host)) return rc;
  launch_rows_sumsq(ev.stream(), ev.L().B2, c->ld, c->np, c->np, 0.0, ev.slot2());  // -diag(K^-1): squared row norms of L^-T
  const int rc = lane_collect(ev, 0, 0, {{alpha_out, ev.alpha()}, {ikdiag, ev.slot2()}}, nullptr, info);
  for (int64_t i = 0; i < c->n; ++i) ikdiag[i] = -ikdiag[i];
  return rc;
}

int lane_collect(const LaneEval& ev, unsigned what, int n_gout, std::initializer_list<LaneVec> vecs, double* value, int* info) {
  gpmi_ctx* c = ev.c;
  Lane& L = ev.L();
  hipStream_t s = L.stream;
  HIPCHK(c, hipGetLastError());
  if (what) HIPCHK(c, hipMemcpyAsync(L.h_red, L.red, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (n_gout > 0) HIPCHK(c, hipMemcpyAsync(L.h_red + 16, ev.gout(), sizeof(double) * n_gout, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(L.h_info, L.info, sizeof(int), hipMemcpyDeviceToHost, s));
  for (const LaneVec& v : vecs)
    if (v.host) HIPCHK(c, hipMemcpyAsync(v.host, v.dev, sizeof(double) * c->n, hipMemcpyDeviceToHost, s));
  if (ev.times) ev.times->enqueued = std::chrono::steady_clock::now();
  HIPCHK(c, hipStreamSynchronize(s));
  if (ev.times) ev.times->done = std::chrono::steady_clock::now();
  const int inf = L.h_info[0];
  // -1/2 v.v - sum ln L_ii (regression.py:539)
  const double lml = -0.5 * L.h_red[0] - L.h_red[1];
  if ((what & LC_LOGDET) && value) *value = L.h_red[1];
  if (what & LC_LML_RAW) *value = lml;
  INFOCHK(c, inf);
  if (what & LC_LML) *value = (inf == 0) ? lml : -1e50;  // sentinel on failure (regression.py:540-542)
  if (info) *info = inf;
  return GPMI_OK;
}

int kernel_posterior_sigma(gpmi_ctx* c, const double* pts, int64_t m, int64_t mp, double* mu_out, double* Sigma, int64_t ldq) {
  hipStream_t s = c->lanes[0].stream;
  const CovParams& p = c->fit_params;
  auto cross = [&]() -> int {
    HIPCHK(c, hipMemcpyAsync(c->pts, pts, sizeof(double) * m * c->d, hipMemcpyHostToDevice, s));
    launch_kbuild_cross(s, p, c->pts, m, mp, c->x, c->n, c->np, c->Q, c->ld);
    return GPMI_OK;
  };
  auto qq = [&] { launch_kbuild_cross(s, p, c->pts, m, mp, c->pts, m, mp, Sigma, ldq); };  // no jitter (regression.py:441)
  return posterior_sigma(c, cross, qq, m, mp, mu_out, Sigma, ldq);
}
