// C-ABI of libgpmi (include/gpmi.h): gpmi_lml_hessian - the log-marginal likelihood, its gradient and its exact Hessian
// by the mean's, the kernel's and the WhiteNoise parameters from ONE factorisation on lane 1.  The kernels and the formula:
// hessian.hip; the stages up to K^-1: api_single.hip (lane_stages), shared with gpmi_lml_grad.
#include "api_internal.h"

namespace {

// GPMI_HESS_GIB: the cap of the Hessian's matrix workspace in GiB (fractions allowed; 0 < v <= 200, else and by default
// 24).  Read at every call: a caller may change it between calls.
int64_t hess_budget_bytes() {
  const char* e = std::getenv("GPMI_HESS_GIB");
  double v = e ? std::atof(e) : 24.0;
  if (!(v > 0.0 && v <= 200.0)) v = 24.0;
  return (int64_t)(v * 1073741824.0);
}

// offsets of the sums in hPart behind the partials, in the order they are copied to the host
struct HessSums {
  int PT, nent, n_mean;
  int64_t trace() const { return 0; }                           // PT x PT: T_ij, i <= j
  int64_t wz() const { return (int64_t)PT * PT; }               // PT x PT: (D_i alpha) . z_j, i <= j
  int64_t contract() const { return 2 * (int64_t)PT * PT; }     // nent second-derivative contractions
  int64_t phi_kphi() const { return contract() + nent; }        // n_mean x n_mean: phi_p . K^-1 phi_q, p <= q
  int64_t phi_z() const { return phi_kphi() + (int64_t)n_mean * n_mean; }  // n_mean x PT: phi_p . z_j
  int64_t total() const { return phi_z() + (int64_t)n_mean * PT; }
};

}  // namespace

extern "C" {

int gpmi_lml_hessian(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag, const double* mu,
                     const double* phi, int n_mean, double* lml, double* grad, double* hess, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, kernel != GPMI_KERNEL_SUM && c->sum_nk == 0,
         "gpmi_lml_hessian does not take sums of kernels (GPMI_KERNEL_SUM, gpmi_set_sum): difference gpmi_lml_grad instead");
  KParams p;
  NO_PERIODIC(c, kernel);
  if (int rc = make_params(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, !c->ycov, "gpmi_lml_hessian needs diagonal data errors (no dense y covariance)");
  ARGCHK(c, extra_diag >= 0.0 && std::isfinite(extra_diag), "extra_diag must be finite and >= 0");
  ARGCHK(c, mu && lml && grad && hess, "mu / lml / grad / hess is NULL");
  ARGCHK(c, n_mean >= 0 && n_mean <= 1 + 2 * GPMI_MAX_D && (n_mean == 0 || phi), "n_mean out of range, or phi is NULL");
  const int64_t np = c->np, ld = c->ld, sMat = np * ld;
  const int PT = n_theta + (extra_diag > 0.0 ? 1 : 0);  // parameters with a derivative matrix
  // groups: per parameter D_i, G_i and - beyond one group - the G_j of the group it is paired with
  int gsz = (int)std::min<int64_t>(PT, hess_budget_bytes() / (3 * sMat * (int64_t)sizeof(double)));
  ARGCHK(c, gsz >= 1,
         "gpmi_lml_hessian: three n x n matrices (one parameter's group) do not fit the workspace cap GPMI_HESS_GIB");
  const bool grouped = gsz < PT;
  const CovParams cp(p);
  const HessSums hs{PT, hess_contract_entries(kernel, p.d), n_mean};
  const int nt64 = (int)(np / 64);
  const int64_t part_trace = (int64_t)PT * PT * nt64, part_contract = hess_contract_ws_doubles(np, kernel, p.d);
  if (int rc = set_device(c)) return rc;
  if (int rc = c->hD.reserve(c, gsz * sMat)) return rc;
  if (int rc = c->hGa.reserve(c, gsz * sMat)) return rc;
  if (grouped)
    if (int rc = c->hGb.reserve(c, gsz * sMat)) return rc;
  if (int rc = c->hVec.reserve(c, (2 * (int64_t)PT + 2 * n_mean) * np)) return rc;
  if (int rc = c->hPart.reserve(c, part_trace + part_contract + hs.total())) return rc;
  if (int rc = c->h_hOut.reserve(c, hs.total())) return rc;
  const LaneEval ev(c, 1);
  // K^-1 in both triangles: the products need all its tiles
  if (int rc = lane_stages(ev, LaneBuild::kernels(cp), LN_BACKWARD | LN_INVERSE | LN_SYRK | LN_MIRROR, mu, n_theta)) return rc;
  hipStream_t s = ev.stream();
  const double* iK = ev.L().A;
  const double* alpha = ev.alpha();
  launch_lml_grad(s, cp, n_theta, c->x, c->n, np, iK, ld, alpha, alpha, ev.partial(false), ev.gout());
  double* W = c->hVec;                   // D_i alpha
  double* Z = W + (int64_t)PT * np;      // z_i = G_i alpha
  double* Phi = Z + (int64_t)PT * np;    // the mean's features, zero padded
  double* KPhi = Phi + (int64_t)n_mean * np;
  double* tpart = c->hPart;
  double* cws = tpart + part_trace;
  double* sums = cws + part_contract;
  const int nt = (int)(np / GPMI_NB);
  const double gemm_flops = 2.0 * (double)np * (double)np * (double)np, mat_bytes = 8.0 * (double)np * (double)np;
  auto build = [&](int p0, int cnt, bool vectors) {
    ProfScope ps(c, s, GPMI_PROF_HESS_BUILD, 0.0, mat_bytes * cnt * (vectors ? 2.0 : 1.0));
    launch_hess_dbuild(s, p, n_theta, p0, cnt, c->x, c->n, np, c->hD, ld, sMat);
    if (vectors)
      for (int m = 0; m < cnt; ++m) launch_rows_dot(s, c->hD + m * sMat, ld, np, np, alpha, W + (int64_t)(p0 + m) * np);
  };
  auto products = [&](double* G, int p0, int cnt, bool vectors) {
    ProfScope ps(c, s, GPMI_PROF_HESS_GEMM, gemm_flops * cnt, 3.0 * mat_bytes * cnt);
    for (int m = 0; m < cnt; ++m) {
      launch_gemm_nt(s, TILES_RECT, OP_ASSIGN, G + m * sMat, ld, iK, ld, c->hD + m * sMat, ld, nt, nt, (int)np);
      if (vectors) launch_rows_dot(s, G + m * sMat, ld, np, np, alpha, Z + (int64_t)(p0 + m) * np);
    }
  };
  auto traces = [&](int a0, int na, const double* GB, int b0, int nb) {
    ProfScope ps(c, s, GPMI_PROF_HESS_TRACE, 2.0 * np * np * na * nb, mat_bytes * na * (nb + (nb + 3) / 4));
    launch_hess_pair_trace(s, c->hGa, a0, na, GB, b0, nb, np, ld, sMat, PT, tpart);
  };
  for (int a0 = 0; a0 < PT; a0 += gsz) {
    const int na = std::min(gsz, PT - a0);
    build(a0, na, true);
    products(c->hGa, a0, na, true);
    traces(a0, na, c->hGa, a0, na);
    for (int b0 = a0 + gsz; b0 < PT; b0 += gsz) {  // (the later groups' products are formed again for every group a)
      const int nb = std::min(gsz, PT - b0);
      build(b0, nb, false);
      products(c->hGb, b0, nb, false);
      traces(a0, na, c->hGb, b0, nb);
    }
  }
  launch_hess_trace_sum(s, tpart, PT, np, sums + hs.trace());
  launch_hess_dots(s, W, PT, Z, PT, np, true, sums + hs.wz());
  {
    ProfScope ps(c, s, GPMI_PROF_HESS_CONTRACT, 0.0, mat_bytes * 0.5);
    if (int rc = launch_hess_contract(c, s, p, c->x, c->n, np, iK, ld, alpha, cws, sums + hs.contract())) return rc;
  }
  if (n_mean > 0) {
    HIPCHK(c, hipMemsetAsync(Phi, 0, sizeof(double) * n_mean * np, s));
    HIPCHK(c, hipMemcpy2DAsync(Phi, sizeof(double) * np, phi, sizeof(double) * c->n, sizeof(double) * c->n, n_mean,
                               hipMemcpyHostToDevice, s));
    for (int q = 0; q < n_mean; ++q) launch_rows_dot(s, iK, ld, np, np, Phi + (int64_t)q * np, KPhi + (int64_t)q * np);
    launch_hess_dots(s, Phi, n_mean, KPhi, n_mean, np, true, sums + hs.phi_kphi());
    launch_hess_dots(s, Phi, n_mean, Z, PT, np, false, sums + hs.phi_z());
  }
  HIPCHK(c, hipMemcpyAsync(c->h_hOut, sums, sizeof(double) * hs.total(), hipMemcpyDeviceToHost, s));
  double lml_v = 0.0;
  int inf = 0;
  if (int rc = lane_collect(ev, LC_LML_RAW, n_theta + 1, {}, &lml_v, &inf)) return rc;
  if (info) *info = inf;
  if (inf != 0) return GPMI_OK;  // K does not factorise: the outputs are untouched
  const double* g = ev.h_gout();
  const double* h = c->h_hOut;
  const double grad_sigma = extra_diag * g[n_theta];  // 1/2 sum Q o (2 sigma^2 I) = sigma^2 tr Q
  *lml = lml_v;
  for (int j = 0; j < n_theta; ++j) grad[j] = g[j];
  grad[n_theta] = extra_diag > 0.0 ? grad_sigma : 0.0;
  const int NH = n_mean + n_theta + 1, off = kernel_theta_offset(kernel), d = p.d;
  std::fill(hess, hess + (size_t)NH * NH, 0.0);
  auto S = [&](int k, int m) { return h[hs.contract() + (int64_t)k * d - (int64_t)k * (k - 1) / 2 + (m - k)]; };
  // 1/2 sum Q o D_ij for i <= j: multiples of the gradient where D_ij is a multiple of a first derivative
  auto first_term = [&](int i, int j) -> double {
    if (i == n_theta) return 2.0 * grad_sigma;  // D = 4 sigma^2 I
    if (j == n_theta) return 0.0;               // the noise has no mixed second derivatives
    if (i == 0) return 2.0 * g[j];              // d2K / d ln a d theta_j = 2 dK / d theta_j; d2K / d ln a^2 = 4 K
    if (off == 2 && i == 1) return j == 1 ? h[hs.contract() + d * (d + 1) / 2 + d] : h[hs.contract() + d * (d + 1) / 2 + (j - 2)];
    const int k = i - off, m = j - off;
    return S(k, m) - (k == m ? 2.0 * g[i] : 0.0);
  };
  for (int i = 0; i < PT; ++i)
    for (int j = i; j < PT; ++j) {
      const double v = first_term(i, j) - h[hs.wz() + (int64_t)i * PT + j] + 0.5 * h[hs.trace() + (int64_t)i * PT + j];
      hess[(size_t)(n_mean + i) * NH + n_mean + j] = v;
      hess[(size_t)(n_mean + j) * NH + n_mean + i] = v;
    }
  for (int pq = 0; pq < n_mean; ++pq) {
    for (int q = pq; q < n_mean; ++q) {
      const double v = -h[hs.phi_kphi() + (int64_t)pq * n_mean + q];
      hess[(size_t)pq * NH + q] = v;
      hess[(size_t)q * NH + pq] = v;
    }
    for (int j = 0; j < PT; ++j) {
      const double v = -h[hs.phi_z() + (int64_t)pq * PT + j];
      hess[(size_t)pq * NH + n_mean + j] = v;
      hess[(size_t)(n_mean + j) * NH + pq] = v;
    }
  }
  return GPMI_OK;
}

int gpmi_lml_hessian_alpha(gpmi_ctx* c, double* alpha_host) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, alpha_host != nullptr, "alpha is NULL");
  ARGCHK(c, c->lanes.size() >= 2 && c->lanes[1].vec, "gpmi_lml_hessian has not been called");
  if (int rc = set_device(c)) return rc;
  const LaneEval ev(c, 1);
  HIPCHK(c, hipMemcpyAsync(alpha_host, ev.alpha(), sizeof(double) * c->n, hipMemcpyDeviceToHost, ev.stream()));
  HIPCHK(c, hipStreamSynchronize(ev.stream()));
  return GPMI_OK;
}

}  // extern "C"
