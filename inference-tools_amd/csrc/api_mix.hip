// C-ABI of libgpmi (include/gpmi.h): mixture covariance (ChangePoint) and per-point noise hyper-parameters (HeteroscedasticNoise).
// (split from api.hip in round 4; the handle, the lanes and the helpers these entry points are built from: api.hip,
// api_internal.h; the pipeline of the single evaluations: api_single.hip)
#include "api_internal.h"

// ---- mixture covariance (ChangePoint) -------------------------------------------------------------------
namespace {

// parse the sub-kernels, upload the weights: fills ps[nk] and the device buffers of the context
int mix_prepare(gpmi_ctx* c, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                const double* g_host, KParams* ps) {
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, nk >= 1 && nk <= GPMI_MAX_MIX, "number of sub-kernels out of range (1..4)");
  ARGCHK(c, kernels && thetas && n_thetas && g_host, "NULL argument");
  int off = 0;
  for (int m = 0; m < nk; ++m) {
    NO_PERIODIC(c, kernels[m]);
    if (int rc = make_params(c, kernels[m], thetas + off, n_thetas[m], 0.0, ps[m])) return rc;
    off += n_thetas[m];
  }
  if (int rc = set_device(c)) return rc;
  if (!c->mix_g)
    if (int rc = c->mix_g.alloc(c, GPMI_MAX_MIX * c->np)) return rc;
  if (!c->mix_scratch)
    if (int rc = c->mix_scratch.alloc(c, c->np * c->ld)) return rc;
  if (!c->mix_zero)
    if (int rc = c->mix_zero.alloc_zeroed(c, c->np)) return rc;
  if (int rc = gpmi_sync(c)) return rc;  // nothing may still be reading the previous weights
  std::vector<double> g((size_t)nk * c->np);
  for (int m = 0; m < nk; ++m)
    for (int64_t i = 0; i < c->np; ++i)
      g[(size_t)m * c->np + i] = i < c->n ? g_host[(size_t)m * c->n + i] : (m == 0 ? 1.0 : 0.0);
  HIPCHK(c, hipMemcpy(c->mix_g, g.data(), sizeof(double) * nk * c->np, hipMemcpyHostToDevice));
  return GPMI_OK;
}

int ensure_q3(gpmi_ctx* c) { return c->Q3.reserve(c, c->mq_cap * c->ld); }

// Rows [m0, m0 + mc) of the m query points and of their nk x m weights gq_host to the device (the weights to gq_dev =
// c->pvec + 2 mp: nk x mp, zero-padded; pvec holds mp (2 + 2 d + d^2 + 4) doubles), then
// c->Q (mp x ld) = sum_m diag(gq_m) K_m(pts, x) diag(g_m)
int upload_and_build_mix_cross(gpmi_ctx* c, const double* pts, const double* gq_host, int64_t m, int64_t m0, int64_t mc,
                               int64_t mp) {
  hipStream_t s = c->lanes[0].stream;
  if (int rc = ensure_q3(c)) return rc;
  double* gq_dev = c->pvec + 2 * mp;
  HIPCHK(c, hipMemsetAsync(gq_dev, 0, sizeof(double) * c->mix_nk * mp, s));
  HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * c->d, sizeof(double) * mc * c->d, hipMemcpyHostToDevice, s));
  for (int k = 0; k < c->mix_nk; ++k)
    HIPCHK(c, hipMemcpyAsync(gq_dev + (int64_t)k * mp, gq_host + (int64_t)k * m + m0, sizeof(double) * mc,
                             hipMemcpyHostToDevice, s));
  for (int k = 0; k < c->mix_nk; ++k) {
    launch_kbuild_cross(s, c->mix_p[k], c->pts, mc, mp, c->x, c->n, c->np, c->Q3, c->ld);
    launch_scale_add(s, c->Q, c->ld, c->Q3, c->ld, gq_dev + (int64_t)k * mp, c->mix_g + (int64_t)k * c->np, mp, c->np, k > 0);
  }
  return GPMI_OK;
}

}  // namespace

extern "C" {

int gpmi_fit_mix(gpmi_ctx* c, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                 const double* g_host, double extra_diag, const double* mu, double* alpha_out,
                 double* logdet_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  KParams ps[GPMI_MAX_MIX];
  if (int rc = mix_prepare(c, nk, kernels, thetas, n_thetas, g_host, ps)) return rc;
  ARGCHK(c, mu != nullptr, "mu is NULL");
  const LaneEval ev(c, 0);
  const MixEval mx{nk, ps, c->mix_g, extra_diag, c->mix_scratch, c->mix_zero};
  if (int rc = lane_stages(ev, LaneBuild::mixture(mx), LN_BACKWARD, mu)) return rc;
  int inf = 0;
  if (int rc = lane_collect(ev, LC_LOGDET, 0, {{alpha_out, ev.alpha()}}, logdet_out, &inf)) return rc;
  if (info) *info = inf;
  c->mix_nk = nk;
  for (int m = 0; m < nk; ++m) c->mix_p[m] = ps[m];
  c->fit_params = CovParams(ps[0]);
  c->fitted = (inf == 0);
  return GPMI_OK;
}

int gpmi_lml_mix(gpmi_ctx* c, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                 const double* g_host, double extra_diag, const double* mu, double* lml, int* info) {
  if (!c) return GPMI_ERR_ARG;
  KParams ps[GPMI_MAX_MIX];
  // the weights of a fitted mixture live in the same device buffer: an evaluation at other hyper-parameters
  // invalidates them for gpmi_predict_mix until the next gpmi_fit_mix (the host wrapper re-fits lazily)
  if (int rc = mix_prepare(c, nk, kernels, thetas, n_thetas, g_host, ps)) return rc;
  ARGCHK(c, mu && lml, "mu / lml is NULL");
  c->fitted = false;
  const LaneEval ev(c, 1);
  const MixEval mx{nk, ps, c->mix_g, extra_diag, c->mix_scratch, c->mix_zero};
  if (int rc = lane_stages(ev, LaneBuild::mixture(mx), 0, mu)) return rc;
  return lane_collect(ev, LC_LML, 0, {}, lml, info);
}

int gpmi_lml_grad_mix(gpmi_ctx* c, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                      const double* g_host, const double* hw_host, double extra_diag, const double* mu, double* lml,
                      double* grad_thetas, double* hrows, double* alpha_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  KParams ps[GPMI_MAX_MIX];
  if (int rc = mix_prepare(c, nk, kernels, thetas, n_thetas, g_host, ps)) return rc;
  ARGCHK(c, mu && lml && grad_thetas && hrows, "mu / lml / grad_thetas / hrows is NULL");
  c->fitted = false;
  const LaneEval ev(c, 1);
  int max_nt = 0;
  for (int m = 0; m < nk; ++m) max_nt = n_thetas[m] > max_nt ? n_thetas[m] : max_nt;
  // row sums (nk x np, or nk x 2 x np with the caller's own weights hw behind them): the scratch matrix is free once
  // K is factorised
  const int nrow = hw_host ? 2 : 1;
  double* hdev = c->mix_scratch;
  double* wdev = c->mix_scratch + (int64_t)2 * GPMI_MAX_MIX * c->np;
  const MixEval mx{nk, ps, c->mix_g, extra_diag, c->mix_scratch, c->mix_zero};
  // K^-1 = L^-T L^-1, lower tiles over L, then both triangles (it is read row-wise below)
  const unsigned steps = LN_BACKWARD | LN_INVERSE | LN_SYRK | LN_MIRROR;
  if (int rc = lane_forward(ev, LaneBuild::mixture(mx), steps, mu, max_nt)) return rc;
  Lane& L = ev.L();
  hipStream_t s = L.stream;
  double* alpha_dev = ev.alpha();
  double* ua = ev.slot2();     // g_m o alpha
  double* gout = ev.gout();    // (n_theta_m + 1) values per sub-kernel, consecutive
  if (hw_host) {
    HIPCHK(c, hipMemsetAsync(wdev, 0, sizeof(double) * 2 * nk * c->np, s));
    HIPCHK(c, hipMemcpy2DAsync(wdev, sizeof(double) * c->np, hw_host, sizeof(double) * c->n, sizeof(double) * c->n,
                               (size_t)2 * nk, hipMemcpyHostToDevice, s));
  }
  if (int rc = lane_solves(ev, steps)) return rc;
  int goff = 0;
  for (int m = 0; m < nk; ++m) {
    const double* gm = c->mix_g + (int64_t)m * c->np;
    // sub-kernel parameters: 1/2 sum Q o (D_m dK_m D_m) = 1/2 sum (D_m Q D_m) o dK_m, the fused contraction on
    // the scaled inverse with u = v = g_m o alpha
    launch_scale_add(s, L.B2, c->ld, L.A, c->ld, gm, gm, c->np, c->np, false);
    launch_vec_mul(s, gm, alpha_dev, ua, c->np);
    launch_lml_grad(s, ps[m], n_thetas[m], c->x, c->n, c->np, L.B2, c->ld, ua, ua, ev.partial(false), gout + goff);
    goff += n_thetas[m] + 1;
    // window parameters: h_m(i) = sum_j Q_ij K_m,ij g_m(j)  (the host contracts it with d g_m / d phi)
    KParams pm = ps[m];
    pm.extra_diag = 0.0;
    launch_kbuild_square(s, pm, c->x, c->n, c->np, c->mix_zero, L.B2, c->ld, false);
    // (the caller's two window factors of a sub-kernel - rows 2 m, 2 m + 1, np apart - in one pass)
    if (hw_host)
      launch_mix_rowsum(s, L.A, L.B2, c->ld, alpha_dev, wdev + (int64_t)m * 2 * c->np, hdev + (int64_t)m * 2 * c->np, c->n, 1, 0,
                        0, 0, nullptr, 0, c->np);
    else
      launch_mix_rowsum(s, L.A, L.B2, c->ld, alpha_dev, gm, hdev + (int64_t)m * c->np, c->n);
  }
  HIPCHK(c, hipGetLastError());
  for (int row = 0; row < nk * nrow; ++row)
    HIPCHK(c, hipMemcpyAsync(hrows + (int64_t)row * c->n, hdev + (int64_t)row * c->np, sizeof(double) * c->n,
                             hipMemcpyDeviceToHost, s));
  const int rc = lane_collect(ev, LC_LML_RAW, goff, {{alpha_out, alpha_dev}}, lml, info);
  goff = 0;
  int o = 0;
  for (int m = 0; m < nk; ++m) {
    for (int j = 0; j < n_thetas[m]; ++j) grad_thetas[o++] = ev.h_gout()[goff + j];
    goff += n_thetas[m] + 1;
  }
  return rc;
}

// gpmi_lml_grad_mix for T hyper-parameter vectors at once (round 4).  For N <= 4096 the evaluations advance in lockstep:
// every sub-kernel build and fold, the factorisation, both sweeps, L^-T, the k-skipped SYRK, and per sub-kernel the
// weight-scaled inverse, the fused contraction and the window row sums carry the chunk in blockIdx.z.  thetas: T rows of
// the sub-kernels' parameters back to back (sum n_thetas each); g_host: T x nk x n window weights; hrows: T x nk x n;
// qdiag_out (optional, T x n): diag(alpha alpha^T - K^-1) for the WhiteNoise term.  Larger problems: one at a time.
int gpmi_lml_grad_batch_mix(gpmi_ctx* c, int nk, const int* kernels, int64_t T, const double* thetas,
                            const int* n_thetas, const double* g_host, const double* hw_host, const double* extra,
                            const double* mus, const double* mu_const, double* lml, double* grad_thetas, double* hrows,
                            double* alpha_out, double* qdiag_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, T >= 1 && T <= RED_SLOTS, "T out of range");
  ARGCHK(c, nk >= 1 && nk <= GPMI_MAX_MIX, "number of sub-kernels out of range (1..4)");
  ARGCHK(c, kernels && thetas && n_thetas && g_host && lml && grad_thetas && hrows, "NULL argument");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  const MixBatch mx(nk, kernels, n_thetas, hw_host != nullptr);
  if (int rc = set_device(c)) return rc;
  const bool lockstep = (T >= 2 || c->lockstep_always) && c->np <= 4096 && !c->ycov;
  if (!lockstep)
    return one_at_a_time(c, T, mus, mu_const, [&](int64_t t, const double* mu_t) -> int {
      int inf = 0;
      const int rc = gpmi_lml_grad_mix(c, nk, kernels, thetas + t * mx.tot_nt, n_thetas, g_host + t * nk * c->n,
                                       hw_host ? hw_host + t * nk * 2 * c->n : nullptr, extra ? extra[t] : 0.0, mu_t,
                                       lml + t, grad_thetas + t * mx.tot_nt, hrows + t * nk * mx.nrow * c->n,
                                       alpha_out ? alpha_out + t * c->n : nullptr, &inf);
      if (info) info[t] = inf;
      if (rc != GPMI_OK) return rc;
      return qdiag_out ? gpmi_lml_grad_qdiag(c, qdiag_out + t * c->n) : GPMI_OK;
    });
  if (c->lanes.size() < 2)
    if (int rc = ensure_lanes(c, 2)) return rc;
  std::vector<KParams> ps;
  if (int rc = make_mix_batch_params(c, mx, T, thetas, ps)) return rc;
  ARGCHK(c, c->bpend[0] == 0 && c->bpend[1] == 0,
         "gpmi_lml_grad_batch_mix: an asynchronous batch is pending on this handle (gpmi_lml_batch_wait first)");
  if (int rc = ensure_batch_ws(c, (int)(T < 64 ? (T < 2 ? 2 : T) : 64))) return rc;
  if (int rc = ensure_batch_grad_ws(c, c->bcap, nk * mx.W() - 1)) return rc;
  if (int rc = ensure_batch_mix_ws(c)) return rc;
  const int cap = c->bgrad_cap;
  if (qdiag_out)
    if (int rc = c->bNoise.reserve(c, cap * c->np)) return rc;
  hipStream_t s = c->lanes[1].stream;
  static const bool stage_times = std::getenv("GPMI_DEBUG_STAGES") != nullptr;  // debugging aid: host time per stage
  RowStage stage(c, s);  // strided outputs reach the caller's arrays through pinned memory (api_internal.h)
  if (int rc = stage.reserve((size_t)cap * (sizeof(double) * (3 * GPMI_MAX_MIX * c->np + c->n) + GPMI_MAX_MIX * sizeof(KParams) + 4096) +
                             (size_t)(2 * GPMI_MAX_MIX + 2) * cap * (sizeof(double) * c->n + 256)))
    return rc;
  for (int64_t t0 = 0; t0 < T; t0 += cap) {
    const auto h0 = std::chrono::steady_clock::now();
    const int B = (int)((T - t0 < cap) ? T - t0 : cap);
    const Chunk k(c, s, 0, B, mus != nullptr);
    if (int rc = stage_mix_inputs(stage, k, mx, t0, T, ps, g_host, hw_host, extra, mus, mu_const)) return rc;
    if (int rc = lockstep_stages(k, ChunkBuild::mixture(mx), LS_CLEAR_INFO | LS_REDUCE | LS_BACKWARD | LS_INVERSE)) return rc;
    // K^-1 = L^-T L^-1 in full (it is read row-wise below)
    k.syrk(1);
    launch_mirror_lower(s, k.A, c->ld, c->np, B, k.bs.sMat);
    if (qdiag_out) launch_qdiag_batched(s, B, k.A, c->ld, k.alpha(), c->bNoise, c->n, k.bs.sMat, k.bs.sVec, c->np);
    mix_sub_kernel_terms(k, mx, nullptr, 0);
    HIPCHK(c, hipGetLastError());
    const auto h1 = std::chrono::steady_clock::now();
    HIPCHK(c, hipMemcpyAsync(c->h_bRed, k.red, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_bGout, c->bGout, sizeof(double) * nk * cap * mx.W(), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_bInfo, k.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    const size_t rowb = sizeof(double) * c->n;
    for (int row = 0; row < nk * mx.nrow; ++row)
      if (int rc = stage.down(hrows + (t0 * nk * mx.nrow + row) * c->n, rowb * nk * mx.nrow, c->bMixH + (int64_t)row * c->np,
                              sizeof(double) * mx.sW(c), rowb, B))
        return rc;
    if (alpha_out)
      if (int rc = stage.down(alpha_out + t0 * c->n, rowb, k.alpha(), sizeof(double) * k.bs.sVec, rowb, B)) return rc;
    if (qdiag_out)
      if (int rc = stage.down(qdiag_out + t0 * c->n, rowb, c->bNoise, sizeof(double) * c->np, rowb, B)) return rc;
    const auto h2 = std::chrono::steady_clock::now();
    HIPCHK(c, hipStreamSynchronize(s));
    stage.finish();
    if (stage_times) {
      const auto h3 = std::chrono::steady_clock::now();
      auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
      std::fprintf(stderr, "[gpmi stages] lml_grad_batch_mix B=%d: uploads+launches %.2f ms, download enqueue %.2f ms, wait %.2f ms\n", B,
                   ms(h0, h1), ms(h1, h2), ms(h2, h3));
    }
    for (int b = 0; b < B; ++b) {
      const int inf = c->h_bInfo[b];
      INFOCHK(c, inf);
      lml[t0 + b] = -0.5 * c->h_bRed[2 * b] - c->h_bRed[2 * b + 1];
      unpack_mix_gradient(c, mx, b, 1.0, grad_thetas + (t0 + b) * mx.tot_nt);
      if (info) info[t0 + b] = inf;
    }
  }
  return GPMI_OK;
}

// Leave-one-out terms and gradient (regression.py:489-526) of a two-or-more-region ChangePoint mixture for T hyper-parameter
// vectors in lockstep (round 5): gpmi_lml_grad_batch_mix's build / factorisation / inverse, then the leave-one-out
// vectors, M = K^-1 diag(c2) K^-1 and, per sub-kernel, the weight-scaled M with u = g_m o p, v = g_m o alpha in the
// fused contraction and the window row sums h_m(i) = sum_j (sym(p alpha^T) - M)_ij K_m,ij g_m(j).  Outputs per evaluation:
// alpha, diag(K^-1), p = K^-1 c1, diag(M) (WhiteNoise: 2 s^2 sum(p o alpha - diag M)), the sub-kernels' gradients and the
// row sums (window parameters: 2 sum_i dw_i (h_1 - h_0)_i, contracted on the host).  Lockstep sizes only.
int gpmi_loo_grad_batch_mix(gpmi_ctx* c, int nk, const int* kernels, int64_t T, const double* thetas,
                            const int* n_thetas, const double* g_host, const double* hw_host, const double* extra,
                            const double* mus, const double* mu_const, double* alpha_out, double* ikdiag_out,
                            double* p_out, double* mdiag_out, double* grad_thetas, double* hrows, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, T >= 1 && T <= RED_SLOTS, "T out of range");
  ARGCHK(c, nk >= 1 && nk <= GPMI_MAX_MIX, "number of sub-kernels out of range (1..4)");
  ARGCHK(c, kernels && thetas && n_thetas && g_host && alpha_out && ikdiag_out && p_out && mdiag_out && grad_thetas && hrows,
         "NULL argument");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  const MixBatch mx(nk, kernels, n_thetas, hw_host != nullptr);
  if (int rc = set_device(c)) return rc;
  ARGCHK(c, c->np <= 4096 && !c->ycov, "lockstep sizes only (n <= 4096, diagonal data errors)");
  if (c->lanes.size() < 2)
    if (int rc = ensure_lanes(c, 2)) return rc;
  std::vector<KParams> ps;
  if (int rc = make_mix_batch_params(c, mx, T, thetas, ps)) return rc;
  ARGCHK(c, c->bpend[0] == 0 && c->bpend[1] == 0,
         "gpmi_loo_grad_batch_mix: an asynchronous batch is pending on this handle (gpmi_lml_batch_wait first)");
  if (int rc = ensure_batch_ws(c, (int)(T < 64 ? (T < 2 ? 2 : T) : 64))) return rc;
  if (int rc = ensure_batch_grad_ws(c, c->bcap, nk * mx.W() - 1)) return rc;
  if (int rc = ensure_batch_mix_ws(c)) return rc;
  const int cap = c->bgrad_cap;
  // four more vectors per problem: diag(K^-1), c1, sqrt(c2) - later diag(M) -, p = K^-1 c1 (regression.py:505-513).
  // (the same stride as the work vectors': the fused contraction takes u = p and v = alpha with ONE stride)
  if (int rc = c->bLoo.reserve(c, cap * 4 * c->np)) return rc;
  const LooVectors lv(c);
  hipStream_t s = c->lanes[1].stream;
  RowStage stage(c, s);  // strided outputs reach the caller's arrays through pinned memory (api_internal.h)
  if (int rc = stage.reserve((size_t)cap * (sizeof(double) * (3 * GPMI_MAX_MIX * c->np + c->n) + GPMI_MAX_MIX * sizeof(KParams) + 4096) +
                             (size_t)(2 * GPMI_MAX_MIX + 4) * cap * (sizeof(double) * c->n + 256)))
    return rc;
  for (int64_t t0 = 0; t0 < T; t0 += cap) {
    const int B = (int)((T - t0 < cap) ? T - t0 : cap);
    const Chunk k(c, s, 0, B, mus != nullptr);
    if (int rc = stage_mix_inputs(stage, k, mx, t0, T, ps, g_host, hw_host, extra, mus, mu_const)) return rc;
    if (int rc = lockstep_stages(k, ChunkBuild::mixture(mx), LS_CLEAR_INFO | LS_BACKWARD | LS_INVERSE)) return rc;
    // M in full as well: it is read row-wise below
    loo_middle(k, lv, true, true);
    // Q = sym(p alpha^T) - M (the contraction returns 1/2 of the sum; the leave-one-out gradient has no 1/2: doubled below)
    mix_sub_kernel_terms(k, mx, lv.p, lv.sLoo);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_bGout, c->bGout, sizeof(double) * nk * cap * mx.W(), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_bInfo, k.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    const size_t rowb = sizeof(double) * c->n;
    for (int row = 0; row < nk * mx.nrow; ++row)
      if (int rc = stage.down(hrows + (t0 * nk * mx.nrow + row) * c->n, rowb * nk * mx.nrow, c->bMixH + (int64_t)row * c->np,
                              sizeof(double) * mx.sW(c), rowb, B))
        return rc;
    if (int rc = stage.down(alpha_out + t0 * c->n, rowb, k.alpha(), sizeof(double) * k.bs.sVec, rowb, B)) return rc;
    if (int rc = stage.down(ikdiag_out + t0 * c->n, rowb, lv.diag, sizeof(double) * lv.sLoo, rowb, B)) return rc;
    if (int rc = stage.down(p_out + t0 * c->n, rowb, lv.p, sizeof(double) * lv.sLoo, rowb, B)) return rc;
    if (int rc = stage.down(mdiag_out + t0 * c->n, rowb, lv.sc2, sizeof(double) * lv.sLoo, rowb, B)) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    stage.finish();
    for (int b = 0; b < B; ++b) {
      const int inf = c->h_bInfo[b];
      INFOCHK(c, inf);
      unpack_mix_gradient(c, mx, b, 2.0, grad_thetas + (t0 + b) * mx.tot_nt);
      if (info) info[t0 + b] = inf;
    }
  }
  return GPMI_OK;
}

int gpmi_loo_terms_mix(gpmi_ctx* c, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                       const double* g_host, double extra_diag, const double* mu, double* alpha_out,
                       double* ikdiag, int* info) {
  if (!c) return GPMI_ERR_ARG;
  KParams ps[GPMI_MAX_MIX];
  if (int rc = mix_prepare(c, nk, kernels, thetas, n_thetas, g_host, ps)) return rc;
  ARGCHK(c, mu && alpha_out && ikdiag, "mu / alpha / ikdiag is NULL");
  c->fitted = false;
  const MixEval mx{nk, ps, c->mix_g, extra_diag, c->mix_scratch, c->mix_zero};
  return lane_loo_terms(LaneEval(c, 1), LaneBuild::mixture(mx), mu, alpha_out, ikdiag, info);
}

int gpmi_predict_mix(gpmi_ctx* c, const double* pts, int64_t m, const double* gq_host, double* mu_out,
                     double* negsumsq_out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted && c->mix_nk > 0, "gpmi_predict_mix needs a successful gpmi_fit_mix");
  ARGCHK(c, pts && gq_host && m > 0, "NULL argument or m <= 0");
  if (int rc = set_device(c)) return rc;
  auto fill = [&](int64_t m0, int64_t mc, int64_t mp) { return upload_and_build_mix_cross(c, pts, gq_host, m, m0, mc, mp); };
  return predict_rows(c, m, fill, 0.0, mu_out, negsumsq_out);  // -|L^-1 k|^2; the host adds K_qq[0, 0]
}

int gpmi_posterior_mix(gpmi_ctx* c, const double* pts, int64_t m, const double* gq_host, double* mu_out,
                       double* cov_out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted && c->mix_nk > 0, "gpmi_posterior_mix needs a successful gpmi_fit_mix");
  ARGCHK(c, pts && gq_host && m > 0, "NULL argument or m <= 0");
  if (int rc = set_device(c)) return rc;
  hipStream_t s = c->lanes[0].stream;
  const int64_t mp = round_up(m, GPMI_NB), ldq = mp + 32;
  if (int rc = ensure_query_ws(c, mp)) return rc;
  // (an error return below may leave work on these in flight: hipFree waits for the device before it releases)
  DevBuf<double> Sigma, tmp;
  if (cov_out) {
    if (int rc = Sigma.alloc(c, mp * ldq)) return rc;
    if (int rc = tmp.alloc(c, mp * ldq)) return rc;
  }
  auto cross = [&] { return upload_and_build_mix_cross(c, pts, gq_host, m, 0, m, mp); };
  // K_qq = sum_m diag(gq_m) K_m(pts, pts) diag(gq_m): no jitter, no noise (covariance.py:529-544)
  auto qq = [&] {
    for (int k = 0; k < c->mix_nk; ++k) {
      const double* gq = c->pvec + 2 * mp + (int64_t)k * mp;
      launch_kbuild_cross(s, c->mix_p[k], c->pts, m, mp, c->pts, m, mp, tmp, ldq);
      launch_scale_add(s, Sigma, ldq, tmp, ldq, gq, gq, mp, mp, k > 0);
    }
  };
  if (int rc = posterior_sigma(c, cross, qq, m, mp, mu_out, Sigma, ldq)) return rc;
  if (cov_out)
    HIPCHK(c, hipMemcpy2DAsync(cov_out, sizeof(double) * m, Sigma, sizeof(double) * ldq, sizeof(double) * m, m,
                               hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return GPMI_OK;
}

}  // extern "C"

// ---- per-point noise hyper-parameters ----------------------------------------------------------------
extern "C" {

int gpmi_set_noise(gpmi_ctx* c, const double* noise_var) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, noise_var != nullptr, "noise_var is NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = gpmi_sync(c)) return rc;  // nothing may still be reading the old values
  HIPCHK(c, hipMemcpy(c->noise, noise_var, sizeof(double) * c->n, hipMemcpyHostToDevice));
  return GPMI_OK;
}

int gpmi_lml_grad_qdiag(gpmi_ctx* c, double* qdiag) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, qdiag != nullptr, "qdiag is NULL");
  ARGCHK(c, c->lanes.size() >= 2 && c->lanes[1].B2, "gpmi_lml_grad has not been called");
  if (int rc = set_device(c)) return rc;
  Lane& L = c->lanes[1];  // after gpmi_lml_grad: L.A = K^-1 (lower tiles), vec + np = alpha
  double* out = LaneEval(c, 1).slot2();
  launch_qdiag(L.stream, L.A, c->ld, LaneEval(c, 1).alpha(), out, c->n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(qdiag, out, sizeof(double) * c->n, hipMemcpyDeviceToHost, L.stream));
  HIPCHK(c, hipStreamSynchronize(L.stream));
  return GPMI_OK;
}

}  // extern "C"

