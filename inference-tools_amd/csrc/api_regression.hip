// C-ABI of libgpmi (include/gpmi.h): the GpRegressor entry points - fit, likelihood (single, lockstep batches, asynchronous slots), likelihood
// and leave-one-out gradients, predict, posterior, spatial gradients, covariance downloads.
// (split from api.hip in round 4; the handle, the lanes and the helpers these entry points are built from: api.hip,
// api_internal.h; the pipeline of the single evaluations: api_single.hip)
#include "api_internal.h"

extern "C" {

int gpmi_fit(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag,
             const double* mu, double* alpha_out, double* logdet_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, mu != nullptr, "mu is NULL");
  if (int rc = set_device(c)) return rc;
  LaneEval ev(c, 0);
  LaneTimes t;
  ev.times = &t;
  t.start = std::chrono::steady_clock::now();
  // alpha = L^-T v, the predict's inverse blocks beside the two sweeps
  if (int rc = lane_stages(ev, LaneBuild::kernels(p), LN_BACKWARD | LN_FIT_SCHEDULE, mu)) return rc;
  int inf = 0;
  const int rc = lane_collect(ev, LC_LOGDET, 0, {{alpha_out, ev.alpha()}}, logdet_out, &inf);
  if (std::getenv("GPMI_DEBUG_TIMING") && t.done != std::chrono::steady_clock::time_point()) {
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "[gpmi_fit] host enqueue factor+forward %.2f ms, backward+copies %.2f ms, final sync %.2f ms\n",
                 ms(t.start, t.forward), ms(t.forward, t.enqueued), ms(t.enqueued, t.done));
  }
  if (rc != GPMI_OK) return rc;
  if (info) *info = inf;
  c->fit_params = p;
  c->fitted = (inf == 0);
  return GPMI_OK;
}

int gpmi_lml(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag,
             const double* mu, double* lml, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, mu != nullptr && lml != nullptr, "mu / lml is NULL");
  int inf = 0;
  int rc = gpmi_lml_batch(c, kernel, 1, theta, n_theta, &extra_diag, mu, nullptr, lml, &inf);
  if (info) *info = inf;
  return rc;
}

int gpmi_lml_batch(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta,
                   const double* extra, const double* mus, const double* mu_const, double* lml,
                   int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, T >= 1 && T <= RED_SLOTS, "T out of range");
  ARGCHK(c, thetas && lml, "thetas / lml is NULL");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  if (int rc = set_device(c)) return rc;
  if (c->lanes.size() < 2)
    if (int rc = ensure_lanes(c, 2)) return rc;
  const int S = (int)c->lanes.size() - 1;
  std::vector<KParams> ps;
  std::vector<CovParams> sps;  // (a sum: its parameters, ps stays empty)
  if (int rc = make_batch_params(c, kernel, T, thetas, n_theta, extra, ps, sps)) return rc;
  if ((T >= 2 || c->lockstep_always) && c->np <= 4096 && !c->ycov) {
    // small problems: all evaluations of a chunk advance in lockstep, one launch per step for the
    // whole chunk (blockIdx.z), instead of one latency-bound launch sequence per evaluation
    ARGCHK(c, c->bpend[0] == 0 && c->bpend[1] == 0,
           "gpmi_lml_batch: an asynchronous batch is pending on this handle (gpmi_lml_batch_wait first)");
    if (int rc = ensure_batch_ws(c, (int)(T < 2 ? 2 : (T > 4096 ? 4096 : T)))) return rc;  // (capped by ensure_batch_ws)
    // A chunk runs as TWO half-batches on two streams (the chunk's workspace split in the middle): while one half is in
    // a latency-bound step - potrf_diag: one workgroup per matrix, 32 of 256 CUs for a half of 32 - the other half's
    // GEMM launches fill the chip.  A value does not depend on the batch it is evaluated in (§4.3), so the split is
    // invisible in the results.  GPMI_BATCH_SPLIT=0: one stream (A/B).
    const bool two = batch_split_enabled() && T >= 16 && ensure_lanes(c, 3) == GPMI_OK;
    const BatchParams bp(kernel, ps, sps);
    auto enqueue = [&](hipStream_t s, int64_t t_first, int off, int B) -> int {
      const Chunk k(c, s, off, B, mus != nullptr);
      HIPCHK(c, hipMemcpyAsync(bp.device(c, off), bp.host(t_first), bp.bytes_each() * B, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(k.Mu, mus ? mus + t_first * c->n : mu_const + t_first, sizeof(double) * B * (mus ? c->n : 1),
                               hipMemcpyHostToDevice, s));
      if (int rc = lockstep_stages(k, ChunkBuild::kernels(bp), LS_CLEAR_INFO | LS_REDUCE)) return rc;
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(c->h_bRed + 2 * off, k.red, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(c->h_bInfo + off, k.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
      return GPMI_OK;
    };
    for (int64_t t0 = 0; t0 < T; t0 += c->bcap) {
      const int B = (int)((T - t0 < c->bcap) ? T - t0 : c->bcap);
      const int B1 = (two && B >= 16) ? B / 2 : B;
      if (int rc = enqueue(c->lanes[1].stream, t0, 0, B1)) return rc;
      if (B1 < B)
        if (int rc = enqueue(c->lanes[2].stream, t0 + B1, B1, B - B1)) return rc;
      HIPCHK(c, hipStreamSynchronize(c->lanes[1].stream));
      if (B1 < B) HIPCHK(c, hipStreamSynchronize(c->lanes[2].stream));
      for (int b = 0; b < B; ++b) {
        const int inf = c->h_bInfo[b];
        INFOCHK(c, inf);
        lml[t0 + b] = (inf == 0) ? (-0.5 * c->h_bRed[2 * b] - c->h_bRed[2 * b + 1]) : -1e50;
        if (info) info[t0 + b] = inf;
      }
    }
    return GPMI_OK;
  }
  std::vector<int> slot_of((size_t)T);
  std::vector<int> used((size_t)S, 0);
  for (int64_t t = 0; t < T; ++t) {
    const int li = (int)(t % S);
    Lane& L = c->lanes[1 + li];
    const int slot = used[li]++;
    slot_of[(size_t)t] = slot;
    double* mu_dev = nullptr;
    if (mus) {
      mu_dev = LaneEval(c, 1 + li).mu();
      HIPCHK(c, hipMemcpyAsync(mu_dev, mus + t * c->n, sizeof(double) * c->n,
                               hipMemcpyHostToDevice, L.stream));
    }
    const CovParams pt = sps.empty() ? CovParams(ps[(size_t)t]) : sps[(size_t)t];
    if (int rc = enqueue_factor_and_forward(c, L, pt, mu_dev,
                                            mu_const ? mu_const[t] : 0.0, slot, S == 1 || T == 1))
      return rc;
  }
  for (int li = 0; li < S; ++li) {
    if (!used[li]) continue;
    Lane& L = c->lanes[1 + li];
    HIPCHK(c, hipMemcpyAsync(L.h_red, L.red, 2 * sizeof(double) * used[li], hipMemcpyDeviceToHost,
                             L.stream));
    HIPCHK(c, hipMemcpyAsync(L.h_info, L.info, sizeof(int) * used[li], hipMemcpyDeviceToHost,
                             L.stream));
  }
  for (int li = 0; li < S; ++li)
    if (used[li]) HIPCHK(c, hipStreamSynchronize(c->lanes[1 + li].stream));
  for (int64_t t = 0; t < T; ++t) {
    Lane& L = c->lanes[1 + (int)(t % S)];
    const int slot = slot_of[(size_t)t];
    const int inf = L.h_info[slot];
    INFOCHK(c, inf);
    // -1/2 v.v - sum ln L_ii (regression.py:539); sentinel on failure (regression.py:540-542)
    lml[t] = (inf == 0) ? (-0.5 * L.h_red[2 * slot] - L.h_red[2 * slot + 1]) : -1e50;
    if (info) info[t] = inf;
  }
  return GPMI_OK;
}

// Asynchronous lockstep batches: gpmi_lml_batch_submit enqueues the T evaluations of a slot and returns; the caller does
// its own work (a tempering driver: the accept / reject bookkeeping of the OTHER half of its chains) and collects the
// values with gpmi_lml_batch_wait.  Two slots, the two halves of the lockstep workspace, on two streams - the same
// device work as one gpmi_lml_batch call of both halves (which runs them as two half-batches side by side), so a value
// is bit-identical either way.  Lockstep sizes only (np <= 4096, no dense y covariance).
int gpmi_lml_batch_submit(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                          const double* mus, const double* mu_const, int slot) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, slot == 0 || slot == 1, "slot must be 0 or 1");
  // evaluations per slot: GPMI_ASYNC_SLOT_MAX (default 256 - 128 until round 6; the workspace budget GPMI_BATCH_GIB /
  // GPMI_BATCH_MAX decides how many of them a slot really gets: api.hip, ensure_batch_ws)
  static const int slot_max = [] {
    const char* e = std::getenv("GPMI_ASYNC_SLOT_MAX");
    const int v = e ? std::atoi(e) : 256;
    return v >= 1 && v <= 2048 ? v : 256;
  }();
  ARGCHK(c, T >= 1 && T <= slot_max, "T out of range (1 .. GPMI_ASYNC_SLOT_MAX per slot, default 256)");
  ARGCHK(c, thetas, "thetas is NULL");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  ARGCHK(c, c->np <= 4096 && !c->ycov, "asynchronous batches: lockstep sizes only (n <= 4096, diagonal data errors)");
  ARGCHK(c, c->bpend[slot] == 0, "this slot has a batch pending (gpmi_lml_batch_wait first)");
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_lanes(c, 3)) return rc;
  // each slot owns half of the workspace: at least 2 T matrices - and, because the workspace can only grow while nothing
  // is pending, all that a slot may ever be asked for (128 evaluations) from the first submission on, as far as the
  // memory cap of ensure_batch_ws allows: a later, larger group of chains then fits whatever the first one was
  if (c->bpend[1 - slot] == 0) {
    if (int rc = ensure_batch_ws(c, 2 * slot_max)) return rc;  // (a no-op once it is that large)
    ARGCHK(c, c->bcap >= 2 * T, "not enough device memory for two batches of this size");
  } else {
    ARGCHK(c, c->bcap >= 2 * T,
           "this batch does not fit the slot (half of the lockstep workspace) and the workspace cannot grow while the other slot is pending");
  }
  const int off = slot * (c->bcap / 2);
  // inputs through pinned staging that lives until the wait (the copies are asynchronous)
  const int64_t mu_doubles = mus ? T * c->n : T;
  const size_t psize = (kernel == GPMI_KERNEL_SUM) ? sizeof(CovParams) : sizeof(KParams);
  const int64_t need = (int64_t)psize * T + (int64_t)sizeof(double) * mu_doubles;
  if (int rc = c->h_bStage[slot].reserve(c, need)) return rc;
  char* const h_stage = c->h_bStage[slot];
  double* mu_stage = reinterpret_cast<double*>(h_stage + psize * T);
  if (kernel == GPMI_KERNEL_SUM) {
    CovParams* sps = reinterpret_cast<CovParams*>(h_stage);
    for (int64_t t = 0; t < T; ++t)
      if (int rc = make_cov(c, kernel, thetas + t * n_theta, n_theta, extra ? extra[t] : 0.0, sps[t])) return rc;
  } else {
    KParams* ps = reinterpret_cast<KParams*>(h_stage);
    for (int64_t t = 0; t < T; ++t)
      if (int rc = make_params(c, kernel, thetas + t * n_theta, n_theta, extra ? extra[t] : 0.0, ps[t])) return rc;
  }
  std::memcpy(mu_stage, mus ? mus : mu_const, sizeof(double) * mu_doubles);
  hipStream_t s = c->lanes[1 + slot].stream;
  const bool sum = (kernel == GPMI_KERNEL_SUM);
  const BatchParams bp = sum ? BatchParams(kernel, nullptr, reinterpret_cast<const CovParams*>(h_stage))
                             : BatchParams(kernel, reinterpret_cast<const KParams*>(h_stage), nullptr);
  const Chunk k(c, s, off, (int)T, mus != nullptr);
  HIPCHK(c, hipMemcpyAsync(bp.device(c, off), h_stage, bp.bytes_each() * T, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(k.Mu, mu_stage, sizeof(double) * mu_doubles, hipMemcpyHostToDevice, s));
  if (int rc = lockstep_stages(k, ChunkBuild::kernels(bp), LS_CLEAR_INFO | LS_REDUCE)) return rc;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_bRed + 2 * off, k.red, sizeof(double) * 2 * T, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(c->h_bInfo + off, k.info, sizeof(int) * T, hipMemcpyDeviceToHost, s));
  c->bpend[slot] = (int)T;
  return GPMI_OK;
}

int gpmi_lml_batch_wait(gpmi_ctx* c, int slot, double* lml, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, slot == 0 || slot == 1, "slot must be 0 or 1");
  ARGCHK(c, c->bpend[slot] > 0, "nothing pending in this slot");
  ARGCHK(c, lml, "lml is NULL");
  if (int rc = set_device(c)) return rc;
  const int T = c->bpend[slot];
  const int off = slot * (c->bcap / 2);
  c->bpend[slot] = 0;  // whatever happens below, the slot is free again
  HIPCHK(c, hipStreamSynchronize(c->lanes[1 + slot].stream));
  for (int b = 0; b < T; ++b) {
    const int inf = c->h_bInfo[off + b];
    INFOCHK(c, inf);
    lml[b] = (inf == 0) ? (-0.5 * c->h_bRed[2 * (off + b)] - c->h_bRed[2 * (off + b) + 1]) : -1e50;
    if (info) info[b] = inf;
  }
  return GPMI_OK;
}

int gpmi_prepare_gradient(gpmi_ctx* c, int n_theta) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, n_theta >= 1 && n_theta <= GPMI_MAX_SUM * (GPMI_MAX_D + 2), "n_theta out of range");
  if (int rc = set_device(c)) return rc;
  // everything gpmi_lml_grad allocates lazily: the lane itself (matrix, inverse blocks, streams - for a large problem the
  // CU-masked pair), the second matrix, the contraction's partial sums for n_theta parameters
  if (int rc = lane_prepare(LaneEval(c, 1), LN_INVERSE, n_theta)) return rc;
  HIPCHK(c, hipDeviceSynchronize());  // the allocations have happened when this returns
  return GPMI_OK;
}

int gpmi_lml_grad(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag,
                  const double* mu, double* lml, double* grad_theta, double* trace_q,
                  double* alpha_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, mu && lml && grad_theta, "mu / lml / grad_theta is NULL");
  if (int rc = set_device(c)) return rc;
  const LaneEval ev(c, 1);
  // K^-1 in the lower tiles only: the contraction reads no others
  if (int rc = lane_stages(ev, LaneBuild::kernels(p), LN_BACKWARD | LN_INVERSE | LN_SYRK, mu, n_theta)) return rc;
  launch_lml_grad(ev.stream(), p, n_theta, c->x, c->n, c->np, ev.L().A, c->ld, ev.alpha(), ev.alpha(), ev.partial(false), ev.gout());
  const int rc = lane_collect(ev, LC_LML_RAW, n_theta + 1, {{alpha_out, ev.alpha()}}, lml, info);
  for (int j = 0; j < n_theta; ++j) grad_theta[j] = ev.h_gout()[j];
  if (trace_q) *trace_q = ev.h_gout()[n_theta];
  return rc;
}

// noise_batch (T x n, host) / qdiag_out (T x n, host): the per-problem noise variances of HeteroscedasticNoise
// (covariance.py:608-690: they are hyper-parameters) and the diagonal of Q = alpha alpha^T - K^-1 their gradient needs;
// both NULL for the plain form
static int lml_grad_batch_impl(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                               const double* mus, const double* mu_const, const double* noise_batch, double* lml,
                               double* grad_theta, double* trace_q, double* alpha_out, double* qdiag_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, T >= 1 && T <= RED_SLOTS, "T out of range");
  ARGCHK(c, thetas && lml && grad_theta, "thetas / lml / grad_theta is NULL");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  if (int rc = set_device(c)) return rc;
  const bool lockstep = (T >= 2 || c->lockstep_always) && c->np <= 4096 && !c->ycov;
  if (!lockstep)
    // large problems are throughput-bound one at a time: the single-evaluation path, one after another
    return one_at_a_time(c, T, mus, mu_const, [&](int64_t t, const double* mu_t) -> int {
      int inf = 0;
      if (noise_batch)
        if (int rc = gpmi_set_noise(c, noise_batch + t * c->n)) return rc;
      const int rc = gpmi_lml_grad(c, kernel, thetas + t * n_theta, n_theta, extra ? extra[t] : 0.0, mu_t, lml + t,
                                   grad_theta + t * n_theta, trace_q ? trace_q + t : nullptr,
                                   alpha_out ? alpha_out + t * c->n : nullptr, &inf);
      if (info) info[t] = inf;
      if (rc != GPMI_OK) return rc;
      return qdiag_out ? gpmi_lml_grad_qdiag(c, qdiag_out + t * c->n) : GPMI_OK;
    });
  if (c->lanes.size() < 2)
    if (int rc = ensure_lanes(c, 2)) return rc;
  std::vector<KParams> ps;
  std::vector<CovParams> sps;  // (a sum: its parameters, ps stays empty)
  if (int rc = make_batch_params(c, kernel, T, thetas, n_theta, extra, ps, sps)) return rc;
  const BatchParams bp(kernel, ps, sps);
  // lockstep: every launch carries the chunk in blockIdx.z - K-build, factorisation, both sweeps, L^-T by forward
  // substitution on the identity, the k-skipped SYRK K^-1 = L^-T L^-1 (regression.py:556-557) and the fused contraction
  ARGCHK(c, c->bpend[0] == 0 && c->bpend[1] == 0,
         "gpmi_lml_grad_batch: an asynchronous batch is pending on this handle (gpmi_lml_batch_wait first)");
  if (int rc = ensure_batch_ws(c, (int)(T < 64 ? (T < 2 ? 2 : T) : 64))) return rc;
  if (int rc = ensure_batch_grad_ws(c, c->bcap, n_theta)) return rc;
  if (noise_batch || qdiag_out)
    if (int rc = c->bNoise.reserve(c, c->bgrad_cap * c->np)) return rc;
  hipStream_t s = c->lanes[1].stream;
  const int W = n_theta + 1;
  const size_t rowb = sizeof(double) * c->n;
  RowStage stage(c, s);  // strided rows travel between the caller's arrays and the device through pinned memory (api_internal.h)
  if (int rc = stage.reserve((size_t)c->bgrad_cap * (7 * (rowb + 256) + sizeof(CovParams) + 512))) return rc;
  for (int64_t t0 = 0; t0 < T; t0 += c->bgrad_cap) {
    const int B = (int)((T - t0 < c->bgrad_cap) ? T - t0 : c->bgrad_cap);
    const Chunk k(c, s, 0, B, mus != nullptr);
    if (int rc = stage_batch_inputs(stage, k, bp, t0, mus, mu_const)) return rc;
    if (int rc = k.clear_info()) return rc;
    if (noise_batch)
      if (int rc = stage.up(c->bNoise, sizeof(double) * c->np, noise_batch + t0 * c->n, rowb, rowb, B)) return rc;
    if (int rc = lockstep_stages(k, ChunkBuild::kernels(bp, noise_batch ? c->bNoise : nullptr), LS_REDUCE | LS_BACKWARD | LS_INVERSE))
      return rc;
    k.syrk(1);
    launch_lml_grad_batched(k, bp, n_theta, k.alpha(), k.alpha(), k.bs.sVec);
    if (qdiag_out) {  // diag(alpha alpha^T - K^-1) per problem, into the noise buffer (consumed by the build above)
      launch_qdiag_batched(s, B, k.A, c->ld, k.alpha(), c->bNoise, c->n, k.bs.sMat, k.bs.sVec, c->np);
      if (int rc = stage.down(qdiag_out + t0 * c->n, rowb, c->bNoise, sizeof(double) * c->np, rowb, B)) return rc;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_bRed, k.red, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_bGout, c->bGout, sizeof(double) * W * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_bInfo, k.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    if (alpha_out)
      if (int rc = stage.down(alpha_out + t0 * c->n, rowb, k.alpha(), sizeof(double) * k.bs.sVec, rowb, B)) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    stage.finish();
    for (int b = 0; b < B; ++b) {
      const int inf = c->h_bInfo[b];
      INFOCHK(c, inf);
      lml[t0 + b] = -0.5 * c->h_bRed[2 * b] - c->h_bRed[2 * b + 1];
      for (int j = 0; j < n_theta; ++j) grad_theta[(t0 + b) * n_theta + j] = c->h_bGout[b * W + j];
      if (trace_q) trace_q[t0 + b] = c->h_bGout[b * W + n_theta];
      if (info) info[t0 + b] = inf;
    }
  }
  return GPMI_OK;
}

int gpmi_lml_grad_batch(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                        const double* mus, const double* mu_const, double* lml, double* grad_theta, double* trace_q,
                        double* alpha_out, int* info) {
  return lml_grad_batch_impl(c, kernel, T, thetas, n_theta, extra, mus, mu_const, nullptr, lml, grad_theta, trace_q,
                             alpha_out, nullptr, info);
}

int gpmi_lml_grad_batch_noise(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                              const double* mus, const double* mu_const, const double* noise_var, double* lml,
                              double* grad_theta, double* trace_q, double* alpha_out, double* qdiag_out, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, noise_var && qdiag_out, "noise_var / qdiag is NULL");
  ARGCHK(c, kernel != GPMI_KERNEL_SUM, "gpmi_lml_grad_batch_noise does not take sums of kernels (GPMI_KERNEL_SUM)");
  ARGCHK(c, !c->ycov, "per-point noise hyper-parameters need diagonal data errors");
  return lml_grad_batch_impl(c, kernel, T, thetas, n_theta, extra, mus, mu_const, noise_var, lml, grad_theta, trace_q,
                             alpha_out, qdiag_out, info);
}

// Leave-one-out log-likelihood terms and gradient (regression.py:489-526) for T hyper-parameter vectors in lockstep: the
// batched form of gpmi_loo_grad - every launch carries the chunk in blockIdx.z.  What the reference's `multiprocessing.Pool`
// farms out start by start (regression.py:597-601) when the model selector is the cross-validation objective.
// noise_batch (T x n, host) / mdiag_out (T x n, host): the per-problem noise variances of HeteroscedasticNoise and the
// diagonal of M = K^-1 diag(c2) K^-1, which the gradient with respect to a point's own noise needs (dK = 2 s_i^2 e_i e_i^T:
// 2 s_i^2 (p_i alpha_i - M_ii)); both NULL for the plain form.  With them every call takes the lockstep path.
static int loo_grad_batch_impl(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                               const double* mus, const double* mu_const, const double* noise_batch, double* alpha_out,
                               double* ikdiag_out, double* p_out, double* mdiag_out, double* grad_theta, double* trace_q,
                               int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, T >= 1 && T <= RED_SLOTS, "T out of range");
  ARGCHK(c, thetas && alpha_out && ikdiag_out && p_out && grad_theta, "NULL argument");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  if (int rc = set_device(c)) return rc;
  const bool lockstep = (T >= 2 || c->lockstep_always || noise_batch) && c->np <= 4096 && !c->ycov;
  ARGCHK(c, lockstep || !noise_batch, "per-point noise in the batch: lockstep sizes only (n <= 4096, diagonal data errors)");
  if (!lockstep)
    return one_at_a_time(c, T, mus, mu_const, [&](int64_t t, const double* mu_t) -> int {
      int inf = 0;
      const int rc = gpmi_loo_grad(c, kernel, thetas + t * n_theta, n_theta, extra ? extra[t] : 0.0, mu_t,
                                   alpha_out + t * c->n, ikdiag_out + t * c->n, p_out + t * c->n,
                                   grad_theta + t * n_theta, trace_q ? trace_q + t : nullptr, &inf);
      if (info) info[t] = inf;
      return rc;
    });
  if (c->lanes.size() < 2)
    if (int rc = ensure_lanes(c, 2)) return rc;
  std::vector<KParams> ps;
  std::vector<CovParams> sps;  // (a sum: its parameters, ps stays empty)
  if (int rc = make_batch_params(c, kernel, T, thetas, n_theta, extra, ps, sps)) return rc;
  const BatchParams bp(kernel, ps, sps);
  ARGCHK(c, c->bpend[0] == 0 && c->bpend[1] == 0,
         "gpmi_loo_grad_batch: an asynchronous batch is pending on this handle (gpmi_lml_batch_wait first)");
  if (int rc = ensure_batch_ws(c, (int)(T < 64 ? (T < 2 ? 2 : T) : 64))) return rc;
  if (int rc = ensure_batch_grad_ws(c, c->bcap, n_theta)) return rc;
  if (noise_batch)
    if (int rc = c->bNoise.reserve(c, c->bgrad_cap * c->np)) return rc;
  // four more vectors per problem: diag(K^-1), c1, sqrt(c2) - later diag(M) -, p = K^-1 c1 (regression.py:505-513).
  // (the same stride as the work vectors': the fused contraction takes u = p and v = alpha with ONE stride)
  if (int rc = c->bLoo.reserve(c, c->bgrad_cap * 4 * c->np)) return rc;
  const LooVectors lv(c);
  hipStream_t s = c->lanes[1].stream;
  const int W = n_theta + 1;
  const size_t rowb = sizeof(double) * c->n;
  RowStage stage(c, s);  // strided rows travel between the caller's arrays and the device through pinned memory (api_internal.h)
  if (int rc = stage.reserve((size_t)c->bgrad_cap * (7 * (rowb + 256) + sizeof(CovParams) + 512))) return rc;
  for (int64_t t0 = 0; t0 < T; t0 += c->bgrad_cap) {
    const int B = (int)((T - t0 < c->bgrad_cap) ? T - t0 : c->bgrad_cap);
    const Chunk k(c, s, 0, B, mus != nullptr);
    if (int rc = stage_batch_inputs(stage, k, bp, t0, mus, mu_const)) return rc;
    if (int rc = k.clear_info()) return rc;
    if (noise_batch)
      if (int rc = stage.up(c->bNoise, sizeof(double) * c->np, noise_batch + t0 * c->n, rowb, rowb, B)) return rc;
    if (int rc = lockstep_stages(k, ChunkBuild::kernels(bp, noise_batch ? c->bNoise : nullptr), LS_BACKWARD | LS_INVERSE)) return rc;
    loo_middle(k, lv, mdiag_out != nullptr, false);
    launch_lml_grad_batched(k, bp, n_theta, lv.p, k.alpha(), lv.sLoo);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_bGout, c->bGout, sizeof(double) * W * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(c->h_bInfo, k.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    if (int rc = stage.down(alpha_out + t0 * c->n, rowb, k.alpha(), sizeof(double) * k.bs.sVec, rowb, B)) return rc;
    if (int rc = stage.down(ikdiag_out + t0 * c->n, rowb, lv.diag, sizeof(double) * lv.sLoo, rowb, B)) return rc;
    if (int rc = stage.down(p_out + t0 * c->n, rowb, lv.p, sizeof(double) * lv.sLoo, rowb, B)) return rc;
    if (mdiag_out)
      if (int rc = stage.down(mdiag_out + t0 * c->n, rowb, lv.sc2, sizeof(double) * lv.sLoo, rowb, B)) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    stage.finish();
    for (int b = 0; b < B; ++b) {
      const int inf = c->h_bInfo[b];
      INFOCHK(c, inf);
      // the contraction returns 1/2 sum Q o dK; the LOO gradient has no 1/2 (regression.py:513)
      for (int j = 0; j < n_theta; ++j) grad_theta[(t0 + b) * n_theta + j] = 2.0 * c->h_bGout[b * W + j];
      if (trace_q) trace_q[t0 + b] = c->h_bGout[b * W + n_theta];
      if (info) info[t0 + b] = inf;
    }
  }
  return GPMI_OK;
}

int gpmi_loo_grad_batch(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                        const double* mus, const double* mu_const, double* alpha_out, double* ikdiag_out, double* p_out,
                        double* grad_theta, double* trace_q, int* info) {
  return loo_grad_batch_impl(c, kernel, T, thetas, n_theta, extra, mus, mu_const, nullptr, alpha_out, ikdiag_out, p_out,
                             nullptr, grad_theta, trace_q, info);
}

int gpmi_loo_grad_batch_noise(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                              const double* mus, const double* mu_const, const double* noise_var, double* alpha_out,
                              double* ikdiag_out, double* p_out, double* mdiag_out, double* grad_theta, double* trace_q,
                              int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, noise_var && mdiag_out, "noise_var / mdiag is NULL");
  ARGCHK(c, kernel != GPMI_KERNEL_SUM, "gpmi_loo_grad_batch_noise does not take sums of kernels (GPMI_KERNEL_SUM)");
  ARGCHK(c, !c->ycov, "per-point noise hyper-parameters need diagonal data errors");
  return loo_grad_batch_impl(c, kernel, T, thetas, n_theta, extra, mus, mu_const, noise_var, alpha_out, ikdiag_out, p_out,
                             mdiag_out, grad_theta, trace_q, info);
}

int gpmi_predict(gpmi_ctx* c, const double* pts, int64_t m, double* mu_out, double* var_out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted, "gpmi_predict needs a successful gpmi_fit");
  ARGCHK(c, c->fit_params.kernel >= 0 || c->mix_nk > 0,
         "gpmi_predict: the model was fitted with a caller-built covariance (gpmi_fit_dense) - use gpmi_predict_dense / gpmi_solve_rows");
  ARGCHK(c, pts && m > 0, "pts is NULL or m <= 0");
  if (int rc = set_device(c)) return rc;
  hipStream_t s = c->lanes[0].stream;
  const CovParams& p = c->fit_params;
  auto fill = [&](int64_t m0, int64_t mc, int64_t mp) -> int {
    HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * c->d, sizeof(double) * mc * c->d, hipMemcpyHostToDevice, s));
    ProfScope ps(c, s, GPMI_PROF_KBUILD, 0.0, 8.0 * mp * c->np);
    launch_kbuild_cross(s, p, c->pts, mc, mp, c->x, c->n, c->np, c->Q, c->ld);
    return GPMI_OK;
  };
  return predict_rows(c, m, fill, p.a2, mu_out, var_out);  // K_qq[0,0] = a^2 (regression.py:210)
}

extern "C++" {
namespace {
// sum of v[0 .. n) as the pairwise tree of predict_batch.hip (halves split at the largest power of two below n)
double tree_sum_host(const double* v, int64_t n) {
  if (n <= 0) return 0.0;
  if (n == 1) return v[0];
  int64_t h = 1;
  while (2 * h < n) h *= 2;
  return tree_sum_host(v, h) + tree_sum_host(v + h, n - h);
}
}  // namespace
}  // extern "C++"

// Prediction under T hyper-parameter vectors and its mixture (include/gpmi.h).  Per chunk of rows, in lockstep on the two
// half-batch streams (as gpmi_lml_batch; chunks capped as the gradient batches): K(theta_z), factor, both sweeps -> alpha_z;
// with a variance L_z^-T by forward substitution on the identity (bB2).  Then per panel of GPMI_PREDICT_PANEL points: the
// batched cross-covariance K*_z, its row dots with alpha_z, V_z = K*_z L_z^-T by the batched k-major GEMM (contraction
// ending with the tile column: L^-T is upper triangular; ring_order_only - a value does not depend on the batch it shares)
// and its row sums of squares; the store kernel files both under the row's place in the T x m arrays of the call.  The
// mixture runs once, behind the last chunk.  Lanes 1 and 2 carry the streams; lane 0 - the fit - is not touched.
int gpmi_predict_batch(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                       const double* mus, const double* mu_const, const double* pts, int64_t m, const double* mu_q,
                       const double* weights, double* mean_t, double* var_t, double* mix_mean, double* mix_var, int* info) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, T >= 1 && T <= RED_SLOTS, "T out of range");
  ARGCHK(c, thetas && pts && m > 0, "thetas / pts is NULL or m <= 0");
  ARGCHK(c, mus || mu_const, "one of mus / mu_const is required");
  ARGCHK(c, mu_q || mu_const, "one of mu_q / mu_const is required");
  ARGCHK(c, mean_t || var_t || mix_mean, "no output requested");
  ARGCHK(c, mix_mean || !mix_var, "mix_var needs mix_mean");
  ARGCHK(c, c->n > 0, "gpmi_set_data has not been called");
  ARGCHK(c, c->np <= 4096 && !c->ycov, "gpmi_predict_batch: lockstep sizes only (n <= 4096, diagonal data errors)");
  ARGCHK(c, T * m <= ((int64_t)1 << 31), "T x m too large");
  if (weights) {
    double wsum = 0.0;
    for (int64_t t = 0; t < T; ++t) {
      ARGCHK(c, std::isfinite(weights[t]) && weights[t] >= 0.0, "weights must be finite and non-negative");
      wsum += weights[t];
    }
    ARGCHK(c, wsum > 0.0, "weights must have a positive sum");
  }
  if (int rc = set_device(c)) return rc;
  std::vector<KParams> ps;
  std::vector<CovParams> sps;  // (a sum: its parameters, ps stays empty)
  if (int rc = make_batch_params(c, kernel, T, thetas, n_theta, extra, ps, sps)) return rc;
  const BatchParams bp(kernel, ps, sps);
  ARGCHK(c, c->bpend[0] == 0 && c->bpend[1] == 0,
         "gpmi_predict_batch: an asynchronous batch is pending on this handle (gpmi_lml_batch_wait first)");
  if (int rc = ensure_lanes(c, 2)) return rc;
  if (int rc = ensure_batch_ws(c, (int)(T < 64 ? (T < 2 ? 2 : T) : 64))) return rc;
  if (int rc = ensure_batch_grad_ws(c, c->bcap, n_theta)) return rc;
  const bool want_var = var_t || mix_var;
  const int64_t P = GPMI_PREDICT_PANEL;
  const int64_t sQ = 2 * P * c->ld;  // per problem: the panel K* and, behind it, V = K* L^-T
  if (int rc = c->bQ.reserve(c, c->bgrad_cap * sQ)) return rc;
  const bool two = batch_split_enabled() && T >= 16 && ensure_lanes(c, 3) == GPMI_OK;
  const int cap = c->bgrad_cap;
  // the call's own device arrays: points, prior means at the points, the T x m results, the mixture's row list
  DevBuf<double> dPts, dPrior, dMean, dVar, dSq, dW, dMix;
  DevBuf<int> dIdx;
  if (int rc = dPts.alloc(c, m * c->d)) return rc;
  if (int rc = dPrior.alloc(c, mu_q ? T * m : T)) return rc;
  if (int rc = dMean.alloc(c, T * m)) return rc;
  if (want_var) {
    if (int rc = dVar.alloc(c, T * m)) return rc;
    if (int rc = dSq.alloc(c, P * cap)) return rc;
  }
  HIPCHK(c, hipMemcpy(dPts, pts, sizeof(double) * m * c->d, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dPrior, mu_q ? mu_q : mu_const, sizeof(double) * (mu_q ? T * m : T), hipMemcpyHostToDevice));
  HIPCHK(c, hipStreamSynchronize(nullptr));  // (the lanes' streams do not wait for the null stream)
  const int nt = (int)(c->np / GPMI_NB);
  auto enqueue = [&](hipStream_t s, int64_t t_first, int off, int B) -> int {
    const Chunk k(c, s, off, B, mus != nullptr);
    double* Q = c->bQ + (int64_t)off * sQ;
    double* V = Q + P * c->ld;
    HIPCHK(c, hipMemcpyAsync(bp.device(c, off), bp.host(t_first), bp.bytes_each() * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(k.Mu, mus ? mus + t_first * c->n : mu_const + t_first, sizeof(double) * B * (mus ? c->n : 1),
                             hipMemcpyHostToDevice, s));
    if (int rc = lockstep_stages(k, ChunkBuild::kernels(bp), LS_CLEAR_INFO | LS_BACKWARD | (want_var ? LS_INVERSE : 0u))) return rc;
    // slots 2 and 3 (2 np >= GPMI_PREDICT_PANEL doubles; the residual is spent) take a panel's row dots: launch_rows_dot
    // strides its output like alpha
    double* dot_dev = k.resid();
    double* sq_dev = want_var ? dSq + (int64_t)off * P : nullptr;
    GemmBatch gb{B, sQ, sQ, k.bs.sMat};
    gb.ring_order_only = true;
    for (int64_t m0 = 0; m0 < m; m0 += P) {
      const int64_t mc = (m - m0 < P) ? m - m0 : P;
      const int64_t mp = round_up(mc, GPMI_NB);
      launch_kbuild_cross_batched(k, bp, dPts + m0 * c->d, mc, mp, Q, sQ);
      launch_rows_dot(s, Q, c->ld, mc, c->np, k.alpha(), dot_dev, B, sQ, k.bs.sVec);
      if (want_var) {
        launch_gemm(s, TILES_RECT, OP_ASSIGN, true, 2, V, c->ld, Q, c->ld, k.B2, c->ld, (int)(mp / GPMI_NB), nt, (int)c->np,
                    nullptr, gb);
        launch_rows_sumsq(s, V, c->ld, mc, c->np, 0.0, sq_dev, B, sQ, P, -1.0);  // (-(0 - sum): the sum itself)
      }
      launch_predict_store(s, B, t_first, m0, mc, m, dot_dev, sq_dev, k.bs.sVec, P, bp.device(c, off), (int64_t)bp.bytes_each(),
                           k.info, mu_q ? dPrior : nullptr, mu_q ? nullptr : dPrior,
                           dMean, dVar);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_bInfo + off, k.info, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    return GPMI_OK;
  };
  std::vector<int> inf_all((size_t)T, 0);
  for (int64_t t0 = 0; t0 < T; t0 += cap) {
    const int B = (int)((T - t0 < cap) ? T - t0 : cap);
    const int B1 = (two && B >= 16) ? B / 2 : B;
    if (int rc = enqueue(c->lanes[1].stream, t0, 0, B1)) return rc;
    if (B1 < B)
      if (int rc = enqueue(c->lanes[2].stream, t0 + B1, B1, B - B1)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->lanes[1].stream));
    if (B1 < B) HIPCHK(c, hipStreamSynchronize(c->lanes[2].stream));
    for (int b = 0; b < B; ++b) {
      const int inf = c->h_bInfo[b];
      INFOCHK(c, inf);
      inf_all[(size_t)(t0 + b)] = inf;
      if (info) info[t0 + b] = inf;
    }
  }
  hipStream_t s = c->lanes[1].stream;
  if (mix_mean) {
    // the rows that factorised, in order, and their weights divided by their sum (equal weights: 1 / their number)
    std::vector<int> idx;
    std::vector<double> w;
    for (int64_t t = 0; t < T; ++t)
      if (inf_all[(size_t)t] == 0) {
        idx.push_back((int)t);
        w.push_back(weights ? weights[t] : 1.0);
      }
    const int64_t G = (int64_t)idx.size();
    const double wsum = weights ? tree_sum_host(w.data(), G) : (double)G;
    if (G == 0 || !(wsum > 0.0)) {
      for (int64_t q = 0; q < m; ++q) {
        mix_mean[q] = std::nan("");
        if (mix_var) mix_var[q] = std::nan("");
      }
    } else {
      for (double& v : w) v = weights ? v / wsum : 1.0 / (double)G;
      if (int rc = dIdx.alloc(c, G)) return rc;
      if (int rc = dW.alloc(c, G)) return rc;
      if (int rc = dMix.alloc(c, 2 * m)) return rc;
      HIPCHK(c, hipMemcpyAsync(dIdx, idx.data(), sizeof(int) * G, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(dW, w.data(), sizeof(double) * G, hipMemcpyHostToDevice, s));
      launch_predict_mix(s, G, dIdx, dW, m, dMean, dVar, dMix,
                         mix_var ? dMix + m : nullptr);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(mix_mean, dMix, sizeof(double) * m, hipMemcpyDeviceToHost, s));
      if (mix_var)
        HIPCHK(c, hipMemcpyAsync(mix_var, dMix + m, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    }
  }
  if (mean_t) HIPCHK(c, hipMemcpyAsync(mean_t, dMean, sizeof(double) * T * m, hipMemcpyDeviceToHost, s));
  if (var_t) HIPCHK(c, hipMemcpyAsync(var_t, dVar, sizeof(double) * T * m, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return GPMI_OK;
}

int gpmi_posterior(gpmi_ctx* c, const double* pts, int64_t m, double* mu_out, double* cov_out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted, "gpmi_posterior needs a successful gpmi_fit");
  ARGCHK(c, c->fit_params.kernel >= 0 || c->mix_nk > 0,
         "gpmi_posterior: the model was fitted with a caller-built covariance (gpmi_fit_dense) - use gpmi_predict_dense / gpmi_solve_rows");
  ARGCHK(c, pts && m > 0, "pts is NULL or m <= 0");
  if (int rc = set_device(c)) return rc;
  hipStream_t s = c->lanes[0].stream;
  const int64_t mp = round_up(m, GPMI_NB), ldq = mp + 32;
  if (int rc = ensure_query_ws(c, mp)) return rc;
  // (an error return below may leave work on Sigma in flight: hipFree waits for the device before it releases)
  DevBuf<double> Sigma;
  if (cov_out)
    if (int rc = Sigma.alloc(c, mp * ldq)) return rc;
  if (int rc = kernel_posterior_sigma(c, pts, m, mp, mu_out, Sigma, ldq)) return rc;
  if (cov_out)
    HIPCHK(c, hipMemcpy2DAsync(cov_out, sizeof(double) * m, Sigma, sizeof(double) * ldq, sizeof(double) * m, m,
                               hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return GPMI_OK;
}

int gpmi_spatial_derivatives(gpmi_ctx* c, const double* pts, int64_t m, double* dmu_out,
                             double* dvar_out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted, "gpmi_spatial_derivatives needs a successful gpmi_fit");
  ARGCHK(c, c->fit_params.kernel >= 0 || c->mix_nk > 0,
         "gpmi_spatial_derivatives: the model was fitted with a caller-built covariance (gpmi_fit_dense) - use gpmi_predict_dense / gpmi_solve_rows");
  ARGCHK(c, c->fit_params.kernel == GPMI_KERNEL_SE || c->fit_params.kernel == GPMI_KERNEL_PER || kernel_is_matern(c->fit_params.kernel),
         "spatial derivatives: SquaredExponential, Matern32, Matern52 and Periodic only (not sums of kernels)");
  ARGCHK(c, pts && m > 0 && dmu_out && dvar_out, "NULL argument or m <= 0");
  if (int rc = set_device(c)) return rc;
  Lane& L = c->lanes[0];
  hipStream_t s = L.stream;
  const CovParams& p = c->fit_params;
  const int64_t chunk = 1024, d = c->d;
  for (int64_t m0 = 0; m0 < m; m0 += chunk) {
    const int64_t mc = (m - m0 < chunk) ? m - m0 : chunk;
    const int64_t mp = round_up(mc, GPMI_NB);
    if (int rc = ensure_query_ws(c, mp)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * d, sizeof(double) * mc * d, hipMemcpyHostToDevice, s));
    launch_kbuild_cross(s, p, c->pts, mc, mp, c->x, c->n, c->np, c->Q, c->ld);
    launch_copy(s, c->Q, c->Q2, mp * c->ld);
    // Matern: the multiplier of the reductions is the derivative profile a^2 g, not K* (predgrad.hip); K* has been
    // copied for the solves, so c->Q is free to be rebuilt
    if (kernel_is_matern(p.kernel)) launch_kbuild_cross_dprofile(s, p, c->pts, mc, mp, c->x, c->n, c->np, c->Q, c->ld);
    // Z = K^-1 k per row: forward then backward solve (regression.py:410)
    if (int rc = enqueue_rows_kinv(c, L, s, mp)) return rc;
    double* dmu_dev = c->pvec;
    double* dvar_dev = c->pvec + mp * d;
    launch_sd_reduce(s, p, c->x, c->n, c->pts, mc, c->Q, c->ld, c->alpha, 0, 1.0, dmu_dev);
    launch_sd_reduce(s, p, c->x, c->n, c->pts, mc, c->Q, c->ld, c->Q2, c->ld, -2.0, dvar_dev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(dmu_out + m0 * d, dmu_dev, sizeof(double) * mc * d, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(dvar_out + m0 * d, dvar_dev, sizeof(double) * mc * d, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return GPMI_OK;
}

int gpmi_gradient(gpmi_ctx* c, const double* pts, int64_t m, double* gmu_out, double* gcov_out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted, "gpmi_gradient needs a successful gpmi_fit");
  ARGCHK(c, c->fit_params.kernel >= 0 || c->mix_nk > 0,
         "gpmi_gradient: the model was fitted with a caller-built covariance (gpmi_fit_dense) - use gpmi_predict_dense / gpmi_solve_rows");
  ARGCHK(c, c->fit_params.kernel == GPMI_KERNEL_SE || c->fit_params.kernel == GPMI_KERNEL_PER || kernel_is_matern(c->fit_params.kernel),
         "gradient: SquaredExponential, Matern32, Matern52 and Periodic only (not sums of kernels)");
  ARGCHK(c, pts && m > 0 && gmu_out && gcov_out, "NULL argument or m <= 0");
  if (int rc = set_device(c)) return rc;
  Lane& L = c->lanes[0];
  hipStream_t s = L.stream;
  const CovParams& p = c->fit_params;
  const int64_t d = c->d;
  int64_t chunk = 1024 / d;  // d right-hand sides per point
  if (chunk < 1) chunk = 1;
  for (int64_t m0 = 0; m0 < m; m0 += chunk) {
    const int64_t mc = (m - m0 < chunk) ? m - m0 : chunk;
    const int64_t rp = round_up(mc * d, GPMI_NB);
    if (int rc = ensure_query_ws(c, rp)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * d, sizeof(double) * mc * d, hipMemcpyHostToDevice, s));
    // c->Q is only ever the multiplier of the two kernels below: K* for SE, the derivative profile a^2 g for Matern
    if (kernel_is_matern(p.kernel))
      launch_kbuild_cross_dprofile(s, p, c->pts, mc, round_up(mc, GPMI_NB), c->x, c->n, c->np, c->Q, c->ld);
    else
      launch_kbuild_cross(s, p, c->pts, mc, round_up(mc, GPMI_NB), c->x, c->n, c->np, c->Q, c->ld);
    double* gmu_dev = c->pvec;
    double* gcov_dev = c->pvec + rp;
    launch_sd_reduce(s, p, c->x, c->n, c->pts, mc, c->Q, c->ld, c->alpha, 0, 1.0, gmu_dev);
    launch_grad_rhs(s, p, c->x, c->n, c->np, c->pts, mc * d, rp, c->Q, c->ld, c->Q2);
    if (int rc = ensure_inv2(c, L, s)) return rc;
    trsm_rows_forward(c, s, L.A, c->np, c->ld, L.inv2, c->Q2, rp, false, c->Q, nullptr);  // c->Q is free again
    launch_grad_cov(s, p, c->Q, c->ld, c->np, mc, gcov_dev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(gmu_out + m0 * d, gmu_dev, sizeof(double) * mc * d, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(gcov_out + m0 * d * d, gcov_dev, sizeof(double) * mc * d * d,
                             hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return GPMI_OK;
}

int gpmi_loo_diag(gpmi_ctx* c, double* ikdiag) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted && ikdiag, "gpmi_loo_diag needs a successful gpmi_fit");
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_lanes(c, 2)) return rc;
  Lane& F = c->lanes[0];
  Lane& L = c->lanes[1];
  if (int rc = ensure_second_matrix(c, L)) return rc;
  HIPCHK(c, hipStreamSynchronize(F.stream));
  // diag(K^-1)_a = sum_i (L^-1)_ia^2 = squared norm of row a of L^-T   (regression.py:460-462)
  if (int rc = enqueue_inverse_factor(c, L, F)) return rc;
  launch_rows_sumsq(L.stream, L.B2, c->ld, c->np, c->np, 0.0, L.vec);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(ikdiag, L.vec, sizeof(double) * c->n, hipMemcpyDeviceToHost, L.stream));
  HIPCHK(c, hipStreamSynchronize(L.stream));
  for (int64_t i = 0; i < c->n; ++i) ikdiag[i] = -ikdiag[i];  // rows_sumsq returns base - sum
  return GPMI_OK;
}

int gpmi_loo_terms(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag,
                   const double* mu, double* alpha_out, double* ikdiag, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, mu && alpha_out && ikdiag, "mu / alpha / ikdiag is NULL");
  if (int rc = set_device(c)) return rc;
  return lane_loo_terms(LaneEval(c, 1), LaneBuild::kernels(p), mu, alpha_out, ikdiag, info);
}

int gpmi_loo_grad(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag,
                  const double* mu, double* alpha_out, double* ikdiag, double* p_out,
                  double* grad_theta, double* trace_q, int* info) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, mu && alpha_out && ikdiag && p_out && grad_theta, "NULL argument");
  if (int rc = set_device(c)) return rc;
  const LaneEval ev(c, 1);
  if (int rc = lane_stages(ev, LaneBuild::kernels(p), LN_BACKWARD | LN_INVERSE | LN_LOO, mu, n_theta)) return rc;
  lane_loo_middle(ev, true, true, false);
  launch_lml_grad(ev.stream(), p, n_theta, c->x, c->n, c->np, ev.L().A, c->ld, ev.loo_p(), ev.alpha(), ev.partial(true), ev.gout());
  const int rc = lane_collect(ev, 0, n_theta + 1, {{alpha_out, ev.alpha()}, {ikdiag, ev.loo_diag()}, {p_out, ev.loo_p()}}, nullptr, info);
  // the contraction returns 1/2 sum Q o dK; the LOO gradient has no 1/2 (regression.py:513)
  for (int j = 0; j < n_theta; ++j) grad_theta[j] = 2.0 * ev.h_gout()[j];
  if (trace_q) *trace_q = ev.h_gout()[n_theta];
  return rc;
}

int gpmi_covariance(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra_diag,
                    int with_noise, double* K_host) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = make_cov(c, kernel, theta, n_theta, extra_diag, p)) return rc;
  ARGCHK(c, K_host != nullptr, "K_host is NULL");
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_lanes(c, 2)) return rc;
  Lane& L = c->lanes[1];
  DevBuf<double> zeros;  // (an error return below may leave the build reading it: hipFree waits for the device before it releases)
  if (!with_noise) {
    if (int rc = zeros.alloc(c, c->np)) return rc;
    HIPCHK(c, hipMemsetAsync(zeros, 0, sizeof(double) * c->np, L.stream));
  }
  launch_kbuild_square(L.stream, p, c->x, c->n, c->np, with_noise ? c->noise : zeros, L.A, c->ld, false);
  if (with_noise && c->ycov) launch_add_full(L.stream, L.A, c->ld, c->ycov, c->n);
  HIPCHK(c, hipMemcpy2DAsync(K_host, sizeof(double) * c->n, L.A, sizeof(double) * c->ld, sizeof(double) * c->n, c->n,
                             hipMemcpyDeviceToHost, L.stream));
  HIPCHK(c, hipStreamSynchronize(L.stream));
  return GPMI_OK;
}

int gpmi_cross_covariance(gpmi_ctx* c, int kernel, const double* theta, int n_theta,
                          const double* pts, int64_t m, double* out) {
  if (!c) return GPMI_ERR_ARG;
  CovParams p;
  if (int rc = make_cov(c, kernel, theta, n_theta, 0.0, p)) return rc;
  ARGCHK(c, pts && out && m > 0, "pts / out is NULL or m <= 0");
  if (int rc = set_device(c)) return rc;
  hipStream_t s = c->lanes[0].stream;
  const int64_t chunk = 2048;
  for (int64_t m0 = 0; m0 < m; m0 += chunk) {
    const int64_t mc = (m - m0 < chunk) ? m - m0 : chunk;
    const int64_t mp = round_up(mc, GPMI_NB);
    if (int rc = ensure_query_ws(c, mp)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pts, pts + m0 * c->d, sizeof(double) * mc * c->d,
                             hipMemcpyHostToDevice, s));
    launch_kbuild_cross(s, p, c->pts, mc, mp, c->x, c->n, c->np, c->Q, c->ld);
    HIPCHK(c, hipMemcpy2DAsync(out + m0 * c->n, sizeof(double) * c->n, c->Q, sizeof(double) * c->ld,
                               sizeof(double) * c->n, mc, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return GPMI_OK;
}

int gpmi_get_K(gpmi_ctx* c, double* K_host) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted && K_host, "gpmi_get_K needs a successful gpmi_fit");
  ARGCHK(c, c->fit_params.kernel >= 0, "gpmi_get_K: the covariance of this fit was built by the caller (gpmi_fit_dense / gpmi_fit_mix)");
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_lanes(c, 2)) return rc;
  Lane& L = c->lanes[1];
  launch_kbuild_square(L.stream, c->fit_params, c->x, c->n, c->np, c->noise, L.A, c->ld, false);
  if (c->ycov) launch_add_full(L.stream, L.A, c->ld, c->ycov, c->n);
  HIPCHK(c, hipMemcpy2DAsync(K_host, sizeof(double) * c->n, L.A, sizeof(double) * c->ld,
                             sizeof(double) * c->n, c->n, hipMemcpyDeviceToHost, L.stream));
  HIPCHK(c, hipStreamSynchronize(L.stream));
  return GPMI_OK;
}

int gpmi_get_L(gpmi_ctx* c, double* L_host) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, c->fitted && L_host, "gpmi_get_L needs a successful gpmi_fit");
  if (int rc = set_device(c)) return rc;
  Lane& L = c->lanes[0];
  HIPCHK(c, hipMemcpy2DAsync(L_host, sizeof(double) * c->n, L.A, sizeof(double) * c->ld,
                             sizeof(double) * c->n, c->n, hipMemcpyDeviceToHost, L.stream));
  HIPCHK(c, hipStreamSynchronize(L.stream));
  for (int64_t i = 0; i < c->n; ++i)
    for (int64_t j = i + 1; j < c->n; ++j) L_host[i * c->n + j] = 0.0;  // numpy returns the upper triangle zeroed
  return GPMI_OK;
}

}  // extern "C"
