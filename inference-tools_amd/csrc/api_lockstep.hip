// What the lockstep batch entry points of api_regression.hip and api_mix.hip share (np <= 4096, every launch carrying a
// chunk of problems in blockIdx.z): the view of a chunk, the stages from the covariance build to the solves, the
// leave-one-out middle part, the mixture batches' workspace, staging and per-sub-kernel terms.  Host code only.
// Uploads and downloads stay with the entry points: each keeps its own mechanism (api_internal.h: lockstep_stages).
#include "api_internal.h"

bool batch_split_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("GPMI_BATCH_SPLIT");
    return !e || std::atoi(e) != 0;
  }();
  return on;
}

Chunk::Chunk(gpmi_ctx* ctx, hipStream_t s, int first, int count, bool mean_rows)
    : c(ctx), stream(s), off(first), B(count), mu_rows(mean_rows),
      bs{count, ctx->np * ctx->ld, (ctx->np / GPMI_NB) * GPMI_NB * GPMI_NB, 4 * ctx->np} {
  A = c->bA + (int64_t)off * bs.sMat;
  Inv = c->bInv + (int64_t)off * bs.sInv;
  Vec = c->bVec + (int64_t)off * bs.sVec;
  Mu = c->bMu + (int64_t)off * (mu_rows ? c->n : 1);
  B2 = c->bB2 ? c->bB2 + (int64_t)off * bs.sMat : nullptr;
  red = c->bRed + 2 * off;
  info = c->bInfo + off;
}

int Chunk::clear_info() const {
  HIPCHK(c, hipMemsetAsync(info, 0, sizeof(int) * B, stream));
  return GPMI_OK;
}

void Chunk::syrk(int kskip) const {
  const int nt = (int)(c->np / GPMI_NB);
  launch_gemm(stream, TILES_LOWER, OP_ASSIGN, false, kskip, A, c->ld, B2, c->ld, B2, c->ld, nt, nt, (int)c->np, nullptr,
              GemmBatch{B, bs.sMat, bs.sMat, bs.sMat});
}

void launch_kbuild_cross_batched(const Chunk& k, const BatchParams& p, const double* U, int64_t mu, int64_t mp, double* out,
                                 int64_t stride) {
  gpmi_ctx* c = k.c;
  if (p.sum)
    launch_kbuild_cross_batched(k.stream, c->bSum + k.off, k.B, U, mu, mp, c->x, c->n, c->np, out, c->ld, stride, (int)c->d);
  else
    launch_kbuild_cross_batched(k.stream, p.kernel, c->bParams + k.off, k.B, U, mu, mp, c->x, c->n, c->np, out, c->ld, stride,
                                (int)c->d);
}

void launch_lml_grad_batched(const Chunk& k, const BatchParams& p, int n_theta, const double* u, const double* v, int64_t sV) {
  gpmi_ctx* c = k.c;
  if (p.sum)
    launch_lml_grad_batched(k.stream, c->bSum + k.off, k.B, n_theta, c->x, c->n, c->np, k.A, c->ld, k.bs.sMat, u, v, sV,
                            c->bGws, c->bGout, (int)c->d, uses_periodic(c, GPMI_KERNEL_SUM));
  else
    launch_lml_grad_batched(k.stream, p.kernel, c->bParams + k.off, k.B, n_theta, c->x, c->n, c->np, k.A, c->ld, k.bs.sMat, u,
                            v, sV, c->bGws, c->bGout);
}

int lockstep_stages(const Chunk& k, const ChunkBuild& b, unsigned steps) {
  gpmi_ctx* c = k.c;
  hipStream_t s = k.stream;
  if (steps & LS_CLEAR_INFO)
    if (int rc = k.clear_info()) return rc;
  if (b.mix) {
    ARGCHK(c, k.off == 0, "internal: a mixture chunk starts at problem 0");
    // the sub-kernels' lower tiles into the second matrix, folded into the first (the upper triangle of the sum is never
    // read before a mirror)
    const int64_t cap = c->bgrad_cap;
    for (int m = 0; m < b.mix->nk; ++m) {
      const double* gm = c->bMixG + (int64_t)m * c->np;
      launch_kbuild_square_batched(s, b.mix->kernels[m], c->bMixP + m * cap, k.B, c->x, c->n, c->np, c->mix_zero, k.B2, c->ld,
                                   k.bs.sMat, (int)c->d, 0);
      launch_scale_add(s, k.A, c->ld, k.B2, c->ld, gm, gm, c->np, c->np, m > 0, k.B, k.bs.sMat, k.bs.sMat, b.mix->sG(c));
    }
    launch_add_diag_vec(s, k.A, c->ld, c->noise, 0.0, c->n, k.B, k.bs.sMat, c->bMixExtra);
  } else if (b.p->sum) {  // (sums take no per-problem noise: the *_noise entry points refuse them)
    launch_kbuild_square_batched(s, c->bSum + k.off, k.B, c->x, c->n, c->np, c->noise, k.A, c->ld, k.bs.sMat, (int)c->d);
  } else {
    launch_kbuild_square_batched(s, b.p->kernel, c->bParams + k.off, k.B, c->x, c->n, c->np, b.noise ? b.noise : c->noise, k.A,
                                 c->ld, k.bs.sMat, (int)c->d, b.noise ? c->np : 0);
  }
  potrf_lower_batched(c, s, k.A, c->np, c->ld, k.Inv, k.info, k.bs);
  launch_residual_batched(s, c->y, k.mu_rows ? k.Mu : nullptr, k.mu_rows ? nullptr : k.Mu, k.resid(), c->n, c->np, k.bs);
  trsv_forward(c, s, k.A, c->np, c->ld, k.Inv, k.resid(), k.v(), k.info, k.bs);
  if (steps & LS_REDUCE) launch_lml_reduce(s, k.v(), k.A, c->ld, c->np, k.red, k.bs);
  if (steps & LS_BACKWARD) trsv_backward(c, s, k.A, c->np, c->ld, k.Inv, k.v(), k.alpha(), k.info, k.bs);
  if (steps & LS_INVERSE) trsm_identity_batched(s, k.A, c->np, c->ld, k.Inv, k.B2, k.bs);
  return GPMI_OK;
}

int stage_batch_inputs(RowStage& stage, const Chunk& k, const BatchParams& p, int64_t t0, const double* mus,
                       const double* mu_const) {
  gpmi_ctx* c = k.c;
  if (int rc = stage.put_copy(p.device(c, k.off), p.host(t0), p.bytes_each() * k.B)) return rc;  // (inputs leave from pinned memory)
  if (mus) return stage.put_copy(k.Mu, mus + t0 * c->n, sizeof(double) * k.B * c->n);
  return stage.put_copy(k.Mu, mu_const + t0, sizeof(double) * k.B);
}

void loo_middle(const Chunk& k, const LooVectors& lv, bool want_mdiag, bool mirror_m) {
  gpmi_ctx* c = k.c;
  hipStream_t s = k.stream;
  const int64_t sMat = k.bs.sMat, sLoo = lv.sLoo;
  // the row sums of squares of L^-T = diag(K^-1), then K^-1 in full (both triangles)
  launch_rows_sumsq(s, k.B2, c->ld, c->np, c->np, 0.0, lv.diag, k.B, sMat, sLoo, -1.0);
  k.syrk(1);
  launch_mirror_lower(s, k.A, c->ld, c->np, k.B, sMat);
  launch_loo_vectors(s, k.alpha(), lv.diag, lv.c1, lv.sc2, c->n, c->np, k.B, k.bs.sVec, sLoo);
  launch_rows_dot(s, k.A, c->ld, c->np, c->np, lv.c1, lv.p, k.B, sMat, sLoo);
  // M = K^-1 diag(c2) K^-1 = G G^T with G = K^-1 diag(sqrt c2); lower tiles, overwriting K^-1
  launch_scale_columns(s, k.A, lv.sc2, k.B2, c->ld, c->np, k.B, sMat, sLoo);
  // M_ii = |row i of G|^2 (sqrt(c2) is spent once G exists)
  if (want_mdiag) launch_rows_sumsq(s, k.B2, c->ld, c->np, c->np, 0.0, lv.sc2, k.B, sMat, sLoo, -1.0);
  k.syrk(0);
  if (mirror_m) launch_mirror_lower(s, k.A, c->ld, c->np, k.B, sMat);
}

// ---- mixture batches ---------------------------------------------------------------------------------------------
int ensure_batch_mix_ws(gpmi_ctx* c) {
  if (!c->mix_zero)
    if (int rc = c->mix_zero.alloc_zeroed(c, c->np)) return rc;
  const int cap = c->bgrad_cap;
  if (c->bMix_cap >= cap) return GPMI_OK;
  c->bMix_cap = 0;
  for (DevBuf<double>* q : {&c->bMixG, &c->bMixH, &c->bMixW, &c->bMixExtra}) q->release();
  c->bMixP.release();
  if (int rc = c->bMixG.alloc(c, (int64_t)cap * GPMI_MAX_MIX * c->np)) return rc;
  // (row sums and the caller's row-sum weights: up to two per sub-kernel)
  if (int rc = c->bMixH.alloc(c, (int64_t)cap * 2 * GPMI_MAX_MIX * c->np)) return rc;
  if (int rc = c->bMixW.alloc(c, (int64_t)cap * 2 * GPMI_MAX_MIX * c->np)) return rc;
  if (int rc = c->bMixExtra.alloc(c, cap)) return rc;
  if (int rc = c->bMixP.alloc(c, (int64_t)cap * GPMI_MAX_MIX)) return rc;
  c->bMix_cap = cap;
  return GPMI_OK;
}

// ps[m][t]
int make_mix_batch_params(gpmi_ctx* c, const MixBatch& mx, int64_t T, const double* thetas, std::vector<KParams>& ps) {
  ps.resize((size_t)mx.nk * T);
  for (int64_t t = 0; t < T; ++t) {
    int off = 0;
    for (int m = 0; m < mx.nk; ++m) {
      NO_PERIODIC(c, mx.kernels[m]);
      if (int rc = make_params(c, mx.kernels[m], thetas + t * mx.tot_nt + off, mx.n_thetas[m], 0.0, ps[(size_t)m * T + t]))
        return rc;
      off += mx.n_thetas[m];
    }
  }
  return GPMI_OK;
}

// weights, padded like mix_prepare does (the identity in the padding belongs to sub-kernel 0); every input of the chunk
// is laid out in the pinned staging buffer and leaves from there (RowStage, api_internal.h)
int stage_mix_inputs(RowStage& stage, const Chunk& k, const MixBatch& mx, int64_t t0, int64_t T, const std::vector<KParams>& ps,
                     const double* g_host, const double* hw_host, const double* extra, const double* mus,
                     const double* mu_const) {
  gpmi_ctx* c = k.c;
  const int B = k.B, nk = mx.nk;
  const int64_t sG = mx.sG(c), sW = mx.sW(c);
  double* gpad = stage.host(sizeof(double) * B * sG);
  std::fill(gpad, gpad + (size_t)B * sG, 0.0);
  for (int b = 0; b < B; ++b)
    for (int m = 0; m < nk; ++m) {
      double* dst = gpad + (size_t)b * sG + (size_t)m * c->np;
      const double* src = g_host + ((t0 + b) * nk + m) * c->n;
      for (int64_t i = 0; i < c->np; ++i) dst[i] = i < c->n ? src[i] : (m == 0 ? 1.0 : 0.0);
    }
  if (int rc = stage.put(c->bMixG, gpad, sizeof(double) * B * sG)) return rc;
  if (hw_host) {
    double* wpad = stage.host(sizeof(double) * B * sW);
    std::fill(wpad, wpad + (size_t)B * sW, 0.0);
    for (int b = 0; b < B; ++b)
      for (int row = 0; row < 2 * nk; ++row)
        std::copy(hw_host + ((t0 + b) * 2 * nk + row) * c->n, hw_host + ((t0 + b) * 2 * nk + row + 1) * c->n,
                  wpad + (size_t)b * sW + (size_t)row * c->np);
    if (int rc = stage.put(c->bMixW, wpad, sizeof(double) * B * sW)) return rc;
  }
  double* ex = stage.host(sizeof(double) * B);
  for (int b = 0; b < B; ++b) ex[b] = extra ? extra[t0 + b] : 0.0;
  if (int rc = stage.put(c->bMixExtra, ex, sizeof(double) * B)) return rc;
  for (int m = 0; m < nk; ++m)
    if (int rc = stage.put_copy(c->bMixP + (int64_t)m * c->bgrad_cap, ps.data() + (size_t)m * T + t0, sizeof(KParams) * B)) return rc;
  if (mus) return stage.put_copy(k.Mu, mus + t0 * c->n, sizeof(double) * B * c->n);
  return stage.put_copy(k.Mu, mu_const + t0, sizeof(double) * B);
}

void mix_sub_kernel_terms(const Chunk& k, const MixBatch& mx, const double* p, int64_t sP) {
  gpmi_ctx* c = k.c;
  hipStream_t s = k.stream;
  const int B = k.B;
  const int64_t sMat = k.bs.sMat, sVec = k.bs.sVec, sG = mx.sG(c), cap = c->bgrad_cap;
  double* ua = k.resid();             // (the residual is spent) g_m o alpha, or g_m o p
  double* va = p ? k.slot3() : ua;    // g_m o alpha
  for (int m = 0; m < mx.nk; ++m) {
    const double* gm = c->bMixG + (int64_t)m * c->np;
    const KParams* pm = c->bMixP + (int64_t)m * cap;
    // 1/2 sum (D_m Q D_m) o dK_m: the fused contraction on the weight-scaled matrix
    launch_scale_add(s, k.B2, c->ld, k.A, c->ld, gm, gm, c->np, c->np, false, B, sMat, sMat, sG);
    if (p) launch_vec_mul(s, gm, p, ua, c->np, B, sG, sP, sVec);
    launch_vec_mul(s, gm, k.alpha(), va, c->np, B, sG, sVec, sVec);
    launch_lml_grad_batched(s, mx.kernels[m], pm, B, mx.n_thetas[m], c->x, c->n, c->np, k.B2, c->ld, sMat, ua, va, sVec, c->bGws,
                            c->bGout + (int64_t)m * cap * mx.W());
    // window parameters: h_m(i) = sum_j Q_ij K_m,ij g_m(j) on the full K_m (lower tiles built, then mirrored)
    launch_kbuild_square_batched(s, mx.kernels[m], pm, B, c->x, c->n, c->np, c->mix_zero, k.B2, c->ld, sMat, (int)c->d, 0);
    launch_mirror_lower(s, k.B2, c->ld, c->np, B, sMat);
    if (mx.nrow == 1)
      launch_mix_rowsum(s, k.A, k.B2, c->ld, k.alpha(), gm, c->bMixH + (int64_t)m * c->np, c->n, B, sMat, sVec, sG, p, sP);
    else  // (weights and rows share the stride, bMixG's differs; the sub-kernel's two window factors in one pass)
      launch_mix_rowsum(s, k.A, k.B2, c->ld, k.alpha(), c->bMixW + (int64_t)(2 * m) * c->np, c->bMixH + (int64_t)(2 * m) * c->np,
                        c->n, B, sMat, sVec, mx.sW(c), p, sP, c->np);
  }
}

void unpack_mix_gradient(const gpmi_ctx* c, const MixBatch& mx, int b, double factor, double* out) {
  for (int m = 0; m < mx.nk; ++m)
    for (int j = 0; j < mx.n_thetas[m]; ++j)
      *out++ = factor * c->h_bGout[(int64_t)m * c->bgrad_cap * mx.W() + (int64_t)b * (mx.n_thetas[m] + 1) + j];
}
