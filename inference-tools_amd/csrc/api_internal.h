// Shared by the translation units of the C-ABI (api.hip: handle, lanes, workspaces, lifecycle, instrumentation;
// api_regression.hip: the GpRegressor entry points; api_mix.hip: ChangePoint mixtures and per-point noise; api_lockstep.hip:
// the chunk pipeline every lockstep batch entry point of those two runs - Chunk, BatchParams, lockstep_stages, the
// leave-one-out middle part, the mixture batches' workspace and staging; api_single.hip: the lane pipeline of their
// single-evaluation entry points - LaneEval, LaneBuild, lane_stages, lane_loo_middle, lane_collect; api_linv.hip:
// GpLinearInverter; api_dense.hip: plugin covariance functions and the rank-one append): error macros and the helpers
// every entry point is built from.
// Internal - the public interface is include/gpmi.h.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <thread>

#include "gpmi_internal.h"

#define HIPCHK(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) {                                                                \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                      \
      return (e__ == hipErrorOutOfMemory) ? GPMI_ERR_NOMEM : GPMI_ERR_HIP;                  \
    }                                                                                       \
  } while (0)

#define ARGCHK(ctx, cond, msg) \
  do {                         \
    if (!(cond)) {             \
      (ctx)->err = (msg);      \
      return GPMI_ERR_ARG;     \
    }                          \
  } while (0)

// hipMemset on device memory returns once the fill is ENQUEUED in the null stream, and the library's streams are
// non-blocking: they do not wait for the null stream.  A buffer whose zeros later kernels rely on (the upper 16-blocks
// of the inverse diagonal blocks, the padding of x / y / noise, the zero vectors) is therefore zeroed AND waited for.
// (Round 5: with eight processes time-slicing one device the fill of `invD` arrived milliseconds late and wiped inverse
// blocks that potrf_diag had already written - pivot failures in the second or third diagonal block, a few per
// thousand evaluations; with the device to itself the fill always won the race.)
#define ZERO_SYNC(ctx, ptr, bytes)                          \
  do {                                                      \
    HIPCHK(ctx, hipMemset((ptr), 0, (bytes)));              \
    HIPCHK(ctx, hipStreamSynchronize(nullptr));             \
  } while (0)

// a negative `info` is written by the flag-ordered kernels when a poll timed out: GPMI_INFO_FLOW_TIMEOUT by the tile-task
// factorisation (potrf_flow.hip) - the one case the stream-ordered schedule (GPMI_OPT_NO_FLOW) cures, marked "[flow-tail]"
// in the error text for the caller that wants to repeat the call -, GPMI_ERR_INTERNAL by the triangular sweeps
#define INFOCHK(ctx, inf)                                                                                     \
  do {                                                                                                        \
    if ((inf) != 0 && std::getenv("GPMI_DEBUG_INFO"))                                                         \
      std::fprintf(stderr, "[gpmi] %s: info = %d (n = %lld)\n", __func__, (int)(inf), (long long)(ctx)->n);    \
    if ((inf) < 0) {                                                                                          \
      (ctx)->err = (inf) == GPMI_INFO_FLOW_TIMEOUT                                                            \
                       ? "internal error: the tile-task factorisation timed out [flow-tail]"                  \
                       : "internal error: a flag-ordered triangular sweep timed out";                         \
      return GPMI_ERR_INTERNAL;                                                                               \
    }                                                                                                         \
  } while (0)

constexpr int RED_SLOTS = 8192;  // per-lane result slots for batched evaluations

// one evaluation of the mixture covariance K = sum_m diag(g_m) K_m diag(g_m) + extra I (+ data errors)
struct MixEval {
  int nk;
  const KParams* p;   // nk sub-kernels (their extra_diag is ignored)
  const double* g;    // nk x np device weights (row m: g_m; padding 1 for m = 0, else 0)
  double extra;       // WhiteNoise variance
  double* scratch;    // np x ld
  const double* zero; // np zeros
};

extern thread_local std::string g_create_err;

// Inputs and outputs of a lockstep chunk between the CALLER's (pageable) host arrays and the device: everything is laid
// out in the handle's pinned, device-mapped staging buffer (allocated once per handle) and moved by a copy kernel that
// reads / writes that buffer over the bus - strided rows packed on the fly, no hipMemcpy2DAsync, no pageable memory handed
// to the runtime, and no per-call host allocation (the std::vector pads of round 5 were 0.4 - 0.8 MB of malloc / free per
// call: part of the heap churn behind the 28 ms batch calls of profiles/r06_search_regression.txt; the cure of that
// stall itself is keep_heap_top_once() in api.hip).
// Usage: reserve() the bytes of a chunk; host() + put() / put_copy() / up() for inputs; down() for outputs;
// hipStreamSynchronize; finish() (pinned -> caller).
struct RowStage {
  gpmi_ctx* c;
  hipStream_t s;
  size_t used = 0;
  struct Item {
    char* dst;
    size_t dpitch, off, width, height;
  };
  std::vector<Item> items;
  RowStage(gpmi_ctx* ctx, hipStream_t stream) : c(ctx), s(stream) {}
  // capacity for everything staged until the next finish(); only while nothing is staged
  int reserve(size_t bytes) {
    return c->h_stage.reserve(c, (int64_t)bytes, hipHostMallocMapped | hipHostMallocPortable);
  }
  size_t take(size_t bytes) {
    const size_t off = used;
    used += (bytes + 255) & ~(size_t)255;
    return off;
  }
  // pinned scratch of `bytes` (a multiple of 8) the caller fills in place, then put()
  double* host(size_t bytes) { return reinterpret_cast<double*>(c->h_stage + take(bytes)); }
  int put(void* dst_dev, const double* pinned, size_t bytes) {
    ARGCHK(c, used <= (size_t)c->h_stage.capacity() && bytes % 8 == 0, "internal: staging buffer too small");
    launch_copy_rows(s, pinned, 0, static_cast<double*>(dst_dev), 0, (int64_t)(bytes / 8), 1);
    return GPMI_OK;
  }
  // a contiguous caller array -> device
  int put_copy(void* dst_dev, const void* src, size_t bytes) {
    const size_t padded = (bytes + 7) & ~(size_t)7;
    ARGCHK(c, used + padded + 256 <= (size_t)c->h_stage.capacity(), "internal: staging buffer too small");
    double* p = host(padded);
    std::memcpy(p, src, bytes);
    return put(dst_dev, p, padded);
  }
  // caller rows (pitch `spitch` bytes) -> device rows (pitch `dpitch` bytes)
  int up(void* dst_dev, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
    ARGCHK(c, used + width * height + 256 <= (size_t)c->h_stage.capacity(), "internal: staging buffer too small");
    double* p = host(width * height);
    for (size_t r = 0; r < height; ++r)
      std::memcpy(reinterpret_cast<char*>(p) + r * width, static_cast<const char*>(src) + r * spitch, width);
    launch_copy_rows(s, p, (int64_t)(width / 8), static_cast<double*>(dst_dev), (int64_t)(dpitch / 8), (int64_t)(width / 8),
                     (int64_t)height);
    return GPMI_OK;
  }
  // `height` device rows of `width` bytes (pitch `spitch`) -> caller rows (pitch `dpitch`), after the sync and finish()
  int down(void* dst, size_t dpitch, const void* src_dev, size_t spitch, size_t width, size_t height) {
    ARGCHK(c, used + width * height + 256 <= (size_t)c->h_stage.capacity(), "internal: staging buffer too small");
    const size_t off = take(width * height);
    launch_copy_rows(s, static_cast<const double*>(src_dev), (int64_t)(spitch / 8),
                     reinterpret_cast<double*>(c->h_stage + off), (int64_t)(width / 8),
                     (int64_t)(width / 8), (int64_t)height);
    items.push_back({static_cast<char*>(dst), dpitch, off, width, height});
    return GPMI_OK;
  }
  // after the stream has been synchronised
  void finish() {
    const char* base = c->h_stage;
    for (const Item& it : items)
      for (size_t r = 0; r < it.height; ++r) std::memcpy(it.dst + r * it.dpitch, base + it.off + r * it.width, it.width);
    items.clear();
    used = 0;
  }
};

// api.hip
int lane_streams(gpmi_ctx* c, Lane& L);
bool ensure_masked_pair(gpmi_ctx* c, Lane& L, int k);
int lane_masked_streams(gpmi_ctx* c, Lane& L);
int lane_alloc(gpmi_ctx* c, Lane& L);
void lane_free(Lane& L);
int ensure_lanes(gpmi_ctx* c, size_t count);
void free_data(gpmi_ctx* c);
// The entry points without Periodic kernels (the exact Hessian, many targets, the generalised GP, the linear inversion,
// the ChangePoint mixtures) refuse GPMI_KERNEL_PER - alone or as a component of the handle's sum - before they build
// parameters or launch anything.
inline bool uses_periodic(const gpmi_ctx* c, int kernel) {
  if (kernel == GPMI_KERNEL_PER) return true;
  if (kernel == GPMI_KERNEL_SUM)
    for (int m = 0; m < c->sum_nk; ++m)
      if (c->sum_kinds[m] == GPMI_KERNEL_PER) return true;
  return false;
}
#define NO_PERIODIC(ctx, kernel) \
  ARGCHK(ctx, !uses_periodic(ctx, kernel), "GPMI_KERNEL_PER is not supported by this entry point")

int make_params(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra, KParams& p);
// make_params for the entry points that also take sums (GPMI_KERNEL_SUM: the layout of gpmi_set_sum)
int make_cov(gpmi_ctx* c, int kernel, const double* theta, int n_theta, double extra, CovParams& p);
// T evaluations: single kernels into ps, sums into sps (the other vector is left empty)
int make_batch_params(gpmi_ctx* c, int kernel, int64_t T, const double* thetas, int n_theta, const double* extra,
                      std::vector<KParams>& ps, std::vector<CovParams>& sps);
int set_device(gpmi_ctx* c);
void build_mix_square(gpmi_ctx* c, hipStream_t s, const MixEval& mx, double* dst, bool lower_only);
int enqueue_factor_and_forward(gpmi_ctx* c, Lane& L, const CovParams& p, const double* mu_dev, double mu_const, int slot, bool allow_lookahead = true,
                               const MixEval* mix = nullptr, bool prebuild_inv2 = false, double* backward_out = nullptr,
                               double* early_identity = nullptr);
int ensure_second_matrix(gpmi_ctx* c, Lane& L);
int ensure_inv2(gpmi_ctx* c, Lane& F, hipStream_t s);
int ensure_trsm_panel(gpmi_ctx* c, int64_t rows);
int enqueue_inverse_factor(gpmi_ctx* c, Lane& L, Lane& F);
int enqueue_rows_kinv(gpmi_ctx* c, Lane& F, hipStream_t s, int64_t mp);
void free_batch_ws(gpmi_ctx* c);  // every lockstep buffer, caps to 0
int64_t batch_budget_bytes();     // GPMI_BATCH_GIB (1 .. 200 GiB, else and by default 24) in bytes: the cap of a lockstep workspace
int ensure_batch_ws(gpmi_ctx* c, int want);
int ensure_batch_grad_ws(gpmi_ctx* c, int want, int n_theta);
int ensure_query_ws(gpmi_ctx* c, int64_t mp);
// v <- -v;  out_i = alpha_i^2 - iK_ii (one problem / problem z of a batch)
void launch_negate(hipStream_t s, double* v, int64_t n);
void launch_qdiag(hipStream_t s, const double* iK, int64_t ld, const double* alpha, double* out, int64_t n);
void launch_qdiag_batched(hipStream_t s, int batch, const double* iK, int64_t ld, const double* alpha, double* out, int64_t n,
                          int64_t sMat, int64_t sVec, int64_t sOut);

// T evaluations one at a time (beyond the lockstep sizes): row(t, mu_t) with the mean of evaluation t as n values
template <class F>
int one_at_a_time(gpmi_ctx* c, int64_t T, const double* mus, const double* mu_const, F&& row) {
  std::vector<double> mu_row(mus ? 0 : (size_t)c->n);
  for (int64_t t = 0; t < T; ++t) {
    if (!mus) std::fill(mu_row.begin(), mu_row.end(), mu_const[t]);
    if (int rc = row(t, mus ? mus + t * c->n : mu_row.data())) return rc;
  }
  return GPMI_OK;
}

// ---- api_lockstep.hip: the lockstep batches (np <= 4096; every launch carries a chunk of problems in blockIdx.z) ----
bool batch_split_enabled();  // GPMI_BATCH_SPLIT=0: a chunk of gpmi_lml_batch / gpmi_predict_batch on one stream (A/B)

// The per-problem parameters of a batch on the host: single kernels (k) or sums (sum, GPMI_KERNEL_SUM), whichever is
// set.  On the device they live in bParams / bSum, at the chunk's offset.
struct BatchParams {
  int kernel;
  const KParams* k;
  const CovParams* sum;
  BatchParams(int kern, const KParams* kp, const CovParams* sp) : kernel(kern), k(sp ? nullptr : kp), sum(sp) {}
  BatchParams(int kern, const std::vector<KParams>& ps, const std::vector<CovParams>& sps)  // (of make_batch_params)
      : BatchParams(kern, ps.data(), sps.empty() ? nullptr : sps.data()) {}
  size_t bytes_each() const { return sum ? sizeof(CovParams) : sizeof(KParams); }
  const void* host(int64_t t) const { return sum ? static_cast<const void*>(sum + t) : static_cast<const void*>(k + t); }
  void* device(const gpmi_ctx* c, int off) const {
    return sum ? static_cast<void*>(c->bSum + off) : static_cast<void*>(c->bParams + off);
  }
};

// B problems of the lockstep workspace from problem `off` on, on one stream: off = 0 for the gradient batches, B1 for the
// second half-batch of gpmi_lml_batch / gpmi_predict_batch, slot * (bcap / 2) for the asynchronous slots.
struct Chunk {
  gpmi_ctx* c;
  hipStream_t stream;
  int off, B;
  bool mu_rows;  // Mu holds n prior means per problem (else one constant)
  BatchShape bs;
  double *A, *Inv, *Vec, *Mu, *B2, *red;  // B2: with the gradient workspace (ensure_batch_grad_ws)
  int* info;
  Chunk(gpmi_ctx* ctx, hipStream_t s, int first, int count, bool mean_rows);
  // the four work vectors of every problem (bs.sVec apart)
  double* v() const { return Vec; }                  // L^-1 (y - mu)
  double* alpha() const { return Vec + c->np; }      // K^-1 (y - mu)
  double* resid() const { return Vec + 2 * c->np; }  // y - mu: spent after the forward sweep
  double* slot3() const { return Vec + 3 * c->np; }
  int clear_info() const;
  // A <- B2 B2^T, lower tiles (kskip: launch_gemm)
  void syrk(int kskip) const;
};

// mixture batches (ChangePoint): K_z = sum_m D_zm K_zm D_zm + noise + extra_z from bMixP / bMixG / bMixExtra.  Those
// buffers, bMixH / bMixW and the mixture's slots of bGout are indexed from problem 0: a mixture chunk has off == 0.
struct MixBatch {
  int nk;
  const int* kernels;
  const int* n_thetas;
  int nrow;  // row sums per sub-kernel: 1 with the sub-kernel's own window weights, 2 with the caller's (hw)
  int tot_nt = 0, max_nt = 0;
  MixBatch(int n, const int* kern, const int* nts, bool hw) : nk(n), kernels(kern), n_thetas(nts), nrow(hw ? 2 : 1) {
    for (int m = 0; m < nk; ++m) {
      tot_nt += n_thetas[m];
      max_nt = n_thetas[m] > max_nt ? n_thetas[m] : max_nt;
    }
  }
  int W() const { return max_nt + 1; }  // values per sub-kernel and problem from the contraction
  int64_t sG(const gpmi_ctx* c) const { return (int64_t)GPMI_MAX_MIX * c->np; }         // between the problems' weight sets
  int64_t sW(const gpmi_ctx* c) const { return (int64_t)nrow * GPMI_MAX_MIX * c->np; }  // ... row-sum (weight) sets
};

// what fills A before the factorisation: the batch's single / sum kernels with the data's noise or - `noise` - with
// per-problem noise vectors (np apart), or the mixture
struct ChunkBuild {
  const BatchParams* p;
  const double* noise;
  const MixBatch* mix;
  static ChunkBuild kernels(const BatchParams& bp, const double* noise_rows = nullptr) { return {&bp, noise_rows, nullptr}; }
  static ChunkBuild mixture(const MixBatch& mx) { return {nullptr, nullptr, &mx}; }  // (chunks at problem 0 only)
};

// The stages every lockstep entry point shares, behind its uploads: [clear info], build, potrf_lower_batched, residual,
// forward sweep, [lml_reduce], [backward sweep -> alpha()], [L^-T -> B2].  The bracketed ones as `steps` says.
enum : unsigned { LS_CLEAR_INFO = 1, LS_REDUCE = 2, LS_BACKWARD = 4, LS_INVERSE = 8 };
int lockstep_stages(const Chunk& k, const ChunkBuild& b, unsigned steps);
void launch_kbuild_cross_batched(const Chunk& k, const BatchParams& p, const double* U, int64_t mu, int64_t mp, double* out,
                                 int64_t stride);
void launch_lml_grad_batched(const Chunk& k, const BatchParams& p, int n_theta, const double* u, const double* v, int64_t sV);
// params + means of chunk rows [t0, t0 + k.B) through the pinned staging (gradient batches)
int stage_batch_inputs(RowStage& stage, const Chunk& k, const BatchParams& p, int64_t t0, const double* mus,
                       const double* mu_const);
// the four leave-one-out vectors of every problem in bLoo (sLoo = 4 np apart)
struct LooVectors {
  double *diag, *c1, *sc2, *p;  // diag K^-1, c1, sqrt c2 - later diag M -, p = K^-1 c1
  int64_t sLoo;
  explicit LooVectors(const gpmi_ctx* c) : diag(c->bLoo), c1(c->bLoo + c->np), sc2(c->bLoo + 2 * c->np), p(c->bLoo + 3 * c->np), sLoo(4 * c->np) {}
};
// behind lockstep_stages(.., LS_BACKWARD | LS_INVERSE): diag K^-1, K^-1 in full, the leave-one-out vectors, p, and
// M = K^-1 diag(c2) K^-1 into A (lower tiles; both triangles with mirror_m); diag M where sc2 was if want_mdiag
void loo_middle(const Chunk& k, const LooVectors& lv, bool want_mdiag, bool mirror_m);
int ensure_batch_mix_ws(gpmi_ctx* c);
int make_mix_batch_params(gpmi_ctx* c, const MixBatch& mx, int64_t T, const double* thetas, std::vector<KParams>& ps);
int stage_mix_inputs(RowStage& stage, const Chunk& k, const MixBatch& mx, int64_t t0, int64_t T, const std::vector<KParams>& ps,
                     const double* g_host, const double* hw_host, const double* extra, const double* mus,
                     const double* mu_const);
// per sub-kernel, on Q in A (both triangles): the weight-scaled contraction into bGout and the window row sums into
// bMixH; p == nullptr: the likelihood form (u = v = g_m o alpha), else u = g_m o p, v = g_m o alpha
void mix_sub_kernel_terms(const Chunk& k, const MixBatch& mx, const double* p, int64_t sP);
// grad_thetas row of problem b of the chunk from h_bGout, times `factor`
void unpack_mix_gradient(const gpmi_ctx* c, const MixBatch& mx, int b, double factor, double* out);

// ---- api_single.hip: one evaluation on one lane (any size): what the single-evaluation entry points share ----
// api_dense.hip: the caller's matrix into L.A, and the dense twin of enqueue_factor_and_forward (no early work, no pair
// quiesce, no split build)
int upload_dense_matrix(gpmi_ctx* c, Lane& L, const double* K_host);
int enqueue_dense_factor_and_forward(gpmi_ctx* c, Lane& L, const double* mu_dev, int slot);

// host times of gpmi_fit's GPMI_DEBUG_TIMING line
struct LaneTimes {
  std::chrono::steady_clock::time_point start, forward, enqueued, done;
};

// One lane as an entry point sees it, the counterpart of Chunk: lane 0 holds the fit (its alpha is the handle's), lane 1
// every other single evaluation.  The lane is named by its index: lane_stages creates it when it is not there yet.
struct LaneEval {
  gpmi_ctx* c;
  int lane;
  LaneTimes* times = nullptr;
  LaneEval(gpmi_ctx* ctx, int index) : c(ctx), lane(index) {}
  Lane& L() const { return c->lanes[(size_t)lane]; }
  hipStream_t stream() const { return L().stream; }
  // the four work vectors
  double* v() const { return L().vec; }                                          // L^-1 (y - mu)
  double* alpha() const { return lane == 0 ? c->alpha : L().vec + c->np; }       // K^-1 (y - mu)
  double* resid() const { return L().vec + 2 * c->np; }                          // y - mu: spent after the forward sweep
  double* slot2() const { return resid(); }                                      // ... then diag K^-1, or g_m o alpha
  double* mu() const { return L().vec + 3 * c->np; }
  // the four leave-one-out vectors in front of the contraction's partial sums (LN_LOO)
  double* loo_diag() const { return L().gws; }
  double* loo_c1() const { return L().gws + c->np; }
  double* loo_sc2() const { return L().gws + 2 * c->np; }
  double* loo_p() const { return L().gws + 3 * c->np; }
  double* partial(bool behind_loo) const { return L().gws + (behind_loo ? 4 * c->np : 0); }
  // the contraction's results: n_theta + 1 values (n_theta <= GPMI_MAX_SUM (GPMI_MAX_D + 2)), on the host after lane_collect
  double* gout() const { return L().red + 16; }
  const double* h_gout() const { return L().h_red + 16; }
};

// what fills L.A before the factorisation
struct LaneBuild {
  const CovParams* p;
  const MixEval* mix;
  const double* dense;  // n x n on the host (a plugin covariance)
  static LaneBuild kernels(const CovParams& cp) { return {&cp, nullptr, nullptr}; }
  static LaneBuild mixture(const MixEval& mx) { return {nullptr, &mx, nullptr}; }
  static LaneBuild from_host(const double* K_host) { return {nullptr, nullptr, K_host}; }
};

// The stages every single-evaluation entry point shares: mu upload, build, factorisation, forward sweep and reduction
// (lane_forward); then [backward sweep -> alpha()], [L^-T -> B2], [K^-1 = B2 B2^T, lower tiles of A], [mirror]
// (lane_solves), the bracketed ones as `steps` says.  LN_FIT_SCHEDULE: gpmi_fit's - the inverse blocks of the predict
// built beside the sweeps.  LN_LOO: room for the leave-one-out vectors.  n_theta >= 0: room for the contraction's partial
// sums.  The lane, its second matrix and L.gws are allocated here as the steps need them (lane_prepare).
enum : unsigned { LN_BACKWARD = 1, LN_INVERSE = 2, LN_SYRK = 4, LN_MIRROR = 8, LN_LOO = 16, LN_FIT_SCHEDULE = 32 };
int lane_prepare(const LaneEval& ev, unsigned steps, int n_theta);
int lane_forward(const LaneEval& ev, const LaneBuild& b, unsigned steps, const double* mu_host, int n_theta = -1);
int lane_solves(const LaneEval& ev, unsigned steps);
inline int lane_stages(const LaneEval& ev, const LaneBuild& b, unsigned steps, const double* mu_host, int n_theta = -1) {
  if (int rc = lane_forward(ev, b, steps, mu_host, n_theta)) return rc;
  return lane_solves(ev, steps);
}
// behind lane_stages(.., LN_BACKWARD | LN_INVERSE | LN_LOO): diag K^-1; with want_p K^-1 in full, the leave-one-out
// vectors and p = K^-1 c1; with want_M also M = K^-1 diag(c2) K^-1 into A (lower tiles; both triangles with mirror_M)
void lane_loo_middle(const LaneEval& ev, bool want_p, bool want_M, bool mirror_M);

// n values of a device vector for the caller
struct LaneVec {
  double* host;
  const double* dev;
};
// The end of an evaluation: copies of red[0..1] (if `what` asks for a value), info, n_gout values of gout() and the
// vectors whose host pointer is not null; the sync; the info check.  *value: sum ln L_ii (LC_LOGDET; value may be null),
// -1/2 v.v - sum ln L_ii as it is (LC_LML_RAW), or with -1e50 for a matrix that did not factorise (LC_LML:
// regression.py:539-542); what = 0: none.
enum : unsigned { LC_LOGDET = 1, LC_LML_RAW = 2, LC_LML = 4 };
int lane_collect(const LaneEval& ev, unsigned what, int n_gout, std::initializer_list<LaneVec> vecs, double* value, int* info);
// alpha and diag K^-1 of one evaluation (gpmi_loo_terms, gpmi_loo_terms_mix): lane_stages, the row norms of L^-T, lane_collect
int lane_loo_terms(const LaneEval& ev, const LaneBuild& b, const double* mu_host, double* alpha_out, double* ikdiag, int* info);

// ---- the fitted lane's queries ----
// The 2048-row chunk loop of the predicts: fill(m0, mc, mp) leaves the chunk's cross-covariance in c->Q; the row dots
// with alpha go to mu_out, sumsq_base - |L^-1 k|^2 to ss_out (each if not null).
template <class Fill>
int predict_rows(gpmi_ctx* c, int64_t m, Fill&& fill, double sumsq_base, double* mu_out, double* ss_out) {
  Lane& L = c->lanes[0];
  hipStream_t s = L.stream;
  const int64_t chunk = 2048;
  for (int64_t m0 = 0; m0 < m; m0 += chunk) {
    const int64_t mc = (m - m0 < chunk) ? m - m0 : chunk;
    const int64_t mp = round_up(mc, GPMI_NB);
    if (int rc = ensure_query_ws(c, mp)) return rc;
    if (int rc = fill(m0, mc, mp)) return rc;
    double* mu_dev = c->pvec;
    double* ss_dev = c->pvec + mp;
    if (mu_out) launch_rows_dot(s, c->Q, c->ld, mp, c->np, c->alpha, mu_dev);
    if (ss_out) {
      if (int rc = ensure_inv2(c, L, s)) return rc;
      trsm_rows_forward(c, s, L.A, c->np, c->ld, L.inv2, c->Q, mp, false, c->Q2, nullptr);
      launch_rows_sumsq(s, c->Q2, c->ld, mp, c->np, sumsq_base, ss_dev);
    }
    HIPCHK(c, hipGetLastError());
    if (mu_out) HIPCHK(c, hipMemcpyAsync(mu_out + m0, mu_dev, sizeof(double) * mc, hipMemcpyDeviceToHost, s));
    if (ss_out) HIPCHK(c, hipMemcpyAsync(ss_out + m0, ss_dev, sizeof(double) * mc, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return GPMI_OK;
}

// Posterior mean and covariance at m points (mp padded): fill_cross() leaves the cross-covariance in c->Q; its row dots
// with alpha go to c->pvec (and to mu_out on the host, if not null); with Sigma != nullptr: Q2 = Q L^-T, fill_qq() leaves
// K_qq in Sigma (leading dimension ldq), Sigma <- Sigma - Q2 Q2^T.  Enqueued on lane 0's stream: the caller synchronises.
template <class Cross, class Qq>
int posterior_sigma(gpmi_ctx* c, Cross&& fill_cross, Qq&& fill_qq, int64_t m, int64_t mp, double* mu_out, double* Sigma,
                    int64_t ldq) {
  Lane& L = c->lanes[0];
  hipStream_t s = L.stream;
  if (int rc = fill_cross()) return rc;
  launch_rows_dot(s, c->Q, c->ld, mp, c->np, c->alpha, c->pvec);
  if (mu_out) HIPCHK(c, hipMemcpyAsync(mu_out, c->pvec, sizeof(double) * m, hipMemcpyDeviceToHost, s));
  if (Sigma) {
    if (int rc = ensure_inv2(c, L, s)) return rc;
    trsm_rows_forward(c, s, L.A, c->np, c->ld, L.inv2, c->Q, mp, false, c->Q2, nullptr);
    fill_qq();
    launch_gemm_nt(s, TILES_RECT, OP_SUB, Sigma, ldq, c->Q2, c->ld, c->Q2, c->ld, (int)(mp / GPMI_NB), (int)(mp / GPMI_NB),
                   (int)c->np);
  }
  HIPCHK(c, hipGetLastError());
  return GPMI_OK;
}
// posterior_sigma with the fitted kernel (or sum) at the m points pts of the host (gpmi_posterior, gpmi_posterior_draws)
int kernel_posterior_sigma(gpmi_ctx* c, const double* pts, int64_t m, int64_t mp, double* mu_out, double* Sigma, int64_t ldq);

// ---- draws.hip: what gpmi_posterior_draws, gpmi_mvn_draws and gpmi_sgp_posterior_draws share ----
int draws_check_args(gpmi_ctx* c, int64_t m, double jitter_rel, int64_t n_draws, int64_t first_draw, const double* draws);
// From Sigma (mp x ld on the device, lower triangle valid in the first m rows and columns; factorised in place) and mu
// (m, device) to the draws on the host, on the stream of `lane`, whose matrices are not touched
int draws_tail(gpmi_ctx* c, Lane& lane, double* A, int64_t ld, int64_t m, int64_t mp, const double* mu_dev, double jitter_rel,
               int64_t n_draws, const double* z_host, int64_t seed, int64_t first_draw, double* draws_host, double* eps_host,
               int* info);
