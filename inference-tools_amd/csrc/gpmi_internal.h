// Internal declarations shared by the HIP translation units of libgpmi.
// Public C-ABI: include/gpmi.h.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "gpmi.h"

constexpr int GPMI_NB = 128;     // tile / inner block size: every device matrix dimension is a multiple
constexpr int GPMI_MAX_D = 64;   // max spatial dimensions handled by the covariance kernels
constexpr int GPMI_INFO_FLOW_TIMEOUT = -6;  // `info` of a factorisation whose tile-task kernel gave up polling (api.hip: INFOCHK)
constexpr int GPMI_NPAIRS = 1;   // CU-masked stream pairs of the look-ahead (32 | 224 CUs)

typedef double d2_t __attribute__((ext_vector_type(2)));
typedef double d4_t __attribute__((ext_vector_type(4)));

static inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Hyper-parameters of one covariance evaluation, passed by value as a kernel argument.  Its size and the offsets of its
// fields are fixed (544 bytes: the lockstep staging, the sparse model's schedule and its documented bytes per problem count
// on them), so the Periodic kernel's own parameters live in fields the other kernels leave unused: the periodic
// dimensions as a bit mask in the place of RQ's kappa, and 1 / p_j of the j-th periodic dimension (ascending) in
// inv_l2[d + j] - which is why that kernel asks for d + n_per <= GPMI_MAX_D.
struct KParams {
  int kernel;                 // GPMI_KERNEL_SE / _RQ / _M32 / _M52 / _PER
  int d;                      // spatial dimensions
  double a2;                  // exp(theta0)^2
  union {
    double kappa;                 // RQ: exp(theta1)
    unsigned long long per_mask;  // Periodic: bit k set - dimension k is periodic
  };
  double extra_diag;          // WhiteNoise variance added to the diagonal
  double inv_l2[GPMI_MAX_D];  // 1 / l_k^2; Periodic: behind the d of them, 1 / p_j
};
static_assert(sizeof(KParams) == 32 + 8 * GPMI_MAX_D, "KParams keeps its layout");

// Whether dimension k of a Periodic kernel is one of its periodic dimensions, and then *ip = 1 / p of it (which may be 0:
// a period that overflowed).  *cursor counts the periodic dimensions met as k ascends (start it at 0): one bit test per
// dimension, everything uniform over the workgroup.
__host__ __device__ inline bool periodic_dim(const KParams& p, int k, int* cursor, double* ip) {
  if (!((p.per_mask >> k) & 1ull)) return false;
  *ip = p.inv_l2[p.d + (*cursor)++];
  return true;
}
// the same for one dimension on its own (the predictive-gradient kernels: one dimension per row or per pass)
__host__ __device__ inline bool periodic_dim(const KParams& p, int k, double* ip) {
  if (!((p.per_mask >> k) & 1ull)) return false;
  *ip = p.inv_l2[p.d + __builtin_popcountll(p.per_mask & ((1ull << k) - 1ull))];
  return true;
}

// The stationary kernels one KParams can describe, and the number of parameters each has in front of its length scales
// (ln a; RQ: ln a, ln kappa).  One explicit decision per id: "not SE" does not mean RQ.  -1: not such a kernel.
__host__ __device__ inline int kernel_theta_offset(int kernel) {
  switch (kernel) {
    case GPMI_KERNEL_SE: return 1;
    case GPMI_KERNEL_RQ: return 2;
    case GPMI_KERNEL_M32: return 1;
    case GPMI_KERNEL_M52: return 1;
    default: return -1;
  }
}
__host__ __device__ inline bool kernel_is_stationary(int kernel) { return kernel_theta_offset(kernel) > 0; }
__host__ __device__ inline bool kernel_is_matern(int kernel) {
  return kernel == GPMI_KERNEL_M32 || kernel == GPMI_KERNEL_M52;
}
// The kernel id as a compile-time constant: f(K) with decltype(K)::value the id, for the kernels that take it as a
// template parameter.  false (f not called): not a stationary kernel.
template <class F>
inline bool with_stationary_kernel(int kernel, F&& f) {
  switch (kernel) {
    case GPMI_KERNEL_SE: f(std::integral_constant<int, GPMI_KERNEL_SE>()); return true;
    case GPMI_KERNEL_RQ: f(std::integral_constant<int, GPMI_KERNEL_RQ>()); return true;
    case GPMI_KERNEL_M32: f(std::integral_constant<int, GPMI_KERNEL_M32>()); return true;
    case GPMI_KERNEL_M52: f(std::integral_constant<int, GPMI_KERNEL_M52>()); return true;
    default: return false;
  }
}

// A covariance evaluation the entry points hold: one stationary or Periodic kernel (the KParams base, nk = 0), or a sum of nk = 2..4 of
// them (GPMI_KERNEL_SUM, gpmi_set_sum).  For a sum the base carries kernel = GPMI_KERNEL_SUM, d, a2 = sum_m a_m^2 (the
// prior variance of a query point, regression.py:210) and the WhiteNoise variance; comp[m] are the components' own
// parameters (extra_diag 0).  The launchers of kbuild.hip / grad.hip have CovParams overloads, which launch the fused
// sum kernels for GPMI_KERNEL_SUM, and KParams forms, which take one stationary kernel and assert so (a sum copied into a
// KParams would lose its components).  KParams itself keeps its layout: it is the kernarg of every single-kernel launch.
constexpr int GPMI_MAX_SUM = 4;
struct CovParams : KParams {
  int nk = 0;
  KParams comp[GPMI_MAX_SUM] = {};
  CovParams() : KParams{} {}
  explicit CovParams(const KParams& k) : KParams(k) {}
};

// a kernel argument: HIP documents 4 KB as the limit of a launch's arguments
static_assert(sizeof(CovParams) <= 4096, "CovParams is passed by value to the sum kernels");
// The kinds a KParams can describe on the builders, the gradient contraction and the lockstep entry points: the
// stationary kernels and GPMI_KERNEL_PER.  (kernel_is_stationary stays the test of the sparse model, the selection and the
// Hessian, which do not take the Periodic kernel.)
__host__ __device__ inline bool kernel_is_single(int kernel) { return kernel_is_stationary(kernel) || kernel == GPMI_KERNEL_PER; }

struct gpmi_ctx;

// ---- ownership of device and pinned host memory ------------------------------------------------------------------
// Every allocation of the library passes through BufMem (the only place that calls the HIP allocator: plain hipMalloc /
// hipFree - callers rely on hipFree waiting for the device before it releases -, no pool, no stream-ordered allocator),
// which keeps the process-wide totals gpmi_live_bytes reports.
struct BufMem {
  static inline std::atomic<int64_t> live[2];  // bytes held now: [0] device, [1] pinned host
  // *p <- `bytes` of device memory, or of pinned host memory with the hipHostMalloc `flags`.  On failure *p is null, the
  // text goes to c->err (c may be null) and the result is GPMI_ERR_NOMEM / GPMI_ERR_HIP.
  static int get(gpmi_ctx* c, void** p, size_t bytes, bool pinned, unsigned flags);
  static void give(void* p, size_t bytes, bool pinned) {
    if (!p) return;
    (void)(pinned ? hipHostFree(p) : hipFree(p));
    live[pinned ? 1 : 0] -= (int64_t)bytes;
  }
};

// Typed, move-only owner of `capacity()` elements of device memory (PINNED: of pinned host memory).  Converts to T*, so
// it is used where the pointer was.  A failed allocation leaves it empty: null pointer, capacity 0.
template <class T, bool PINNED = false>
class DevBuf {
  T* p_ = nullptr;
  int64_t cap_ = 0;

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {  // releases what it held, at once
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p_; }
  T* get() const { return p_; }  // (where no conversion applies: reinterpret_cast)
  int64_t capacity() const { return cap_; }
  void release() {
    BufMem::give(p_, sizeof(T) * (size_t)cap_, PINNED);
    p_ = nullptr;
    cap_ = 0;
  }
  // `count` elements, contents undefined; what the buffer held before is freed first.  flags: hipHostMalloc's (PINNED)
  int alloc(gpmi_ctx* c, int64_t count, unsigned flags = 0) {
    release();
    if (int rc = BufMem::get(c, reinterpret_cast<void**>(&p_), sizeof(T) * (size_t)count, PINNED, flags)) return rc;
    cap_ = count;
    return GPMI_OK;
  }
  // alloc, then zeros that have ARRIVED: filled and waited for on the null stream (api_internal.h: ZERO_SYNC)
  int alloc_zeroed(gpmi_ctx* c, int64_t count);
  // at least `count` elements: nothing if it is large enough, else freed and allocated anew (contents lost)
  int reserve(gpmi_ctx* c, int64_t count, unsigned flags = 0) { return cap_ >= count ? GPMI_OK : alloc(c, count, flags); }
};
template <class T>
using PinBuf = DevBuf<T, true>;

struct ProfSlot {
  hipEvent_t e0, e1;
  int klass;
  double flops, bytes;
};

// The memory of a lane, as bases of Lane so that each group is released by assigning an empty one (api.hip: lane_free,
// potrf_flow.hip: potrf_flow_free) at its place in the teardown order.
struct LaneBufs {
  DevBuf<double> A;         // np x ld scratch (K then L)
  DevBuf<double> invD;      // (np/128) x 128 x 128 inverses of the diagonal blocks
  DevBuf<double> B2;        // second np x ld matrix (L^-T for the gradient / LOO paths), allocated lazily
  // inverses of the 512 x 512 diagonal blocks of L (many-right-hand-side solves), built lazily from invD
  DevBuf<double> inv2;      // ceil(nt / 4) x 512 x 512
  DevBuf<double> inv2_t;    // scratch: ceil(nt / 4) x 256 x 256
  DevBuf<double> gws;       // gradient partial sums
  DevBuf<double> vec;       // 4 x np work vectors
  DevBuf<double> red;       // small reduction outputs (device)
  DevBuf<int> info;         // device info word
  PinBuf<double> h_red;     // pinned host mirror of red
  PinBuf<int> h_info;       // pinned host mirror of info
  // fused panel column of the stream-ordered chain (potrf_panel.hip): GPMI_PANEL_FL_INTS ints, zeroed once at the
  // allocation - the row counters are monotone
  DevBuf<int> panel_flags;
};
// flag-ordered factorisation of the chain-bound part (potrf_flow.hip): task lists of a tail of flow_m tile rows
struct LaneFlowBufs {
  DevBuf<char> flow_tasks;  // FlowTask records
  DevBuf<int> flow_off;
  DevBuf<int> flow_flags;
};

// One independent evaluation lane: a stream with its own n x n scratch matrix and vectors.
struct Lane : LaneBufs, LaneFlowBufs {
  hipStream_t stream = nullptr;    // full-chip stream: covariance build, solves, small factorisations
  bool owns_stream = true;         // false (lanes 2..): the stream is lane 0's or lane 1's (api.hip: lane_streams)
  // look-ahead pairs (CU-masked, disjoint; lanes 0 and 1 only, created with the lane): pair k factors the next panel on
  // gpmi_ctx::pair_cus[k] CUs (sp) while the trailing update runs on all the others (su)
  hipStream_t sp[GPMI_NPAIRS] = {nullptr};
  hipStream_t su[GPMI_NPAIRS] = {nullptr};
  bool owns_pair = true;           // false (lane 1): the pair is lane 0's (api.hip: lane_alloc)
  // Work of the alpha phase that does not depend on the factor (the residual y - mu, the sentinel fills of the two sweeps'
  // outputs), enqueued on the lane's stream by the factorisation at the point where that stream has handed the work to the
  // masked pair and would otherwise idle until the join (potrf_lower / potrf_flow_tail call lane_run_early; whoever set it
  // calls it again behind the factorisation, where it is a no-op unless no such point came up): ~15 us per fit off the
  // critical path (round 6)
  struct EarlyWork {
    bool pending = false;
    const double* y = nullptr;
    const double* mu = nullptr;
    double mu_const = 0.0;
    double* r = nullptr;
    int64_t n = 0, np = 0;
    double* fill[2] = {nullptr, nullptr};
    double* ident = nullptr;  // np x np matrix (leading dimension ident_ld) to be set to the identity: the right-hand side
    int64_t ident_ld = 0;     // of the inverse factor the gradient paths compute next (enqueue_inverse_factor)
  } early;
  bool identity_ready = false;  // EarlyWork has written the identity into B2 for the inverse factor that follows
  bool pair_checked = false;       // potrf_pair_quiesce has run for the factorisation being enqueued (potrf.hip)
  hipEvent_t ev_la = nullptr, ev_panel = nullptr, ev_join = nullptr, ev_main = nullptr, ev_slice = nullptr;
  bool inv2_valid = false;  // inv2 holds the blocks of the factor in A
  // the task lists in LaneFlowBufs
  int flow_m = 0, flow_nwg = 0, flow_nlists = 0;
  int64_t flow_ntasks = 0;
  double flow_flops_update = 0.0, flow_flops_trsm = 0.0;
  unsigned panel_seq = 0;  // fused panel-column launches (panel_flags) the lane has enqueued so far
};
// Lane::panel_flags: the row-block counters of the inverse on lines of their own (32 r), the abort word
constexpr int GPMI_PANEL_FL_INVROW = 0, GPMI_PANEL_FL_ABORT = 256, GPMI_PANEL_FL_INTS = 288;

// device state of the linear-inversion entry points (gpmi_linv_*): m data values, model matrix A (m x n)
struct LinvState {
  int64_t m = 0, mp = 0, ldm = 0;
  DevBuf<double> A;     // mp x ld   model matrix, zero padded
  DevBuf<double> At;    // np x ldm  its transpose
  DevBuf<double> y;     // mp
  DevBuf<double> sig2;  // mp        y_err^2, 1 in the padding (keeps the padded J positive definite)
  DevBuf<double> zero;  // np        zeros (the prior covariance carries no data noise)
  DevBuf<double> K;     // np x ld   prior covariance (later A^T J^-1 A, K - X X^T)
  DevBuf<double> T;     // mp x ld   A K (later J^-1 A)
  DevBuf<double> J;     // mp x ldm  A K A^T + Sigma, then its factor L
  DevBuf<double> J2;    // mp x ldm  L^-T, then J^-1          (gradient only)
  DevBuf<double> Q;     // np x ldm  K A^T                    (posterior only)
  DevBuf<double> X;     // np x ldm  K A^T L^-T               (posterior only)
  DevBuf<double> invD;  // 128-wide inverse diagonal blocks of L
  DevBuf<double> inv2;  // 512-wide
  DevBuf<double> inv2_t;
  DevBuf<double> panel; // mp x 544 (in-place many-right-hand-side solve)
  DevBuf<double> vec;   // 8 x max(mp, np) work vectors
  DevBuf<double> gws;
};

struct KdeState;  // kde.hip
struct gpmi_sgp;  // sparse.hip

// The device memory of a handle in the groups that are released together, as bases of gpmi_ctx: a group is released by
// assigning an empty one (api.hip: free_data, free_batch_ws, ensure_*), which also zeroes the group's capacity.
// the data set (gpmi_set_data) and the fitted alpha
struct DataBufs {
  DevBuf<double> x;      // np x d (rows >= n are zero)
  DevBuf<double> y;      // np
  DevBuf<double> noise;  // np diagonal data variances (zero padded)
  DevBuf<double> ycov;   // n x n dense y covariance or empty
  DevBuf<double> alpha;  // np — fitted alpha
};
// prediction workspace, sized together for mq_cap query rows (ensure_query_ws)
struct QueryBufs {
  DevBuf<double> Q;     // mq_cap x ld
  DevBuf<double> Q2;    // second panel (spatial derivatives)
  DevBuf<double> pts;   // mq_cap x d
  DevBuf<double> pvec;  // vectors of length mq_cap * (2 + 2 d)
  int64_t mq_cap = 0;
};
// gradient batches, sized together for bgrad_cap problems of bgrad_ntheta parameters (ensure_batch_grad_ws)
struct BatchGradBufs {
  DevBuf<double> bB2;     // second matrix per problem (L^-T)
  DevBuf<double> bGws;    // partial sums of the fused contraction
  DevBuf<double> bGout;   // (n_theta + 1) results per problem
  PinBuf<double> h_bGout;
  int bgrad_cap = 0, bgrad_ntheta = 0;
};
// batched small-problem workspace (gpmi_lml_batch for np <= 4096): `bcap` matrices side by side (ensure_batch_ws), and
// what the batch entry points add per problem
struct BatchBufs : BatchGradBufs {
  int bcap = 0;
  DevBuf<double> bA, bInv, bVec, bRed, bMu;
  DevBuf<int> bInfo;
  DevBuf<KParams> bParams;
  DevBuf<CovParams> bSum;  // the per-problem parameters of a lockstep batch of sums (bcap of them)
  PinBuf<double> h_bRed;
  PinBuf<int> h_bInfo;
  DevBuf<double> bNoise;   // gpmi_lml_grad_batch_noise: one noise-variance vector per problem
  DevBuf<double> bQ;       // gpmi_predict_batch: per problem two panels of GPMI_PREDICT_PANEL x ld (K*, K* L^-T)
  DevBuf<double> bLoo;     // gpmi_loo_grad_batch: 4 vectors per problem (diag K^-1, c1, sqrt c2, p)
  // gpmi_lml_grad_batch_mix (ensure_batch_mix_ws, bMix_cap problems): per problem the window weights g_m and the row sums
  // h_m (GPMI_MAX_MIX x np each), the sub-kernels' parameters (GPMI_MAX_MIX arrays of bcap KParams) and the WhiteNoise
  // variances
  DevBuf<double> bMixG, bMixH;
  DevBuf<double> bMixW;    // the caller's row-sum weights (gpmi_*_grad_batch_mix: hw)
  DevBuf<KParams> bMixP;
  DevBuf<double> bMixExtra;
  int bMix_cap = 0;
};
// fitted mixture model (gpmi_fit_mix): the training-point weights g and the third query panel
struct MixBufs {
  int mix_nk = 0;
  DevBuf<double> mix_g;        // nk x np (row m: g_m; padding 1 for m = 0, 0 otherwise)
  DevBuf<double> mix_scratch;  // np x ld
  DevBuf<double> mix_zero;     // np zeros
  DevBuf<double> Q3;           // third query panel (mq_cap x ld at its allocation)
};

// many targets on one factorisation (api_multi.hip, gpmi_mt_*): mt_T targets stored as rows, mt_Tp = mt_T rounded up to
// the tile, zero in the padding; each buffer is allocated by the first call that needs it
struct MultiBufs {
  int64_t mt_T = 0, mt_Tp = 0, mt_ldt = 0;  // mt_ldt = mt_Tp + 32: the pitch of the arrays with one row per data point
  bool mt_fitted = false;   // mtA belongs to the factor in lane 0 (gpmi_mt_fit was the last fit and succeeded)
  DevBuf<double> mtR;       // mt_Tp x ld   residuals Y - m, one target per row
  DevBuf<double> mtA;       // mt_Tp x ld   A^T = R^T K^-1 of the fit
  DevBuf<double> mtW;       // mt_Tp x ld   V^T, then A^T of an evaluation on lane 1
  DevBuf<double> mtAn;      // np x mt_ldt  transposed copies: the upload, A / sqrt(T), A, A_it / (K^-1)_ii
  DevBuf<double> mtMean;    // 2048 x mt_ldt predictive means of a chunk of query points
  DevBuf<double> mtVec;     // mt_Tp + 8 + np: |V_t|^2 per target, their sum (at mt_Tp), sum_t A_it^2 per point (at mt_Tp + 8)
  DevBuf<double> mtZero;    // np zeros: u and v of the contraction
  PinBuf<double> h_mtVec;   // pinned mirror of mtVec
};

// gpmi_lml_hessian (api_hessian.hip): the derivative matrices D_i of a group of parameters, the products G_i = K^-1 D_i of
// that group (hGa) and - only when the parameters do not fit one group - of a second group (hGb), the vectors
// (D_i alpha, G_i alpha, the mean's features and K^-1 times them) and the partial sums of the contractions; each is
// allocated by the first call that needs it and grows as later calls ask
struct HessBufs {
  DevBuf<double> hD, hGa, hGb;  // g x np x ld each
  DevBuf<double> hVec;          // (2 (n_theta + 1) + 2 n_mean) x np
  DevBuf<double> hPart;         // partial sums of the pair traces and of the second-derivative contraction, then the sums
  PinBuf<double> h_hOut;        // pinned mirror of the sums
};

// generalised GP (api_generalised.hip, gpmi_ggp_*): the observations of a non-Gaussian likelihood and, per lane (0: the fit,
// 1: evaluations at other hyper-parameters), the latent covariance, the work vectors of Newton's iteration, the block
// partials of its sums and the record the host reads once per step; each lane's buffers are allocated by its first call
constexpr int GGP_NVEC = 18;  // work vectors per lane (api_generalised.hip: GgpVecs)
struct GgpBufs {
  int ggp_lik = -1;           // GPMI_GGP_*; -1: gpmi_ggp_set_observations has not been called for this data set
  double ggp_offset = 0.0;    // the constant prior mean m of f
  bool ggp_fitted = false;    // lane 0 holds the factor of B at the mode (gpmi_ggp_fit was the last fit and succeeded)
  DevBuf<double> ggY, ggAux, ggConst;  // np each: y, the per-point data of the likelihood, the f-independent part of log p
  DevBuf<double> ggZero;      // np zeros: the latent K carries no data noise
  DevBuf<double> ggK[2];      // np x ld   latent covariance K (both triangles, identity in the padding)
  DevBuf<double> ggVec[2];    // GGP_NVEC x np
  DevBuf<double> ggPart[2];   // ggp_part_doubles(np)
  DevBuf<double> ggRec[2];    // 8: sum log p, a^T (f - m), max |f - f_prev|, max |f|
  PinBuf<double> h_ggRec;     // pinned mirror of a record
  DevBuf<double> ggMean;      // 2048 predictive means of a chunk of query points
};

struct gpmi_ctx : DataBufs, QueryBufs, BatchBufs, MixBufs, MultiBufs, HessBufs, GgpBufs {
  int device = 0;
  int ncu = 256;      // compute units of the device
  int pair_cus[GPMI_NPAIRS] = {32};  // CUs of the panel stream of look-ahead pair k (the update stream has the rest)
  std::string err;
  // data
  int64_t n = 0, d = 0, np = 0, ld = 0;
  // fitted state lives in lanes[0]
  std::vector<Lane> lanes;
  bool fitted = false;
  bool lockstep_always = false;  // GPMI_OPT_LOCKSTEP_ALWAYS
  bool no_flow = false;          // GPMI_OPT_NO_FLOW
  int64_t reserve = 0;           // GPMI_OPT_RESERVE_POINTS: extra rows of padding at the next gpmi_set_data
  CovParams fit_params;
  int sum_nk = 0;                   // gpmi_set_sum: components of this handle's GPMI_KERNEL_SUM (0: none declared)
  int sum_kinds[GPMI_MAX_SUM] = {};
  int n_per = 0;                    // gpmi_set_periodic: periodic dimensions of this handle's GPMI_KERNEL_PER (0: none declared)
  int per_dim[GPMI_MAX_PERIODIC] = {};
  DevBuf<double> trsm_panel;  // rows x 544 scratch of the in-place many-right-hand-side solve
  PinBuf<char> h_stage;       // host staging of the lockstep chunks (RowStage)
  // asynchronous lockstep batches (gpmi_lml_batch_submit / _wait): two slots = the two halves of the workspace, on the
  // streams of lanes 1 and 2; evaluations pending per slot (0: free), pinned staging of their inputs
  int bpend[2] = {0, 0};
  PinBuf<char> h_bStage[2];
  LinvState linv;
  KParams mix_p[4];  // gpmi_fit_mix: the sub-kernels' parameters (MixBufs::mix_nk of them)
  // RCCL result gather (comm.hip)
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  hipStream_t comm_stream = nullptr;
  DevBuf<double> comm_buf;
  hipStream_t dev_masked = nullptr;  // tools: CU-masked stream of the device-pointer entry points (GPMI_DEV_CUS)
  std::vector<DevBuf<char>> dev_allocs;  // tools: what gpmi_dev_alloc has handed out and gpmi_dev_free not taken back
  KdeState* kde = nullptr;  // kde.hip: stream, workspaces and live objects of the gpmi_kde_* entry points
  // sparse.hip: the live objects of the gpmi_sgp_* entry points and the stream they share (created with the first one)
  std::vector<gpmi_sgp*> sgp_live;
  hipStream_t sgp_stream = nullptr;
  // instrumentation
  hipEvent_t t0 = nullptr, t1 = nullptr;
  unsigned prof_mask = 0;
  // device-stamped launches (trailing-update class): {min start, max end} per launch
  DevBuf<unsigned long long> stamp_pool;
  std::vector<double> stamp_flops, stamp_bytes;
  std::vector<int> stamp_class;
  std::vector<ProfSlot> prof_slots;
  size_t prof_used = 0;
  double prof_clock_cycles = 0.0, prof_clock_ticks = 0.0;  // shader cycles / 10 ns ticks over stamped workgroups
  double prof_ms[GPMI_PROF_NCLASS] = {};
  double prof_flops[GPMI_PROF_NCLASS] = {};
  double prof_bytes[GPMI_PROF_NCLASS] = {};
  int64_t prof_launches[GPMI_PROF_NCLASS] = {};
};

inline int BufMem::get(gpmi_ctx* c, void** p, size_t bytes, bool pinned, unsigned flags) {
  const hipError_t e = pinned ? hipHostMalloc(p, bytes, flags) : hipMalloc(p, bytes);
  if (e == hipSuccess) {
    live[pinned ? 1 : 0] += (int64_t)bytes;
    return GPMI_OK;
  }
  *p = nullptr;
  if (c) c->err = std::string(pinned ? "hipHostMalloc" : "hipMalloc") + " of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? GPMI_ERR_NOMEM : GPMI_ERR_HIP;
}
template <class T, bool PINNED>
int DevBuf<T, PINNED>::alloc_zeroed(gpmi_ctx* c, int64_t count) {
  if (int rc = alloc(c, count)) return rc;
  hipError_t e = hipMemset(p_, 0, sizeof(T) * (size_t)count);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) return GPMI_OK;
  if (c) c->err = std::string("zeroing a new buffer: ") + hipGetErrorString(e);
  return GPMI_ERR_HIP;
}

// kde.hip: destroy the handle's density objects and their stream / workspaces (gpmi_destroy)
void kde_release_all(gpmi_ctx* c);
// sparse.hip: the same for the inducing-point models (gpmi_destroy)
void sgp_release_all(gpmi_ctx* c);

// instrumentation helpers (api.hip)
constexpr int GPMI_STAMP_SLOTS = 16384;
constexpr int GPMI_STAMP_WORDS = 24;  // per launch: 8 start words + 8 end words (one per XCD) + 8 clock words, see gemm_f64.hip
// next stamp slot (GPMI_STAMP_WORDS words) for a trailing-update launch, or nullptr when that class is not profiled
unsigned long long* prof_stamp_slot(gpmi_ctx* c, double flops, double bytes, int klass = GPMI_PROF_SYRK);
struct ProfScope {
  gpmi_ctx* c;
  hipStream_t s;
  int64_t slot;  // index into gpmi_ctx::prof_slots (-1: not timed) - not a pointer: a scope opened inside this one may grow the vector
  ProfScope(gpmi_ctx* ctx, hipStream_t st, int klass, double flops, double bytes);
  ~ProfScope();
};

// ---- kernel launchers -------------------------------------------------------------
// kbuild.hip
// square covariance of the np x np padded problem (identity in the padding), lower tiles only if lower_only
void launch_kbuild_square(hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np,
                          const double* noise, double* A, int64_t ld, bool lower_only);
void launch_kbuild_square_part(hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np,
                               const double* noise, double* A, int64_t ld, int part, int split_cols);
// cross covariance U (mp x d, mu valid rows) vs V (np x d, n valid rows): out mp x ld, zeros in padding
void launch_kbuild_cross(hipStream_t s, const KParams& p, const double* U, int64_t mu, int64_t mp,
                         const double* V, int64_t n, int64_t np, double* out, int64_t ld);
// the same cross build of the Matern DERIVATIVE profile a^2 g (kmath.h: matern_profile) in the place of K = a^2 C: the
// rows the predictive-gradient kernels multiply by (predgrad.hip).  Matern kernels only.
void launch_kbuild_cross_dprofile(hipStream_t s, const KParams& p, const double* U, int64_t mu, int64_t mp,
                                  const double* V, int64_t n, int64_t np, double* out, int64_t ld);
void launch_add_full(hipStream_t s, double* A, int64_t ld, const double* Y, int64_t n);
// The same builders for a CovParams: the fused sum build when p.kernel == GPMI_KERNEL_SUM, else its base's build.  (The
// KParams forms take SE / RQ only: a sum is never passed as its base.)
void launch_kbuild_square(hipStream_t s, const CovParams& p, const double* x, int64_t n, int64_t np,
                          const double* noise, double* A, int64_t ld, bool lower_only);
void launch_kbuild_square_part(hipStream_t s, const CovParams& p, const double* x, int64_t n, int64_t np,
                               const double* noise, double* A, int64_t ld, int part, int split_cols);
void launch_kbuild_cross(hipStream_t s, const CovParams& p, const double* U, int64_t mu, int64_t mp,
                         const double* V, int64_t n, int64_t np, double* out, int64_t ld);
// lockstep batch of sums (pdev: batch CovParams of kind GPMI_KERNEL_SUM), the square lower tiles as
// launch_kbuild_square_batched
void launch_kbuild_square_batched(hipStream_t s, const CovParams* pdev, int batch, const double* x, int64_t n,
                                  int64_t np, const double* noise, double* A, int64_t ld, int64_t stride, int d);

// lockstep batch of cross covariances: problem z builds K*_z (mp x ld: the mu valid rows of U against the n valid rows of
// V, zeros in the padding) from pdev[z] into out + z * stride - element for element launch_kbuild_cross for that problem
void launch_kbuild_cross_batched(hipStream_t s, int kernel, const KParams* pdev, int batch, const double* U, int64_t mu,
                                 int64_t mp, const double* V, int64_t n, int64_t np, double* out, int64_t ld,
                                 int64_t stride, int d);
void launch_kbuild_cross_batched(hipStream_t s, const CovParams* pdev, int batch, const double* U, int64_t mu, int64_t mp,
                                 const double* V, int64_t n, int64_t np, double* out, int64_t ld, int64_t stride, int d);

// predict_batch.hip: the per-row results of a panel of gpmi_predict_batch and their mixture
// rows [m0, m0 + rows) of problems [t_first, t_first + batch): mean = dot + prior mean, var = |a_z^2 - sumsq|, NaN where
// info[z] != 0.  dot / sumsq: the panel's row sums at dot + z * sDot, sumsq + z * sSq (sumsq == nullptr: means only); a2 of
// problem z at params + z * pstride bytes (the KParams base of either parameter struct); mu_q (T x m) or mu_const (T), device
void launch_predict_store(hipStream_t s, int batch, int64_t t_first, int64_t m0, int64_t rows, int64_t m,
                          const double* dot, const double* sumsq, int64_t sDot, int64_t sSq, const void* params,
                          int64_t pstride, const int* info, const double* mu_q, const double* mu_const, double* mean_t,
                          double* var_t);
// mix_mean[q] = sum_g w[g] mean_t[idx[g]][q], mix_var[q] = sum_g w[g] (var_t[idx[g]][q] + (mean_t[idx[g]][q] - mix_mean[q])^2)
// over the G listed rows, each sum a pairwise tree in list order (var_t / mix_var == nullptr: the mean alone)
void launch_predict_mix(hipStream_t s, int64_t G, const int* idx, const double* w, int64_t m, const double* mean_t,
                        const double* var_t, double* mix_mean, double* mix_var);

// grad.hip: fused contraction 1/2 sum (alpha alpha^T - K^-1) o dK/dtheta_j with dK recomputed from x.
// out[0..n_theta) = gradient, out[n_theta] = sum_i (alpha_i^2 - K^-1_ii).  iK holds K^-1 (lower tiles).
int64_t grad_ws_doubles(int64_t np, int n_theta);
// general form: Q_ab = 1/2 (u_a v_b + u_b v_a) - iK_ab  (LML gradient: u = v = alpha)
void launch_lml_grad(hipStream_t s, const KParams& p, int n_theta, const double* x, int64_t n,
                     int64_t np, const double* iK, int64_t ld, const double* u, const double* v,
                     double* ws, double* out);
// (kernel: the kind of every pdev[z], which selects the instantiation)
void launch_lml_grad_batched(hipStream_t s, int kernel, const KParams* pdev, int batch, int n_theta, const double* x,
                             int64_t n, int64_t np, const double* iK, int64_t ld, int64_t sK, const double* u,
                             const double* v, int64_t sV, double* ws, double* out);
// the same for a CovParams (the fused contraction of a sum: partials [component 1, ..., component nk, trace]) and for a
// lockstep batch of sums
void launch_lml_grad(hipStream_t s, const CovParams& p, int n_theta, const double* x, int64_t n,
                     int64_t np, const double* iK, int64_t ld, const double* u, const double* v,
                     double* ws, double* out);
void launch_lml_grad_batched(hipStream_t s, const CovParams* pdev, int batch, int n_theta, const double* x, int64_t n,
                             int64_t np, const double* iK, int64_t ld, int64_t sK, const double* u, const double* v,
                             int64_t sV, double* ws, double* out, int d, bool has_periodic);
void launch_mirror_lower(hipStream_t s, double* A, int64_t ld, int64_t np, int batch = 1, int64_t sMat = 0);
// (batch > 1: problem z works on A / G + z sMat and on vectors sVec (sAlpha, sLoo) apart)
void launch_scale_columns(hipStream_t s, const double* A, const double* sc, double* G, int64_t ld,
                          int64_t np, int batch = 1, int64_t sMat = 0, int64_t sVec = 0);
void launch_loo_vectors(hipStream_t s, const double* alpha, const double* ikdiag, double* c1,
                        double* sc2, int64_t n, int64_t np, int batch = 1, int64_t sAlpha = 0, int64_t sLoo = 0);

// hessian.hip: the kernels of gpmi_lml_hessian.  Parameters are numbered as theta is laid out (ln a; RQ: ln kappa; ln l_1 ..
// ln l_d) with ln sigma of the WhiteNoise variance at n_theta.
// D[m] (np x ld, sMat apart, both triangles, zeros in the padding) = dK / d parameter (p0 + m), m < cnt
void launch_hess_dbuild(hipStream_t s, const KParams& p, int n_theta, int p0, int cnt, const double* x, int64_t n, int64_t np,
                        double* D, int64_t ld, int64_t sMat);
// part[((iA0 + i) PT + jB0 + j) (np / 64) + ta] = sum over the 64-row block ta of a and all b of GA[i][a][b] GB[j][b][a], for the
// pairs with iA0 + i <= jB0 + j; launch_hess_trace_sum: out[i PT + j] = their sum over ta in ascending order (i <= j)
void launch_hess_pair_trace(hipStream_t s, const double* GA, int iA0, int nA, const double* GB, int jB0, int nB, int64_t np,
                            int64_t ld, int64_t sMat, int PT, double* part);
void launch_hess_trace_sum(hipStream_t s, const double* part, int PT, int64_t np, double* out);
// out[i nv + j] = sum_a U[i][a] V[j][a] over np values (rows np apart), a fixed order; upper: only i <= j
void launch_hess_dots(hipStream_t s, const double* U, int nu, const double* V, int nv, int64_t np, bool upper, double* out);
// 1/2 sum_ab Q_ab of the second-derivative profiles over the lower 64 x 64 tiles of iK (off-diagonal elements twice),
// Q = alpha alpha^T - K^-1: hess_contract_entries(kernel, d) sums into out - S_km = a^2 g2 q_k q_m for k <= m row by row,
// then (RQ) the d mixed profiles with ln kappa and the second derivative by ln kappa.  ws: hess_contract_ws_doubles.
int hess_contract_entries(int kernel, int d);
int64_t hess_contract_ws_doubles(int64_t np, int kernel, int d);
int launch_hess_contract(gpmi_ctx* c, hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np, const double* iK,
                         int64_t ld, const double* alpha, double* ws, double* out);

// batch of independent equal-shape problems in one launch (blockIdx.z): strides in doubles
struct GemmBatch {
  int count = 1;
  int64_t sC = 0, sA = 0, sB = 0;
  // CUs the launch's stream may use (0: the whole chip): the choice of 32-row tiles ("while CUs are idle") scales with it
  int ncu_hint = 0;
  // B of a one-tile-column product with K = 128 is lower triangular (B[j][k] = 0 for k > j: the inverse of a diagonal
  // block): the kernel skips the zero part
  bool b_lower_tri = false;
  // lockstep launches whose values must not depend on how many problems share the launch: only tile shapes that sum in
  // the ring kernels' order (no 32-row register-staged tiles at K > 128, whose use depends on the batch size; round 6:
  // the inverse of a gradient batch of one differed from the same problem's inside a batch of six in the last bits)
  bool ring_order_only = false;
};
struct BatchShape {
  int count = 1;
  int64_t sMat = 0;   // between the np x ld matrices
  int64_t sInv = 0;   // between the invD arrays
  int64_t sVec = 0;   // between the work-vector sets
};

// mix.hip: pieces of the mixture covariance K = sum_m diag(g_m) K_m diag(g_m) (ChangePoint)
constexpr int GPMI_MAX_MIX = 4;
// (batch > 1: problem z of a lockstep batch works on matrices sD / sS / sA / sMat apart and on weight vectors sG apart)
void launch_scale_add(hipStream_t s, double* dst, int64_t ldd, const double* src, int64_t lds,
                      const double* gr, const double* gc, int64_t rows, int64_t cols, bool accumulate, int batch = 1,
                      int64_t sD = 0, int64_t sS = 0, int64_t sG = 0);
void launch_add_diag_vec(hipStream_t s, double* A, int64_t ld, const double* noise, double extra, int64_t n,
                         int batch = 1, int64_t sA = 0, const double* extras = nullptr);
void launch_vec_mul(hipStream_t s, const double* a, const double* b, double* out, int64_t n, int batch = 1,
                    int64_t sA = 0, int64_t sB = 0, int64_t sOut = 0);
// h_i = sum_j (1/2 (u_i alpha_j + alpha_i u_j) - iK_ij) Km_ij g_j  (iK, Km full n x n; u = nullptr: u = alpha, the LML form);
// pair != 0: the same pass also takes the weights at g + pair into h + pair
void launch_mix_rowsum(hipStream_t s, const double* iK, const double* Km, int64_t ld, const double* alpha,
                       const double* g, double* h, int64_t n, int batch = 1, int64_t sMat = 0, int64_t sAlpha = 0,
                       int64_t sG = 0, const double* u = nullptr, int64_t sU = 0, int64_t pair = 0);

// gemm_f64.hip  (all dims multiples of 128, k multiple of 16)
enum GemmTiles { TILES_RECT = 0, TILES_LOWER = 1 };
enum GemmOp { OP_SUB = 0, OP_ASSIGN = 1 };
// C(ntr*128 x ntc*128) op= A(rows x k) * B(cols x k)^T ; TILES_LOWER visits tiles ti >= tj only
void launch_gemm_nt(hipStream_t s, GemmTiles tiles, GemmOp op, double* C, int64_t ldc,
                    const double* A, int64_t lda, const double* B, int64_t ldb, int ntr, int ntc,
                    int k, unsigned long long* stamp = nullptr, const GemmBatch& bt = GemmBatch());

// balanced form of launch_gemm_nt for big launches (gemm_f64.hip): the first `nfull` = gemm_split_point(T, ncu, k)
// tiles run as 128 x 128 tiles, the tiles of the nearly empty last round as 64 x 64 tiles in a second launch;
// `stamp` times the first launch only.  nend >= 0: the product stops at logical tile `nend` - the tiles from there on
// are somebody else's (launch_gemm_nt_range on another stream)
int64_t gemm_split_point(int64_t T, int ncu, int k);
bool gemm_mixed_launches();  // GPMI_GEMM_MIXED: launch_gemm_nt_split puts the remainder's quarters into the launch of the full rounds
void launch_gemm_nt_split(hipStream_t s, GemmTiles tiles, GemmOp op, double* C, int64_t ldc, const double* A,
                          int64_t lda, const double* B, int64_t ldb, int ntr, int ntc, int k, int64_t nfull,
                          unsigned long long* stamp = nullptr, unsigned long long* stamp_rest = nullptr,
                          int64_t nend = -1);
void launch_gemm_nt_range(hipStream_t s, GemmTiles tiles, GemmOp op, double* C, int64_t ldc, const double* A,
                          int64_t lda, const double* B, int64_t ldb, int ntr, int ntc, int k, int64_t first,
                          int64_t count, unsigned long long* stamp = nullptr);

// general form: b_kmajor -> B is (k x cols) row-major; kskip = 1 (TILES_LOWER) -> contraction starts at
// the tile row's first column, kskip = 2 -> it ends with the tile column (B lower triangular)
void launch_gemm(hipStream_t s, GemmTiles tiles, GemmOp op, bool b_kmajor, int kskip, double* C,
                 int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb, int ntr,
                 int ntc, int k, unsigned long long* stamp = nullptr, const GemmBatch& bt = GemmBatch());

// potrf.hip
hipStream_t potrf_first_update_stream(gpmi_ctx* c, Lane& lane, int64_t np, bool allow_lookahead);
// waits for whatever an earlier (failed / foreign) call left on the lane's CU-masked pair; before the caller's own enqueues
void potrf_pair_quiesce(Lane& lane);
void launch_potrf_diag(hipStream_t s, double* Ablk, int64_t ld, double* invD, int* info, int col0,
                       unsigned long long* dbg = nullptr, const BatchShape& bs = BatchShape());
void launch_potrf_diag_fault(hipStream_t s, double* Ablk, int64_t ld, const BatchShape& bs = BatchShape());  // test hook
// batched, in-order factorisation of bs.count matrices (small problems: no look-ahead)
void potrf_lower_batched(gpmi_ctx* c, hipStream_t s, double* A, int64_t np, int64_t ld, double* invD,
                         int* info, const BatchShape& bs);
void launch_kbuild_square_batched(hipStream_t s, int kernel, const KParams* pdev, int batch, const double* x,
                                  int64_t n, int64_t np, const double* noise, double* A, int64_t ld,
                                  int64_t stride, int d, int64_t noise_stride = 0);
// blocked right-looking Cholesky, in place, lower; invD receives the inverses of the diagonal blocks
// allow_lookahead = false keeps everything on the lane's full-chip stream (several lanes running
// concurrently already fill the chip, and their masked stream pairs would only fight for HW queues)
void potrf_lower(gpmi_ctx* c, Lane& lane, double* A, int64_t np, int64_t ld, double* invD,
                 int* info, bool allow_lookahead = true);

// potrf_panel.hip: potrf_diag of a tile column and the panel TRSM under it in one launch (GPMI_PANEL_FUSED)
bool potrf_panel_fused(gpmi_ctx* c, Lane& lane);
void launch_panel_column(Lane& lane, hipStream_t s, double* Akk, int64_t ld, double* invD, int* info, int col0, int below,
                         int ncu, unsigned long long* dbg = nullptr, unsigned long long* stamp = nullptr);

// potrf_flow.hip: the chain-bound part of the factorisation as one persistent tile-task launch beside the panel chain
bool potrf_flow_enabled(gpmi_ctx* c, Lane& lane, int m);
bool potrf_flow_tail(gpmi_ctx* c, Lane& lane, double* A, int64_t ld, double* invD, int* info, int nt, int t0);
void potrf_flow_free(Lane& lane);

// solve.hip
// forward substitution  L v = r : the solution goes to `out` (no aliasing; `r` is only read).
// `err` (device int, may be null) receives GPMI_ERR_INTERNAL if the sweep's polling ever times out.
// `prefilled`: `out` already holds the sentinel (lane_run_early), the sweep does not fill it again.
void trsv_forward(gpmi_ctx* c, hipStream_t s, const double* L, int64_t np, int64_t ld,
                  const double* invD, const double* r, double* out, int* err = nullptr,
                  const BatchShape& bs = BatchShape(), bool prefilled = false);
// backward substitution  L^T a = v : the solution goes to `out` (no aliasing; `r` is only read)
void trsv_backward(gpmi_ctx* c, hipStream_t s, const double* L, int64_t np, int64_t ld,
                   const double* invD, const double* r, double* out, int* err = nullptr,
                   const BatchShape& bs = BatchShape(), bool prefilled = false);
// the lane's pending EarlyWork, if any, on stream s (the lane's own stream)
void lane_run_early(Lane& lane, hipStream_t s);
// lockstep batch: Q_z <- L_z^-T (np <= 4096), every launch carries the batch
void trsm_identity_batched(hipStream_t s, const double* L, int64_t np, int64_t ld, const double* invD, double* Q,
                           const BatchShape& bs);
// inverses of the 512-wide diagonal blocks of L from the 128-wide ones: inv2 (slots of 512 x 512, ld 512),
// tmp: slots of 256 x 256
constexpr int GPMI_OB = 512;
void build_inv2(hipStream_t s, const double* L, int64_t np, int64_t ld, const double* invD, double* inv2,
                double* tmp);
// X = Q L^-T  (forward solve of mp right-hand sides stored as rows of Q, mp x np, ld).  Q is consumed.
// Qout != nullptr: X goes to Qout (same shape / ld).  Qout == nullptr: X replaces Q, staged through
// `panel` (mp x 544).  upper_rhs: Q is upper triangular (rows below the current block still zero).
void trsm_rows_forward(gpmi_ctx* c, hipStream_t s, const double* L, int64_t np, int64_t ld,
                       const double* inv2, double* Q, int64_t mp, bool upper_rhs, double* Qout,
                       double* panel);
void launch_set_identity(hipStream_t s, double* Q, int64_t ld, int64_t np, int batch = 1, int64_t sMat = 0);
// device-to-device vector copy as a kernel (a runtime D2D memcpy stalled the stream for tens of ms)
void launch_copy(hipStream_t s, const double* src, double* dst, int64_t n);
// `height` rows of `width` doubles: src rows `spitch` doubles apart -> dst rows `dpitch` doubles apart
void launch_copy_rows(hipStream_t s, const double* src, int64_t spitch, double* dst, int64_t dpitch, int64_t width,
                      int64_t height);
// r = y - mu (padded with zeros)
void launch_residual(hipStream_t s, const double* y, const double* mu, double mu_const, double* r,
                     int64_t n, int64_t np);
// batched: r_z = y - mu_consts[z]  (or mus + z * n when mus != nullptr), r_z at r + z * sVec
void launch_residual_batched(hipStream_t s, const double* y, const double* mus, const double* mu_consts,
                             double* r, int64_t n, int64_t np, const BatchShape& bs);
// red[0] = sum v^2, red[1] = sum log diag(L)
void launch_lml_reduce(hipStream_t s, const double* v, const double* L, int64_t ld, int64_t np,
                       double* red, const BatchShape& bs = BatchShape());
// out[m] = sum_n Q[m][n] * a[n]
void launch_rows_dot(hipStream_t s, const double* Q, int64_t ld, int64_t mp, int64_t np,
                     const double* a, double* out, int batch = 1, int64_t sQ = 0, int64_t sVec = 0);
// out[m] = sign (base - sum_n Q[m][n]^2)
void launch_rows_sumsq(hipStream_t s, const double* Q, int64_t ld, int64_t mp, int64_t np,
                       double base, double* out, int batch = 1, int64_t sQ = 0, int64_t sVec = 0, double sign = 1.0);

// Q (mp x np) <- Q L^-1   (backward solve of mp right-hand sides stored as rows)
// (inv2 / panel: the 512 x 512 inverse blocks and an mp x (512 + 32) scratch panel, as for trsm_rows_forward; without them
// the sweep runs over the 128-wide blocks with invD)
void trsm_rows_backward(gpmi_ctx* c, hipStream_t s, const double* L, int64_t np, int64_t ld,
                        const double* invD, double* Q, int64_t mp, const double* inv2 = nullptr, double* panel = nullptr);

// generalised.hip: the kernels of the generalised GP (gpmi_ggp_*)
struct GgpTerms {
  double *g, *W, *sw, *d3, *b;  // np each: d log p / df, -d^2 log p / df^2, its root, d^3 log p / df^3, W (f - m) + g
};
struct GgpKv {
  const double* v[4];
  double* y[4];
};
int64_t ggp_part_doubles(int64_t np);
// the likelihood terms at f = fm + offset (a, fm, fm_prev: np each; fm_prev may be null) and the record
// rec[0..3] = {sum log p, a^T fm, max |fm - fm_prev|, max |f|}; part: ggp_part_doubles(np)
void launch_ggp_terms(hipStream_t s, int lik, const double* y, const double* aux, const double* lconst, double offset,
                      const double* a, const double* fm, const double* fm_prev, int64_t n, int64_t np, const GgpTerms& t,
                      double* part, double* rec);
// y[q] = K v[q] for q < nv (1 .. 4) in one pass over the np x np matrix K (both triangles stored); the bits of a product do
// not depend on nv
void launch_ggp_kv(hipStream_t s, const double* K, int64_t ld, int64_t np, int nv, const GgpKv& a);
void launch_ggp_blend(hipStream_t s, const double* lo, const double* hi, double step, double* out, int64_t cnt);
void launch_ggp_newton_a(hipStream_t s, const double* b, const double* sw, const double* t, double* a_new, int64_t np);
void launch_ggp_s2(hipStream_t s, const double* K, int64_t ld, const double* ss, const double* d3, double* s2, int64_t np);
void launch_ggp_grad_u(hipStream_t s, const double* g, const double* s2, const double* rt, double* u, int64_t np);
void launch_ggp_scale_cols(hipStream_t s, double* Q, int64_t ld, int64_t rows, int64_t np, const double* sc);

// predgrad.hip
void launch_sd_reduce(hipStream_t s, const KParams& p, const double* x, int64_t n, const double* pts,
                      int64_t m, const double* Kq, int64_t ld, const double* W, int64_t ldw,
                      double scale, double* out);
void launch_grad_rhs(hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np,
                     const double* pts, int64_t rows_valid, int64_t rows_padded, const double* Kq,
                     int64_t ld, double* G);
void launch_grad_cov(hipStream_t s, const KParams& p, const double* G, int64_t ld, int64_t np,
                     int64_t m, double* cov);
