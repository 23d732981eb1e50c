// Greedy conditional-variance selection of inducing points (include/gpmi.h: gpmi_select_points): the pivoted partial
// Cholesky factorisation of C = K / a^2 over n points, one launch per step.
//
//   step t:  p = argmax over the eligible of w_i d_i (lowest index among equals),  c_i = C(x_i, x_p) - sum_{l<t} V_li V_lp,
//            V_ti = c_i / sqrt(d_p),  d_i <- max(d_i - V_ti^2, 0),  d_p <- 0,  tr_{t+1} = sum_i w_i d_i
//
// A workgroup owns 256 consecutive points, one per thread.  Launch t opens with the finish of step t - 1: every workgroup
// reduces the block partials (best score, lowest index, its d, partial trace) that launch t - 1 left, in one fixed order,
// so all of them arrive at the same pivot and the same stop decision without talking to each other; workgroup 0 writes
// the step's results.  Then the pivot's coordinates and its column V_{0..t-1, p} go to LDS once and the sweep reads row l
// of V for the workgroup's points, coalesced, eight rows in flight per thread: a step moves 8 t n bytes, a selection
// 8 n m^2 / 2 - it is bound by HBM.  The steps are ordered by the launch boundaries of the stream alone: no workgroup
// waits for another, nothing is summed with atomics, the host does not synchronise until the last launch is enqueued.
// Once a step stops the selection the word `stop` is set and the launches behind it return at once.
//
// Bits: s = sum_k 1/2 dx_k^2 / l_k^2 is the chain of pair_tile::accumulate_s (one fma per dimension, ascending k) and C
// comes from kfun<KERNEL, 1>, so C(x_i, x_p) is the builders' value; the sum over l runs in ascending l in one chain.
// V_ti therefore depends on (x_i, the pivots, theta) alone, not on n or on the place of row i.
#include <limits>

#include "api_internal.h"
#include "pair_tile.h"

namespace {

constexpr int SEL_NT = 256;     // threads = points per workgroup
constexpr int SEL_UNROLL = 8;   // rows of V in flight per thread

// what a workgroup (and, reduced, a step) knows of its points
struct SelPartial {
  double score;  // max w_i d_i over the eligible points; -1: none
  double dvar;   // d of that point
  double trace;  // sum w_i d_i over all points
  int idx;       // that point, the lowest index among equal scores; -1: none
  int pad;
};

struct SelState {
  const double* x;    // n x d
  const double* w;    // n or nullptr (all 1)
  double* dvar;       // n: d_i
  double* V;          // m_max x n, row t contiguous
  SelPartial* part;   // 2 x nblocks: launch t reads half t & 1 and writes the other
  int64_t* index;     // m_max pivots
  double* trace;      // m_max + 1
  double* pivot_var;  // m_max
  int* word;          // [0] stop, [1] count
  int64_t n;
  int nblocks, m_max;
  double floor_rel, trace_tol;
};

__device__ __forceinline__ bool sel_better(double sa, int ia, double sb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return sa > sb || (sa == sb && ia < ib);
}

// the best (score, index, d) and the sum of the traces of the 256 threads' values, the same in every thread: shuffles
// inside a wave, the four waves through LDS, in one fixed order
__device__ inline SelPartial sel_block_reduce(double score, int idx, double dv, double tr, double* red_d, int* red_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double s2 = __shfl_down(score, off, 64), d2 = __shfl_down(dv, off, 64);
    const int i2 = __shfl_down(idx, off, 64);
    tr += __shfl_down(tr, off, 64);
    if (sel_better(s2, i2, score, idx)) {
      score = s2;
      idx = i2;
      dv = d2;
    }
  }
  __syncthreads();  // (red_* may still be read from the previous call)
  if (lane == 0) {
    red_d[wave * 3 + 0] = score;
    red_d[wave * 3 + 1] = dv;
    red_d[wave * 3 + 2] = tr;
    red_i[wave] = idx;
  }
  __syncthreads();
  SelPartial r;
  r.score = red_d[0];
  r.dvar = red_d[1];
  r.trace = red_d[2];
  r.idx = red_i[0];
  r.pad = 0;
#pragma unroll
  for (int k = 1; k < SEL_NT / 64; ++k) {
    r.trace += red_d[k * 3 + 2];
    if (sel_better(red_d[k * 3], red_i[k], r.score, r.idx)) {
      r.score = red_d[k * 3];
      r.dvar = red_d[k * 3 + 1];
      r.idx = red_i[k];
    }
  }
  return r;
}

// t < 0: d_i = 1 and the partials step 0 opens with.  0 <= t < m_max: step t.  t = m_max: the finish of the last step alone.
template <int KERNEL>
__global__ __launch_bounds__(SEL_NT) void select_step_kernel(KParams p, SelState st, int t) {
  __shared__ double s_col[GPMI_SGP_MAX_M];  // V_{l, pivot}, l < t
  __shared__ double s_xp[GPMI_MAX_D];
  __shared__ double red_d[3 * SEL_NT / 64];
  __shared__ int red_i[SEL_NT / 64];
  if (t >= 0 && st.word[0] != 0) return;
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * SEL_NT + tid;
  const bool valid = i < st.n;
  const double wi = valid ? (st.w ? st.w[i] : 1.0) : 0.0;
  double di = 1.0;
  if (t >= 0) {
    // the finish of step t - 1: block partials in ascending order per thread, then the fixed tree
    const SelPartial* in = st.part + (size_t)(t & 1) * st.nblocks;
    double score = -1.0, dv = 0.0, tr = 0.0;
    int idx = -1;
    for (int b = tid; b < st.nblocks; b += SEL_NT) {
      const SelPartial q = in[b];
      tr += q.trace;
      if (sel_better(q.score, q.idx, score, idx)) {
        score = q.score;
        idx = q.idx;
        dv = q.dvar;
      }
    }
    const SelPartial best = sel_block_reduce(score, idx, dv, tr, red_d, red_i);
    const double tr0 = (t == 0) ? best.trace : st.trace[0];  // (written by launch 0, a launch boundary ago)
    const bool stop = t == st.m_max || best.idx < 0 || best.trace <= st.trace_tol * tr0;
    if (blockIdx.x == 0 && tid == 0) {
      st.trace[t] = best.trace;
      if (stop) {
        st.word[1] = t;
        st.word[0] = 1;
      } else {
        st.index[t] = best.idx;
        st.pivot_var[t] = best.dvar;
      }
    }
    if (stop) return;
    const int64_t piv = best.idx;
    for (int k = tid; k < p.d; k += SEL_NT) s_xp[k] = st.x[piv * p.d + k];
    for (int l = tid; l < t; l += SEL_NT) s_col[l] = st.V[(int64_t)l * st.n + piv];
    __syncthreads();
    if (valid) {
      const double* xi = st.x + i * p.d;
      double s1[1] = {0.0}, C1[1];
      for (int k = 0; k < p.d; ++k) {
        const double dx = xi[k] - s_xp[k];
        s1[0] = fma(0.5 * dx * dx, p.inv_l2[k], s1[0]);
      }
      kfun<KERNEL, 1>(p, s1, C1);
      const double* Vi = st.V + i;
      double acc = 0.0;
      int l = 0;
      for (; l + SEL_UNROLL <= t; l += SEL_UNROLL) {
        double v[SEL_UNROLL];
#pragma unroll
        for (int u = 0; u < SEL_UNROLL; ++u) v[u] = Vi[(int64_t)(l + u) * st.n];
#pragma unroll
        for (int u = 0; u < SEL_UNROLL; ++u) acc = fma(v[u], s_col[l + u], acc);
      }
      for (; l < t; ++l) acc = fma(Vi[(int64_t)l * st.n], s_col[l], acc);
      const double v = (C1[0] - acc) / sqrt(best.dvar);
      st.V[(int64_t)t * st.n + i] = v;
      di = (i == piv) ? 0.0 : fmax(st.dvar[i] - v * v, 0.0);
      st.dvar[i] = di;
    }
  } else if (valid) {
    st.dvar[i] = 1.0;
  }
  const bool eligible = valid && di > st.floor_rel && wi > 0.0;
  const SelPartial mine = sel_block_reduce(eligible ? wi * di : -1.0, eligible ? (int)i : -1, di, valid ? wi * di : 0.0, red_d, red_i);
  if (tid == 0) st.part[(size_t)((t + 1) & 1) * st.nblocks + blockIdx.x] = mine;
}

// workgroups of a step (one point per thread), the block partials every workgroup reduces at the next launch
int select_blocks(int64_t n) { return (int)((n + SEL_NT - 1) / SEL_NT); }
bool select_n_ok(int64_t n) { return n >= 1 && n <= ((int64_t)1 << 30); }

int select_arg_error(gpmi_ctx* c, const char* what) {
  c->err = std::string("gpmi_select_points: ") + what;
  return GPMI_ERR_ARG;
}

}  // namespace

extern "C" int gpmi_select_schedule(int64_t n, int64_t out[1]) {
  if (!out || !select_n_ok(n)) return GPMI_ERR_ARG;
  out[0] = select_blocks(n);
  return GPMI_OK;
}

extern "C" int gpmi_select_points(gpmi_ctx* c, int64_t n, int64_t d, const double* x, const double* weight, int kernel,
                                  const double* theta, int n_theta, int64_t m_max, double floor_rel, double trace_tol,
                                  int64_t* index, double* trace, double* pivot_var, int64_t* count) {
  if (!c) return GPMI_ERR_ARG;
  if (!x || !theta || !index || !trace || !count)
    return select_arg_error(c, "x_host, theta, index_host, trace_host and count must be non-NULL");
  if (!select_n_ok(n)) return select_arg_error(c, "n out of range (1 .. 2^30)");
  if (d < 1 || d > GPMI_MAX_D) return select_arg_error(c, "d out of range (1 .. 64)");
  if (m_max < 1 || m_max > std::min<int64_t>(n, GPMI_SGP_MAX_M))
    return select_arg_error(c, "m_max out of range (1 .. min(n, 4096 = GPMI_SGP_MAX_M))");
  if (kernel == GPMI_KERNEL_SUM || !kernel_is_stationary(kernel))
    return select_arg_error(c, "the kernel must be GPMI_KERNEL_SE, _RQ, _M32 or _M52");
  const int off = kernel_theta_offset(kernel);
  if (n_theta != d + off) return select_arg_error(c, "n_theta does not match the kernel and the data dimension");
  for (int k = 0; k < n_theta; ++k)
    if (!std::isfinite(theta[k])) return select_arg_error(c, "theta must be finite");
  if (!(std::isfinite(floor_rel) && floor_rel >= 0.0)) return select_arg_error(c, "floor_rel must be finite and not negative");
  if (!(std::isfinite(trace_tol) && trace_tol >= 0.0)) return select_arg_error(c, "trace_tol must be finite and not negative");
  for (int64_t k = 0; k < n * d; ++k)
    if (!std::isfinite(x[k])) return select_arg_error(c, "x_host must be finite");
  if (weight) {
    bool positive = false;
    for (int64_t k = 0; k < n; ++k) {
      if (!(std::isfinite(weight[k]) && weight[k] >= 0.0)) return select_arg_error(c, "the weights must be finite and not negative");
      positive = positive || weight[k] > 0.0;
    }
    if (!positive) return select_arg_error(c, "the weights have no positive entry");
  }
  KParams p;
  std::memset(&p, 0, sizeof(p));
  p.kernel = kernel;
  p.d = (int)d;
  p.a2 = 1.0;  // (theta[0] = ln a is not used: the selection works on K / a^2)
  p.kappa = (kernel == GPMI_KERNEL_RQ) ? std::exp(theta[1]) : 1.0;
  for (int k = 0; k < p.d; ++k) {
    const double l = std::exp(theta[off + k]);
    p.inv_l2[k] = 1.0 / (l * l);
  }
  if (int rc = set_device(c)) return rc;
  if (!c->sgp_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->sgp_stream, hipStreamNonBlocking));
  hipStream_t s = c->sgp_stream;

  // device memory of the call, released at return
  const int nblocks = select_blocks(n);
  const int mm = (int)m_max;
  DevBuf<double> bx, bw, bd, bV, btr, bpv;
  DevBuf<SelPartial> bpart;
  DevBuf<int64_t> bidx;
  DevBuf<int> bword;
  if (int rc = bV.alloc(c, n * m_max)) return rc;
  if (int rc = bx.alloc(c, n * d)) return rc;
  if (weight)
    if (int rc = bw.alloc(c, n)) return rc;
  if (int rc = bd.alloc(c, n)) return rc;
  if (int rc = bpart.alloc(c, 2 * nblocks)) return rc;
  if (int rc = bidx.alloc(c, m_max)) return rc;
  if (int rc = btr.alloc(c, m_max + 1)) return rc;
  if (int rc = bpv.alloc(c, m_max)) return rc;
  if (int rc = bword.alloc(c, 2)) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipMemcpy(bx, x, sizeof(double) * (size_t)n * (size_t)d, hipMemcpyHostToDevice));
  if (weight) HIPCHK(c, hipMemcpy(bw, weight, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  ZERO_SYNC(c, bword, sizeof(int) * 2);

  SelState st;
  st.x = bx;
  st.w = weight ? bw : nullptr;
  st.dvar = bd;
  st.V = bV;
  st.part = bpart;
  st.index = bidx;
  st.trace = btr;
  st.pivot_var = bpv;
  st.word = bword;
  st.n = n;
  st.nblocks = nblocks;
  st.m_max = mm;
  st.floor_rel = floor_rel;
  st.trace_tol = trace_tol;
  with_stationary_kernel(kernel, [&](auto K) {
    // launch -1 sets the state up, launch t <= m_max finishes step t - 1 and, below m_max, sweeps step t
    for (int t = -1; t <= mm; ++t)
      hipLaunchKernelGGL(select_step_kernel<decltype(K)::value>, dim3((unsigned)nblocks), dim3(SEL_NT), 0, s, p, st, t);
  });
  HIPCHK(c, hipGetLastError());
  int word[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(word, st.word, sizeof(word), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const int64_t cnt = word[1];
  if (word[0] != 1 || cnt < 0 || cnt > m_max) {
    c->err = "gpmi_select_points: internal error: the selection did not come to its end";
    return GPMI_ERR_INTERNAL;
  }
  // entries beyond count stay as the caller left them
  if (cnt > 0) {
    HIPCHK(c, hipMemcpy(index, st.index, sizeof(int64_t) * (size_t)cnt, hipMemcpyDeviceToHost));
    if (pivot_var) HIPCHK(c, hipMemcpy(pivot_var, st.pivot_var, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost));
  }
  HIPCHK(c, hipMemcpy(trace, st.trace, sizeof(double) * (size_t)(cnt + 1), hipMemcpyDeviceToHost));
  *count = cnt;
  return GPMI_OK;
}
