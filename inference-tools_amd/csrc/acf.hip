// Circular autocorrelation sums of the columns of a sample, cut at the first negative lag: the device side of the
// effective sample size (effective_sample_size, reference inference/mcmc/utilities.py:83-95), with the C-ABI entry points
// gpmi_acf_columns and gpmi_acf_lag_blocks of include/gpmi.h.  For a column x of n rows, y = x - mean(x) and
//   f[k] = sum_{t < n} y[t] y[(t + k) mod n],   cut = the lowest k in [1, n / 2) with f[k] < 0,
// the entry point returns f[0], sum_{k < cut} f[k] and cut.  The reference takes f from an FFT of the whole column; only
// the lags below cut are ever used, which is tens to hundreds of lags for a converged chain, so the lags are summed
// directly and in rounds that stop, column by column, at the first negative one.
//
// A block of columns (as many as the workspace cap allows) is copied to the device and brought to one run of
// S = n + n / 2 doubles per column (a C-order block through col_transpose, a column-contiguous one by a pitched copy):
//   acf_centre  one workgroup per column: the sum of the column in a fixed order (a strided partial per thread, an LDS
//               tree), y = x - sum / n in place, the wrap-around tail y[n + j] = y[j] for j < n / 2 - the lag kernel
//               needs no modulo -, and the flag of a column holding a NaN or an infinity.
//   acf_lags    one round = one block of lags [K, K + B) (gpmi_acf_lag_blocks: 256, 256, 512, 1024, 2048, 2048, ...).
//               A workgroup takes one still-active column, ACF_T = 2048 values of t and 256 lags.  It stages y[t0 .. t0 + T)
//               (zero from t = n on) and y[t0 + K' .. t0 + K' + T + 256) in LDS.  A lane owns 8 consecutive lags and 256
//               consecutive t (a wave: 32 lag groups x 2 halves of t; 4 waves: 8 ranges of t): it keeps a window of 16
//               values in registers and per 8 values of t reads 8 new window values and 8 broadcast y[t] for 64 FMAs -
//               one LDS double per 4 FMAs.  The window rows are stored 80 bytes apart per 8 doubles, so the 16-byte
//               reads of 16 neighbouring lanes fall on 16 different groups of 4 banks.  The 8 ranges of t are added in
//               order through LDS and the workgroup writes 256 partials.
//   acf_finish  one workgroup per active column adds the partials in chunk order, finds the first negative lag of the
//               block, adds the lags before it to the column's running sum and marks the column done (cut found, or
//               the last block passed without one: flag 2, as for f[0] == 0).
// The host reads back the done marks of the active columns after a round and launches the next round for the rest:
// plain stream-ordered launches, no flags between workgroups.  Every sum is reduced in an order fixed by n alone (t inside
// a lane, the 8 ranges, the chunks, the lags of a block by thread and tree, the blocks by round), so a column alone and
// inside any batch, layout or workspace cap gives the same bits.  No atomics.
#include "api_internal.h"
#include "col_transpose.h"
#include "kde_state.h"

namespace {

constexpr int ACF_NT = 256;                    // threads of every kernel
constexpr int ACF_T = 2048;                    // values of t per workgroup of acf_lags
constexpr int ACF_LW = 256;                    // lags per workgroup of acf_lags, and the smallest block
constexpr int ACF_BMAX = 2048;                 // largest block of lags
constexpr int ACF_GROUPS = (ACF_T + ACF_LW) / 8;  // staged window: 288 groups of 8 doubles ...
constexpr int ACF_GPITCH = 10;                 // ... 10 doubles (80 bytes) apart
constexpr size_t ACF_DEFAULT_WS = (size_t)4 << 30;
constexpr int64_t ACF_MAX_N = (int64_t)1 << 30;
constexpr int64_t ACF_MAX_BLOCK = 65535;       // columns per block (grid.z of acf_lags)

// the block of lags that starts at K
inline int64_t acf_block(int64_t K) { return K == 0 ? ACF_LW : std::min<int64_t>(K, ACF_BMAX); }

__device__ __forceinline__ bool acf_finite(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// Column blockIdx.x of y (runs of S doubles, the first n given): centred in place, tail of kmax values, flag.
__global__ __launch_bounds__(ACF_NT) void acf_centre(double* __restrict__ y, int64_t S, int64_t n, int64_t kmax,
                                                     int* __restrict__ flag) {
  __shared__ double red[ACF_NT];
  double* p = y + (int64_t)blockIdx.x * S;
  double s = 0.0;
  int bad = 0;
  for (int64_t t = threadIdx.x; t < n; t += ACF_NT) {
    const double v = p[t];
    bad |= !acf_finite(v);
    s += v;
  }
  red[threadIdx.x] = s;
  bad = __syncthreads_or(bad);
  for (int h = ACF_NT >> 1; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const double mean = red[0] / (double)n;
  for (int64_t t = threadIdx.x; t < n; t += ACF_NT) p[t] = p[t] - mean;
  __syncthreads();  // (the tail reads what other threads of the workgroup have just written)
  for (int64_t j = threadIdx.x; j < kmax; j += ACF_NT) p[n + j] = p[j];
  if (threadIdx.x == 0) flag[blockIdx.x] = bad ? 1 : 0;
}

__device__ __forceinline__ void acf_load8(double* r, const double* sh) {
  const double2* q = reinterpret_cast<const double2*>(sh);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double2 v = q[i];
    r[2 * i] = v.x;
    r[2 * i + 1] = v.y;
  }
}

// Chunk blockIdx.x of t, lags [K + 256 blockIdx.y, + 256), column active[blockIdx.z]:
// part[((blockIdx.z * nchunk + blockIdx.x) * B + 256 blockIdx.y + j] = sum over the chunk's t < n of y[t] y[t + lag j]
__global__ __launch_bounds__(ACF_NT) void acf_lags(const double* __restrict__ y, int64_t S, int64_t n, int64_t K, int B,
                                                   int64_t nchunk, const int* __restrict__ active,
                                                   double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double A[ACF_T];
  __shared__ __attribute__((aligned(16))) double W[ACF_GROUPS * ACF_GPITCH];
  const double* p = y + (int64_t)active[blockIdx.z] * S;
  const int64_t t0 = (int64_t)blockIdx.x * ACF_T;
  const int64_t w0 = t0 + K + (int64_t)blockIdx.y * ACF_LW;
  for (int e = threadIdx.x; e < ACF_T; e += ACF_NT) A[e] = t0 + e < n ? p[t0 + e] : 0.0;
  // (a valid lag k < n / 2 at t < n reads y[t + k] with t + k < S; what lies beyond belongs to lags that nobody uses)
  for (int e = threadIdx.x; e < ACF_GROUPS * 8; e += ACF_NT) W[e + 2 * (e >> 3)] = w0 + e < S ? p[w0 + e] : 0.0;
  __syncthreads();
  const int lane = threadIdx.x & 63, lg = lane & 31;
  const int sub = (threadIdx.x >> 6) * 2 + (lane >> 5);  // the range [256 sub, 256 sub + 256) of the chunk's t
  const double* a_ptr = A + sub * 256;
  const double* w_ptr = W + (sub * 32 + lg) * ACF_GPITCH;  // group sub * 32 + lg: element t + 8 lg of the window
  double acc[8], w[16], a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  acf_load8(w, w_ptr);
#pragma unroll 2
  for (int g = 0; g < 32; ++g) {
    acf_load8(w + 8, w_ptr + (g + 1) * ACF_GPITCH);  // (the last group read is 7 * 32 + 31 + 32 = 287 < ACF_GROUPS)
    acf_load8(a, a_ptr + g * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fma(a[i], w[i + j], acc[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = w[j + 8];
  }
  __syncthreads();  // W becomes the 8 x 256 table of the ranges' sums
#pragma unroll
  for (int j = 0; j < 8; ++j) W[sub * ACF_LW + 8 * lg + j] = acc[j];
  __syncthreads();
  double s = W[threadIdx.x];
#pragma unroll
  for (int q = 1; q < 8; ++q) s += W[q * ACF_LW + threadIdx.x];
  part[((int64_t)blockIdx.z * nchunk + blockIdx.x) * B + blockIdx.y * ACF_LW + threadIdx.x] = s;
}

// Active column blockIdx.x after the round of the block [K, K + B): f of the block from the partials, the first negative
// lag, the running sum, done[blockIdx.x].
__global__ __launch_bounds__(ACF_NT) void acf_finish(const double* __restrict__ part, int64_t nchunk, int64_t K, int B,
                                                     int64_t kmax, const int* __restrict__ active, int* __restrict__ flag,
                                                     double* __restrict__ f0, double* __restrict__ sum,
                                                     long long* __restrict__ cut, int* __restrict__ done) {
  __shared__ double f[ACF_BMAX];
  __shared__ double red[ACF_NT];
  __shared__ int redi[ACF_NT];
  const int col = active[blockIdx.x];
  const double* q = part + (int64_t)blockIdx.x * nchunk * B;
  for (int j = threadIdx.x; j < B; j += ACF_NT) {
    double s = 0.0;
    for (int64_t c = 0; c < nchunk; ++c) s += q[c * B + j];
    f[j] = s;
  }
  __syncthreads();
  int cand = INT32_MAX;
  for (int j = threadIdx.x; j < B; j += ACF_NT) {
    const int64_t k = K + j;
    if (k >= 1 && k < kmax && f[j] < 0.0) {
      cand = j;
      break;
    }
  }
  redi[threadIdx.x] = cand;
  __syncthreads();
  for (int h = ACF_NT >> 1; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h && redi[threadIdx.x + h] < redi[threadIdx.x]) redi[threadIdx.x] = redi[threadIdx.x + h];
    __syncthreads();
  }
  cand = redi[0];
  const bool found = cand != INT32_MAX;
  const int64_t left = kmax - K;  // lags of the block that exist (at least 1)
  const int lim = found ? cand : (int)(left < B ? left : B);
  double s = 0.0;
  for (int j = threadIdx.x; j < lim; j += ACF_NT) s += f[j];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = ACF_NT >> 1; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double f0v = K == 0 ? f[0] : f0[col];
    if (K == 0) f0[col] = f0v;
    sum[col] = (K == 0 ? 0.0 : sum[col]) + red[0];
    int d = 0, none = 0;
    if (found) {
      cut[col] = K + cand;
      d = 1;
    } else if (K + B >= kmax) {
      none = 1;
    }
    if (K == 0 && !(f0v > 0.0)) none = 1;  // a constant column (and one whose sums are NaN)
    if (flag[col] == 1) d = 1;             // a non-finite column: its numbers mean nothing, it leaves at once
    else if (none) {
      flag[col] = 2;
      d = 1;
    }
    done[blockIdx.x] = d;
  }
}

}  // namespace

extern "C" {

int gpmi_acf_lag_blocks(int64_t n, int64_t cap, int64_t* starts, int64_t* count) {
  if (!count || n < 2 || cap < 0 || (cap > 0 && !starts)) return GPMI_ERR_ARG;
  const int64_t kmax = n / 2;
  int64_t cnt = 0;
  for (int64_t K = 0; K < kmax; K += acf_block(K)) {
    if (starts && cnt < cap) starts[cnt] = K;
    ++cnt;
  }
  *count = cnt;
  return starts && cnt > cap ? GPMI_ERR_ARG : GPMI_OK;
}

int gpmi_acf_columns(gpmi_ctx* c, int64_t n, int64_t m, int64_t row_stride, int64_t col_stride, const double* sample,
                     int64_t ws_bytes, double* f0, double* sum, int64_t* cut, int32_t* flag) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, sample && f0 && sum && cut && flag, "gpmi_acf_columns: sample, f0, sum, cut and flag must be non-NULL");
  ARGCHK(c, n >= 2 && n <= ACF_MAX_N, "gpmi_acf_columns: n out of range (2 .. 2^30)");
  ARGCHK(c, m >= 1 && m <= INT32_MAX, "gpmi_acf_columns: m out of range (1 .. 2^31 - 1)");
  ARGCHK(c, ws_bytes >= 0, "gpmi_acf_columns: ws_bytes must not be negative");
  // the two dense layouts; a single column is one contiguous run either way
  const bool by_col = row_stride == 1 && (col_stride >= n || m == 1);
  const bool by_row = !by_col && col_stride == 1 && row_stride >= m;
  ARGCHK(c, by_col || by_row,
         "gpmi_acf_columns: the strides must be (ld, 1) with ld >= m or (1, ld) with ld >= n, in elements");
  const int64_t ld = by_col ? (m == 1 ? n : col_stride) : row_stride;
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;

  const int64_t kmax = n / 2, S = n + kmax;
  const int64_t nchunk = (n + ACF_T - 1) / ACF_T;
  int64_t bmax = ACF_LW;  // the largest block of the schedule
  for (int64_t K = 0; K < kmax; K += acf_block(K)) bmax = std::max(bmax, acf_block(K));
  const size_t cap = ws_bytes ? (size_t)ws_bytes : ACF_DEFAULT_WS;
  const size_t col_bytes = 8 * (size_t)n, y_bytes = 8 * (size_t)S, p_bytes = 8 * (size_t)nchunk * (size_t)bmax;
  const size_t small = 8 + 8 + 8 + 4 + 4 + 4;  // f0, sum, cut, flag, the active list and the done marks
  const size_t per_col = (by_row ? col_bytes : 0) + y_bytes + p_bytes + small;
  const size_t fixed = 9 * 256;  // the alignment of nine regions
  if (cap < fixed + per_col) {
    c->err = "gpmi_acf_columns: one column of " + std::to_string(n) + " rows needs " + std::to_string(fixed + per_col) +
             " bytes of workspace, more than the cap of " + std::to_string(cap);
    return GPMI_ERR_ARG;
  }
  const int64_t mb_max = std::min<int64_t>(std::min<int64_t>(m, ACF_MAX_BLOCK), (int64_t)((cap - fixed) / per_col));

  // the workspace, carved for the largest (first) block
  const size_t raw_b = by_row ? kde_align256(col_bytes * mb_max) : 0;
  const size_t y_b = kde_align256(y_bytes * mb_max);
  const size_t part_b = kde_align256(p_bytes * mb_max);
  const size_t d8_b = kde_align256(8 * (size_t)mb_max), d4_b = kde_align256(4 * (size_t)mb_max);
  if (int rc = st->reserve_work(c, raw_b + y_b + part_b + 3 * d8_b + 3 * d4_b))
    return rc;
  if (int rc = st->reserve_pinned(c, 3 * d8_b + 3 * d4_b)) return rc;
  char* w = st->d_work;
  double* d_raw = reinterpret_cast<double*>(w);
  double* d_y = reinterpret_cast<double*>(w + raw_b);
  double* d_part = reinterpret_cast<double*>(w + raw_b + y_b);
  char* d_res = w + raw_b + y_b + part_b;  // f0, sum, cut, flag: one run, copied back together
  double* d_f0 = reinterpret_cast<double*>(d_res);
  double* d_sum = reinterpret_cast<double*>(d_res + d8_b);
  long long* d_cut = reinterpret_cast<long long*>(d_res + 2 * d8_b);
  int* d_flag = reinterpret_cast<int*>(d_res + 3 * d8_b);
  int* d_act = reinterpret_cast<int*>(d_res + 3 * d8_b + d4_b);
  int* d_done = reinterpret_cast<int*>(d_res + 3 * d8_b + 2 * d4_b);
  char* h_res = st->h_stage;
  int* h_act = reinterpret_cast<int*>(st->h_stage + 3 * d8_b + d4_b);
  int* h_done = reinterpret_cast<int*>(st->h_stage + 3 * d8_b + 2 * d4_b);

  for (int64_t c0 = 0; c0 < m; c0 += mb_max) {
    const int64_t mb = std::min<int64_t>(mb_max, m - c0);
    // the block as it lies on the host: n rows of mb doubles (by_row), or mb rows of n doubles (by_col)
    const double* src = sample + (by_row ? c0 : c0 * ld);
    if (by_row) {
      const size_t width = 8 * (size_t)mb;
      if ((size_t)ld * 8 == width) {
        HIPCHK(c, hipMemcpyAsync(d_raw, src, width * (size_t)n, hipMemcpyHostToDevice, st->stream));
      } else {
        HIPCHK(c, hipMemcpy2DAsync(d_raw, width, src, 8 * (size_t)ld, width, (size_t)n, hipMemcpyHostToDevice, st->stream));
      }
      hipLaunchKernelGGL(col_transpose, dim3((unsigned)((n + 31) / 32), (unsigned)((mb + 31) / 32)), dim3(256), 0, st->stream,
                         d_raw, d_y, n, mb, S);
      HIPCHK(c, hipGetLastError());
    } else if (mb == 1) {
      HIPCHK(c, hipMemcpyAsync(d_y, src, col_bytes, hipMemcpyHostToDevice, st->stream));
    } else {
      HIPCHK(c, hipMemcpy2DAsync(d_y, y_bytes, src, 8 * (size_t)ld, col_bytes, (size_t)mb, hipMemcpyHostToDevice, st->stream));
    }
    HIPCHK(c, hipMemsetAsync(d_res, 0, 3 * d8_b, st->stream));  // (a flagged column may never write its numbers)
    hipLaunchKernelGGL(acf_centre, dim3((unsigned)mb), dim3(ACF_NT), 0, st->stream, d_y, S, n, kmax, d_flag);
    HIPCHK(c, hipGetLastError());

    int64_t nact = mb;
    for (int64_t i = 0; i < mb; ++i) h_act[i] = (int)i;
    for (int64_t K = 0; K < kmax && nact > 0; K += acf_block(K)) {
      const int B = (int)acf_block(K);
      HIPCHK(c, hipMemcpyAsync(d_act, h_act, 4 * (size_t)nact, hipMemcpyHostToDevice, st->stream));
      hipLaunchKernelGGL(acf_lags, dim3((unsigned)nchunk, (unsigned)(B / ACF_LW), (unsigned)nact), dim3(ACF_NT), 0, st->stream,
                         d_y, S, n, K, B, nchunk, d_act, d_part);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(acf_finish, dim3((unsigned)nact), dim3(ACF_NT), 0, st->stream, d_part, nchunk, K, B, kmax, d_act,
                         d_flag, d_f0, d_sum, d_cut, d_done);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(h_done, d_done, 4 * (size_t)nact, hipMemcpyDeviceToHost, st->stream));
      HIPCHK(c, hipStreamSynchronize(st->stream));
      int64_t keep = 0;
      for (int64_t i = 0; i < nact; ++i)
        if (!h_done[i]) h_act[keep++] = h_act[i];
      nact = keep;
    }
    HIPCHK(c, hipMemcpyAsync(h_res, d_res, 3 * d8_b + 4 * (size_t)mb, hipMemcpyDeviceToHost, st->stream));
    HIPCHK(c, hipStreamSynchronize(st->stream));
    std::memcpy(f0 + c0, h_res, 8 * (size_t)mb);
    std::memcpy(sum + c0, h_res + d8_b, 8 * (size_t)mb);
    std::memcpy(cut + c0, h_res + 2 * d8_b, 8 * (size_t)mb);
    std::memcpy(flag + c0, h_res + 3 * d8_b, 4 * (size_t)mb);
  }
  return GPMI_OK;
}

}  // extern "C"
