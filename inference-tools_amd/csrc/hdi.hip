// Highest-density intervals of the columns of a sample (sample_hdi, reference inference/pdf/hdi.py:6-105) on the device,
// with the C-ABI entry point gpmi_hdi_columns of include/gpmi.h.  For a column sorted ascending into s and a window
// length L < n the answer is (s[i*], s[i* + L]) with i* the LOWEST i that attains min_i (s[i + L] - s[i]), 0 <= i < n - L
// (hdi.py:94-104, numpy's argmin); for L >= n it is (s[0], s[n - 1]).  The kernels compare doubles and make that one
// subtraction, so a finite column gives the reference's bits.
//
// A block of columns (as many as the workspace cap allows) is copied to the device as it lies in host memory (a pitched
// copy) and brought to one contiguous run of n doubles per column: a C-order block is transposed through a 32 x 33 LDS
// tile (col_transpose of col_transpose.h, both sides coalesced), a column-contiguous one lands there directly.  Then
//   n <= HDI_C  hdi_small: a workgroup loads one column (or, below 2048 rows, 2048 / P columns of P = max(64, 2^ceil(log2
//               n)) slots each) into LDS, pads with +inf, sorts with a direction-free bitonic network and scans every
//               window length straight from LDS.
//   n >  HDI_C  hdi_chunk_sort sorts HDI_C-element chunks in LDS in place; ceil(log2(chunks)) passes of hdi_merge between
//               two global buffers double the run length (each workgroup makes a fixed 2048-element tile of the output:
//               it finds its two diagonals by binary search - merge path -, stages the two input pieces in LDS, merges
//               8 outputs per thread and stores the tile coalesced; a last run without a partner is "merged" with an
//               empty one, which copies it); hdi_window makes the partial minimum of 4096 window starts per workgroup
//               and hdi_window_finish reduces the partials of a (column, L).
// Every minimum is over (w, i) pairs ordered by w, then i, in LDS trees: no atomics, the lowest index wins, and the
// result does not depend on launch order.  A column of 10^7 rows is 1221 chunks, 4883 merge tiles per pass and 2442
// window workgroups: it spreads over the chip.
//
// Non-finite input: a column holding NaN or +-inf sets flag[column] (the caller discards its numbers and recomputes it
// on the host).  The kernels never index by an assumption of order: the sorting network is data-oblivious, both
// merge-path searches keep their two indices inside the runs by construction of [lo, hi], the piece lengths are
// clamped to the runs, and the serial merge checks both cursors - so such a column costs what any other does, stays
// in bounds and terminates.
#include "api_internal.h"
#include "col_transpose.h"
#include "kde_state.h"

#pragma clang fp contract(off)

namespace {

constexpr int HDI_C = 8192;        // chunk capacity in doubles: 64 KiB of LDS, two workgroups per CU
constexpr int HDI_NT = 512;        // threads of the LDS sort kernels
constexpr int HDI_PACK = 2048;     // slots of a packed workgroup (columns of fewer rows share one)
constexpr int HDI_PMIN = 64;       // fewest slots per column: at most 32 columns per workgroup, 16 threads each
constexpr int HDI_TILE = 2048;     // outputs of a merge workgroup
constexpr int HDI_MT = 256;        // threads of the merge and window kernels
constexpr int HDI_ITEMS = HDI_TILE / HDI_MT;
constexpr int HDI_WCH = 4096;      // window starts per workgroup of hdi_window
constexpr size_t HDI_DEFAULT_WS = (size_t)4 << 30;
constexpr int64_t HDI_MAX_N = (int64_t)1 << 30;
constexpr int64_t HDI_MAX_BLOCK = 65535;  // columns per block (grid.z of hdi_window, grid.y of the others)

struct WinPart {
  double w;
  long long i;
};

__device__ __forceinline__ bool hdi_finite(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

__device__ __forceinline__ double hdi_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ void cmpswap(double* sh, int i, int j) {
  const double a = sh[i], b = sh[j];
  if (b < a) {
    sh[i] = b;
    sh[j] = a;
  }
}

// Ascending sort of every aligned block of P slots of sh[0 .. T) (T, P powers of two, P <= T): the bitonic network in its
// direction-free form (the first step of a stage mirrors the upper half), the same index pattern whatever the data.
__device__ __forceinline__ void bitonic_blocks(double* sh, int T, int P) {
  const int half = T >> 1;
  for (int k = 2; k <= P; k <<= 1) {
    const int hk = k >> 1;
    for (int t = threadIdx.x; t < half; t += blockDim.x) {
      const int blk = t / hk, off = t - blk * hk;
      cmpswap(sh, blk * k + off, blk * k + k - 1 - off);
    }
    __syncthreads();
    for (int j = hk >> 1; j >= 1; j >>= 1) {
      for (int t = threadIdx.x; t < half; t += blockDim.x) {
        const int i = 2 * j * (t / j) + (t % j);
        cmpswap(sh, i, i + j);
      }
      __syncthreads();
    }
  }
}

// (w, i) < (bw, bi) in the order by w, then i
__device__ __forceinline__ bool win_less(double w, long long i, double bw, long long bi) {
  return w < bw || (w == bw && i < bi);
}

// n <= HDI_C: cpw columns of P slots per workgroup (cpw * P = T <= HDI_C), sort and window scan in LDS.
// out[(f * 2 + side) * mb + column], flag[column]
__global__ __launch_bounds__(HDI_NT) void hdi_small(const double* __restrict__ cols, int n, int64_t mb, int P, int cpw,
                                                    int n_frac, const long long* __restrict__ Ls, double* __restrict__ out,
                                                    int* __restrict__ flag) {
  __shared__ double sh[HDI_C];
  __shared__ double redw[HDI_NT];
  __shared__ int redi[HDI_NT];
  __shared__ int bad[HDI_PACK / HDI_PMIN];
  const int T = cpw * P;
  const int64_t col0 = (int64_t)blockIdx.x * cpw;
  if (threadIdx.x < cpw) bad[threadIdx.x] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < T; e += HDI_NT) {
    const int j = e / P, r = e - j * P;
    const int64_t col = col0 + j;
    double v = hdi_inf();
    if (col < mb && r < n) {
      v = cols[col * n + r];
      if (!hdi_finite(v)) atomicOr(&bad[j], 1);
    }
    sh[e] = v;
  }
  __syncthreads();
  bitonic_blocks(sh, T, P);
  const int tpc = HDI_NT / cpw;  // threads of a column
  const int j = threadIdx.x / tpc, lt = threadIdx.x - j * tpc;
  const int64_t col = col0 + j;
  const double* s = sh + j * P;
  if (lt == 0 && col < mb) flag[col] = bad[j];
  for (int f = 0; f < n_frac; ++f) {
    const long long L = Ls[f];
    if (L >= n) {  // (the same for every column of the call)
      if (lt == 0 && col < mb) {
        out[(int64_t)(2 * f) * mb + col] = s[0];
        out[(int64_t)(2 * f + 1) * mb + col] = s[n - 1];
      }
      continue;
    }
    const int cnt = n - (int)L;
    double bw = hdi_inf();
    int bi = INT32_MAX;
    for (int i = lt; i < cnt; i += tpc) {
      const double w = s[i + L] - s[i];
      if (win_less(w, i, bw, bi)) {
        bw = w;
        bi = i;
      }
    }
    redw[threadIdx.x] = bw;
    redi[threadIdx.x] = bi;
    __syncthreads();
    for (int h = tpc >> 1; h >= 1; h >>= 1) {
      if (lt < h && win_less(redw[threadIdx.x + h], redi[threadIdx.x + h], redw[threadIdx.x], redi[threadIdx.x])) {
        redw[threadIdx.x] = redw[threadIdx.x + h];
        redi[threadIdx.x] = redi[threadIdx.x + h];
      }
      __syncthreads();
    }
    if (lt == 0 && col < mb) {
      int i = redi[threadIdx.x];
      if (i >= cnt) i = 0;  // (only a column of NaN differences)
      out[(int64_t)(2 * f) * mb + col] = s[i];
      out[(int64_t)(2 * f + 1) * mb + col] = s[i + L];
    }
    __syncthreads();
  }
}

// n > HDI_C: chunk blockIdx.x of column blockIdx.y, sorted in place
__global__ __launch_bounds__(HDI_NT) void hdi_chunk_sort(double* __restrict__ cols, int64_t n, int* __restrict__ flag) {
  __shared__ double sh[HDI_C];
  double* p = cols + (int64_t)blockIdx.y * n;
  const int64_t base = (int64_t)blockIdx.x * HDI_C;
  bool bad = false;
  for (int e = threadIdx.x; e < HDI_C; e += HDI_NT) {
    double v = hdi_inf();
    if (base + e < n) {
      v = p[base + e];
      bad |= !hdi_finite(v);
    }
    sh[e] = v;
  }
  if (bad) flag[blockIdx.y] = 1;  // (every writer stores the same value; the flags were zeroed before the launch)
  __syncthreads();
  bitonic_blocks(sh, HDI_C, HDI_C);
  for (int e = threadIdx.x; e < HDI_C; e += HDI_NT)
    if (base + e < n) p[base + e] = sh[e];
}

// How many of the first d merged outputs of A (la elements) and B (lb) come from A, ties to A.  mid stays in [0, la) and
// d - 1 - mid in [0, lb) for any data, because max(0, d - lb) <= lo <= mid < hi <= min(d, la).
template <typename I>
__device__ __forceinline__ I merge_path(const double* A, I la, const double* B, I lb, I d) {
  I lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One pass: runs of R (a multiple of HDI_TILE) sorted elements of src merge pairwise into dst.  Tile blockIdx.x of
// column blockIdx.y.
__global__ __launch_bounds__(HDI_MT) void hdi_merge(const double* __restrict__ src, double* __restrict__ dst, int64_t n,
                                                    int64_t R) {
  __shared__ double sh[HDI_TILE];
  __shared__ long long cut[2];
  const double* s = src + (int64_t)blockIdx.y * n;
  double* o = dst + (int64_t)blockIdx.y * n;
  const int64_t o0 = (int64_t)blockIdx.x * HDI_TILE;
  const int64_t ps = o0 / (2 * R) * (2 * R);  // start of the pair of runs
  const int64_t la = n - ps < R ? n - ps : R;
  const int64_t lb = n - ps - la < R ? n - ps - la : R;
  const double* A = s + ps;
  const double* B = A + la;
  const int64_t d0 = o0 - ps;
  const int64_t d1 = d0 + HDI_TILE < la + lb ? d0 + HDI_TILE : la + lb;
  if (threadIdx.x < 2) cut[threadIdx.x] = merge_path<int64_t>(A, la, B, lb, threadIdx.x ? d1 : d0);
  __syncthreads();
  const int64_t a0 = cut[0], b0 = d0 - a0;
  const int tot = (int)(d1 - d0);
  // pieces [a0, a0 + na) of A and [b0, b0 + nb) of B; the clamps act on unordered (non-finite) columns only
  int64_t na64 = cut[1] - a0;
  const int64_t amax = la - a0 < tot ? la - a0 : tot;
  na64 = na64 < 0 ? 0 : (na64 > amax ? amax : na64);
  int64_t nb64 = tot - na64;
  if (b0 + nb64 > lb) {
    nb64 = lb - b0;
    na64 = tot - nb64;
  }
  const int na = (int)na64, nb = (int)nb64;
  for (int e = threadIdx.x; e < tot; e += HDI_MT) sh[e] = e < na ? A[a0 + e] : B[b0 + (e - na)];
  __syncthreads();
  const double* SA = sh;
  const double* SB = sh + na;
  int td = threadIdx.x * HDI_ITEMS;
  if (td > tot) td = tot;
  int ai = merge_path<int>(SA, na, SB, nb, td);
  int bi = td - ai;
  double r[HDI_ITEMS];
#pragma unroll
  for (int k = 0; k < HDI_ITEMS; ++k) {
    r[k] = 0.0;
    if (td + k < tot) {
      // ai + bi = td + k < na + nb: one of the two cursors is inside its piece
      const bool take_a = ai < na && (bi >= nb || !(SB[bi] < SA[ai]));
      r[k] = take_a ? SA[ai] : SB[bi];
      ai += take_a ? 1 : 0;
      bi += take_a ? 0 : 1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < HDI_ITEMS; ++k)
    if (td + k < tot) sh[td + k] = r[k];
  __syncthreads();
  for (int e = threadIdx.x; e < tot; e += HDI_MT) o[o0 + e] = sh[e];
}

__device__ __forceinline__ void win_tree(double& bw, long long& bi, double* redw, long long* redi) {
  redw[threadIdx.x] = bw;
  redi[threadIdx.x] = bi;
  __syncthreads();
  for (int h = HDI_MT >> 1; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h &&
        win_less(redw[threadIdx.x + h], redi[threadIdx.x + h], redw[threadIdx.x], redi[threadIdx.x])) {
      redw[threadIdx.x] = redw[threadIdx.x + h];
      redi[threadIdx.x] = redi[threadIdx.x + h];
    }
    __syncthreads();
  }
  bw = redw[0];
  bi = redi[0];
}

// part[(column * n_frac + f) * nblk + blockIdx.x] = the least (w, i) of the window starts [blockIdx.x * HDI_WCH, + HDI_WCH)
__global__ __launch_bounds__(HDI_MT) void hdi_window(const double* __restrict__ cols, int64_t n, int n_frac,
                                                     const long long* __restrict__ Ls, int nblk, WinPart* __restrict__ part) {
  __shared__ double redw[HDI_MT];
  __shared__ long long redi[HDI_MT];
  const int f = blockIdx.y;
  const long long L = Ls[f];
  if (L >= n) return;
  const double* s = cols + (int64_t)blockIdx.z * n;
  const int64_t cnt = n - L, base = (int64_t)blockIdx.x * HDI_WCH;
  double bw = hdi_inf();
  long long bi = INT64_MAX;
  for (int u = 0; u < HDI_WCH / HDI_MT; ++u) {
    const int64_t i = base + threadIdx.x + (int64_t)u * HDI_MT;
    if (i < cnt) {
      const double w = s[i + L] - s[i];
      if (win_less(w, i, bw, bi)) {
        bw = w;
        bi = i;
      }
    }
  }
  win_tree(bw, bi, redw, redi);
  if (threadIdx.x == 0) part[((int64_t)blockIdx.z * n_frac + f) * nblk + blockIdx.x] = WinPart{bw, bi};
}

// the partials of (f = blockIdx.x, column = blockIdx.y) -> out
__global__ __launch_bounds__(HDI_MT) void hdi_window_finish(const double* __restrict__ cols, int64_t n, int64_t mb, int n_frac,
                                                            const long long* __restrict__ Ls, int nblk,
                                                            const WinPart* __restrict__ part, double* __restrict__ out) {
  __shared__ double redw[HDI_MT];
  __shared__ long long redi[HDI_MT];
  const int f = blockIdx.x;
  const int64_t col = blockIdx.y;
  const long long L = Ls[f];
  const double* s = cols + col * n;
  if (L >= n) {
    if (threadIdx.x == 0) {
      out[(int64_t)(2 * f) * mb + col] = s[0];
      out[(int64_t)(2 * f + 1) * mb + col] = s[n - 1];
    }
    return;
  }
  const WinPart* p = part + (col * n_frac + f) * nblk;
  double bw = hdi_inf();
  long long bi = INT64_MAX;
  for (int b = threadIdx.x; b < nblk; b += HDI_MT) {
    const WinPart q = p[b];
    if (win_less(q.w, q.i, bw, bi)) {
      bw = q.w;
      bi = q.i;
    }
  }
  win_tree(bw, bi, redw, redi);
  if (threadIdx.x == 0) {
    if (bi >= n - L) bi = 0;  // (only a column of NaN differences)
    out[(int64_t)(2 * f) * mb + col] = s[bi];
    out[(int64_t)(2 * f + 1) * mb + col] = s[bi + L];
  }
}

}  // namespace

extern "C" {

int gpmi_hdi_columns(gpmi_ctx* c, int64_t n, int64_t m, int64_t row_stride, int64_t col_stride, const double* sample,
                     int n_frac, const int64_t* L, int64_t ws_bytes, double* hdi, int32_t* flag) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, sample && L && hdi && flag, "gpmi_hdi_columns: sample, L, hdi and flag must be non-NULL");
  ARGCHK(c, n >= 2 && n <= HDI_MAX_N, "gpmi_hdi_columns: n out of range (2 .. 2^30)");
  ARGCHK(c, m >= 1 && m <= INT32_MAX, "gpmi_hdi_columns: m out of range (1 .. 2^31 - 1)");
  ARGCHK(c, n_frac >= 1 && n_frac <= 65535, "gpmi_hdi_columns: n_frac out of range (1 .. 65535)");
  ARGCHK(c, ws_bytes >= 0, "gpmi_hdi_columns: ws_bytes must not be negative");
  for (int f = 0; f < n_frac; ++f) ARGCHK(c, L[f] >= 0, "gpmi_hdi_columns: a window length is negative");
  // the two dense layouts; a single column is one contiguous run either way
  const bool by_col = row_stride == 1 && (col_stride >= n || m == 1);
  const bool by_row = !by_col && col_stride == 1 && row_stride >= m;
  ARGCHK(c, by_col || by_row,
         "gpmi_hdi_columns: the strides must be (ld, 1) with ld >= m or (1, ld) with ld >= n, in elements");
  const int64_t ld = by_col ? (m == 1 ? n : col_stride) : row_stride;
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;

  const bool large = n > HDI_C;
  const int nblk = (int)((n + HDI_WCH - 1) / HDI_WCH);
  const size_t cap = ws_bytes ? (size_t)ws_bytes : HDI_DEFAULT_WS;
  const size_t col_bytes = 8 * (size_t)n;
  const size_t per_col = col_bytes * ((by_row ? 1 : 0) + 1 + (large ? 1 : 0)) +
                         (large ? sizeof(WinPart) * (size_t)n_frac * nblk : 0) + 16 * (size_t)n_frac + 4;
  const size_t fixed = kde_align256(8 * (size_t)n_frac) + 6 * 256;  // the window lengths, and the alignment of six regions
  if (cap < fixed + per_col) {
    c->err = "gpmi_hdi_columns: one column of " + std::to_string(n) + " rows needs " + std::to_string(fixed + per_col) +
             " bytes of workspace, more than the cap of " + std::to_string(cap);
    return GPMI_ERR_ARG;
  }
  const int64_t mb_max = std::min<int64_t>(std::min<int64_t>(m, HDI_MAX_BLOCK), (int64_t)((cap - fixed) / per_col));

  // the workspace, carved for the largest (first) block
  const size_t l_bytes = kde_align256(8 * (size_t)n_frac);
  const size_t raw_bytes = by_row ? kde_align256(col_bytes * mb_max) : 0;
  const size_t a_bytes = kde_align256(col_bytes * mb_max);
  const size_t b_bytes = large ? a_bytes : 0;
  const size_t part_bytes = large ? kde_align256(sizeof(WinPart) * (size_t)n_frac * nblk * mb_max) : 0;
  const size_t out_bytes = kde_align256(16 * (size_t)n_frac * mb_max);
  const size_t flag_bytes = kde_align256(4 * (size_t)mb_max);
  if (int rc = st->reserve_work(c, l_bytes + raw_bytes + a_bytes + b_bytes + part_bytes + out_bytes + flag_bytes))
    return rc;
  if (int rc = st->reserve_pinned(c, l_bytes + out_bytes + flag_bytes)) return rc;
  char* w = st->d_work;
  long long* d_L = reinterpret_cast<long long*>(w);
  double* d_raw = reinterpret_cast<double*>(w + l_bytes);
  double* d_a = reinterpret_cast<double*>(w + l_bytes + raw_bytes);
  double* d_b = reinterpret_cast<double*>(w + l_bytes + raw_bytes + a_bytes);
  WinPart* d_part = reinterpret_cast<WinPart*>(w + l_bytes + raw_bytes + a_bytes + b_bytes);
  double* d_out = reinterpret_cast<double*>(w + l_bytes + raw_bytes + a_bytes + b_bytes + part_bytes);
  int* d_flag = reinterpret_cast<int*>(w + l_bytes + raw_bytes + a_bytes + b_bytes + part_bytes + out_bytes);
  char* h_out = st->h_stage + l_bytes;

  std::memcpy(st->h_stage, L, 8 * (size_t)n_frac);
  HIPCHK(c, hipMemcpyAsync(d_L, st->h_stage, 8 * (size_t)n_frac, hipMemcpyHostToDevice, st->stream));

  // slots per column and columns per workgroup of hdi_small
  int P = HDI_PMIN;
  while (P < n && P < HDI_C) P <<= 1;
  const int cpw = P < HDI_PACK ? HDI_PACK / P : 1;

  for (int64_t c0 = 0; c0 < m; c0 += mb_max) {
    const int64_t mb = std::min<int64_t>(mb_max, m - c0);
    // the block as it lies on the host: n rows of mb doubles (by_row), or mb rows of n doubles (by_col)
    const double* src = sample + (by_row ? c0 : c0 * ld);
    double* dst = by_row ? d_raw : d_a;
    const size_t width = 8 * (size_t)(by_row ? mb : n), height = (size_t)(by_row ? n : mb);
    if (height == 1 || (size_t)ld * 8 == width) {
      HIPCHK(c, hipMemcpyAsync(dst, src, width * height, hipMemcpyHostToDevice, st->stream));
    } else {
      HIPCHK(c, hipMemcpy2DAsync(dst, width, src, 8 * (size_t)ld, width, height, hipMemcpyHostToDevice, st->stream));
    }
    if (by_row) {
      hipLaunchKernelGGL(col_transpose, dim3((unsigned)((n + 31) / 32), (unsigned)((mb + 31) / 32)), dim3(256), 0, st->stream,
                         d_raw, d_a, n, mb, n);
      HIPCHK(c, hipGetLastError());
    }
    if (!large) {
      hipLaunchKernelGGL(hdi_small, dim3((unsigned)((mb + cpw - 1) / cpw)), dim3(HDI_NT), 0, st->stream, d_a, (int)n, mb, P, cpw,
                         n_frac, d_L, d_out, d_flag);
      HIPCHK(c, hipGetLastError());
    } else {
      HIPCHK(c, hipMemsetAsync(d_flag, 0, 4 * (size_t)mb, st->stream));
      const unsigned nchunks = (unsigned)((n + HDI_C - 1) / HDI_C), ntiles = (unsigned)((n + HDI_TILE - 1) / HDI_TILE);
      hipLaunchKernelGGL(hdi_chunk_sort, dim3(nchunks, (unsigned)mb), dim3(HDI_NT), 0, st->stream, d_a, n, d_flag);
      HIPCHK(c, hipGetLastError());
      double* cur = d_a;
      double* nxt = d_b;
      for (int64_t R = HDI_C; R < n; R *= 2) {
        hipLaunchKernelGGL(hdi_merge, dim3(ntiles, (unsigned)mb), dim3(HDI_MT), 0, st->stream, cur, nxt, n, R);
        HIPCHK(c, hipGetLastError());
        std::swap(cur, nxt);
      }
      hipLaunchKernelGGL(hdi_window, dim3((unsigned)nblk, (unsigned)n_frac, (unsigned)mb), dim3(HDI_MT), 0, st->stream, cur, n,
                         n_frac, d_L, nblk, d_part);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(hdi_window_finish, dim3((unsigned)n_frac, (unsigned)mb), dim3(HDI_MT), 0, st->stream, cur, n, mb, n_frac,
                         d_L, nblk, d_part, d_out);
      HIPCHK(c, hipGetLastError());
    }
    const size_t ob = 16 * (size_t)n_frac * mb;
    HIPCHK(c, hipMemcpyAsync(h_out, d_out, ob, hipMemcpyDeviceToHost, st->stream));
    HIPCHK(c, hipMemcpyAsync(h_out + out_bytes, d_flag, 4 * (size_t)mb, hipMemcpyDeviceToHost, st->stream));
    HIPCHK(c, hipStreamSynchronize(st->stream));
    for (int r = 0; r < 2 * n_frac; ++r)
      std::memcpy(hdi + (size_t)r * m + c0, h_out + 8 * (size_t)r * mb, 8 * (size_t)mb);
    std::memcpy(flag + c0, h_out + out_bytes, 4 * (size_t)mb);
  }
  return GPMI_OK;
}

}  // extern "C"
