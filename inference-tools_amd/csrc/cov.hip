// The covariance matrix of a tall sample: numpy.cov(sample.T) for n rows and m <= 512 columns, the device side of
// `sample_covariance` and of PcaChain's direction updates (reference inference/mcmc/pca.py:98-108), with the C-ABI entry
// point gpmi_cov_columns of include/gpmi.h.  Two passes over the sample, which is copied to the device as it lies on the
// host (C order compacted to n x m, or m runs of n): the column means, then S = y^T y of the centred y = x - mean on the
// fp64 matrix cores - a tall-skinny SYRK in which the rows, not the tiles, fill the machine.
//
// Both passes cut the rows into chunks of R = GPMI_COV_CHUNK_ROWS and walk a chunk in slabs of COV_KB = 32 rows x 64
// columns, staged in LDS as [row][column] whatever the layout in memory (cov_load / cov_store):
//   cov_colsum   a workgroup per chunk and 64 columns.  Thread (g, c) adds the rows g, g + 4, g + 8, ... of the chunk's
//                column c in ascending order; the four are added as ((p0 + p1) + p2) + p3 and written as the chunk's sum,
//                with the chunk's mark of a NaN or an infinity.
//   cov_mean     a thread per column adds the chunk sums in ascending order, divides by n, and ors the marks into the flag.
//   cov_tiles    a workgroup per chunk and pair (ti <= tj) of 64-column tiles of the upper triangle.  The slabs of the two
//                tiles are centred on their way into LDS (rows from n on and columns from m on are zeros); wave (wr, wc)
//                owns the 32 x 32 quadrant as 2 x 2 v_mfma_f64_16x16x4_f64 accumulators and per four rows reads two A and
//                two B fragments for four MFMAs.  The next slab is in registers while the MFMAs of this one run.  The
//                chunk's 64 x 64 partial tile goes to the workspace.
//   cov_reduce   a thread per element of a tile pair adds the partial tiles to the running sum in ascending chunk order; after
//                the last chunk the upper triangle is scaled by fl(1 / (n - 1)) and written with its mirror image.
// An element (i, j) is therefore one chain of MFMA accumulations over the rows of a chunk, four rows at a time from the
// chunk's first row, and one chain of additions over the chunks: the order is fixed by n alone, whatever the other columns,
// the position of i and j, the layout or the workspace cap (chunks are walked in groups that fit it; the running sum
// carries on where the group before stopped).  No atomics.
#include "api_internal.h"
#include "kde_state.h"

namespace {

typedef double cov_d4 __attribute__((ext_vector_type(4)));

constexpr int COV_NT = 256;
constexpr int COV_R = GPMI_COV_CHUNK_ROWS;
constexpr int COV_KB = 32;                       // rows of a slab
constexpr int COV_TILE = 64;                     // columns of a tile
constexpr int COV_LD = 81;                       // LDS row pitch in doubles: odd, so that a lane per row (the column-
                                                 // contiguous layout's stores) and a lane per column both spread over the banks
constexpr int COV_PER = COV_KB * COV_TILE / COV_NT;  // slab elements per thread: 8
constexpr int64_t COV_MAX_N = (int64_t)1 << 30;
constexpr int64_t COV_MAX_M = 512;
constexpr size_t COV_DEFAULT_WS = (size_t)1 << 30;
constexpr size_t COV_TILE_BYTES = 8 * (size_t)COV_TILE * COV_TILE;
static_assert(COV_R % COV_KB == 0 && COV_KB % 4 == 0, "a chunk is whole slabs, a slab whole MFMA steps");

__device__ __forceinline__ bool cov_finite(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// Element u of this thread in a slab: (row k, column j) of the slab.  by_row (C order): neighbouring lanes take neighbouring
// columns; otherwise neighbouring rows - either way neighbouring addresses.
__device__ __forceinline__ void cov_elem(int u, bool by_row, int& k, int& j) {
  const int e = (int)threadIdx.x + COV_NT * u;
  if (by_row) {
    j = e & (COV_TILE - 1);
    k = e >> 6;
  } else {
    k = e & (COV_KB - 1);
    j = e >> 5;
  }
}

// The slab of rows [t0, t0 + 32) (below tend) and columns [c0, c0 + 64) (below m) into registers: zeros outside.
// Element (t, c) of the sample is x[t * rs + c * cs].
__device__ __forceinline__ void cov_load(double* r, const double* __restrict__ x, int64_t rs, int64_t cs, bool by_row,
                                         int64_t t0, int64_t tend, int64_t c0, int64_t m, const double* mean) {
#pragma unroll
  for (int u = 0; u < COV_PER; ++u) {
    int k, j;
    cov_elem(u, by_row, k, j);
    const int64_t t = t0 + k, c = c0 + j;
    double v = 0.0;
    if (t < tend && c < m) {
      v = x[t * rs + c * cs];
      if (mean) v -= mean[c];
    }
    r[u] = v;
  }
}

__device__ __forceinline__ void cov_store(double* lds, const double* r, bool by_row) {
#pragma unroll
  for (int u = 0; u < COV_PER; ++u) {
    int k, j;
    cov_elem(u, by_row, k, j);
    lds[k * COV_LD + j] = r[u];
  }
}

// Chunk blockIdx.x, columns [64 blockIdx.y, + 64): psum[chunk * mp + column], pbad likewise.
__global__ __launch_bounds__(COV_NT) void cov_colsum(const double* __restrict__ x, int64_t rs, int64_t cs, int by_row,
                                                     int64_t n, int64_t m, int64_t mp, double* __restrict__ psum,
                                                     int* __restrict__ pbad) {
  __shared__ double slab[COV_KB * COV_LD];
  __shared__ double four[4][COV_TILE];
  __shared__ int marks[4][COV_TILE];
  const int64_t t_first = (int64_t)blockIdx.x * COV_R;
  const int64_t t_end = t_first + COV_R < n ? t_first + COV_R : n;
  const int64_t c0 = (int64_t)blockIdx.y * COV_TILE;
  const int g = threadIdx.x >> 6, cl = threadIdx.x & 63;
  double s = 0.0;
  int bad = 0;
  for (int64_t t0 = t_first; t0 < t_end; t0 += COV_KB) {
    double r[COV_PER];
    cov_load(r, x, rs, cs, by_row, t0, t_end, c0, m, nullptr);
    cov_store(slab, r, by_row);
    __syncthreads();
#pragma unroll
    for (int k = g; k < COV_KB; k += 4) {
      const double v = slab[k * COV_LD + cl];  // (the zeros beyond the sample are finite and add nothing)
      bad |= !cov_finite(v);
      s += v;
    }
    __syncthreads();
  }
  four[g][cl] = s;
  marks[g][cl] = bad;
  __syncthreads();
  if (g == 0) {
    psum[(int64_t)blockIdx.x * mp + c0 + cl] = ((four[0][cl] + four[1][cl]) + four[2][cl]) + four[3][cl];  // (c0 + cl < mp)
    pbad[(int64_t)blockIdx.x * mp + c0 + cl] = marks[0][cl] | marks[1][cl] | marks[2][cl] | marks[3][cl];
  }
}

// One thread per column below mp: the chunk sums in ascending order, the mean, the flag.
__global__ __launch_bounds__(COV_NT) void cov_mean(const double* __restrict__ psum, const int* __restrict__ pbad,
                                                   int64_t nchunk, int64_t mp, int64_t n, double* __restrict__ mean,
                                                   int* __restrict__ flag) {
  const int64_t c = (int64_t)blockIdx.x * COV_NT + threadIdx.x;
  if (c >= mp) return;
  double s = 0.0;
  int b = 0;
#pragma unroll 8
  for (int64_t k = 0; k < nchunk; ++k) {
    s += psum[k * mp + c];
    b |= pbad[k * mp + c];
  }
  mean[c] = s / (double)n;
  flag[c] = b ? 1 : 0;
}

// Chunk chunk0 + blockIdx.x, tile pair blockIdx.y = (ti[blockIdx.y], tj[blockIdx.y]):
// part[(blockIdx.x * npair + blockIdx.y) * 4096 + 64 r + c] = sum over the chunk's rows t of y[t][64 ti + r] y[t][64 tj + c]
__global__ __launch_bounds__(COV_NT) void cov_tiles(const double* __restrict__ x, int64_t rs, int64_t cs, int by_row,
                                                    int64_t n, int64_t m, const double* __restrict__ mean, int64_t chunk0,
                                                    int npair, const int* __restrict__ pair_i,
                                                    const int* __restrict__ pair_j, double* __restrict__ part) {
  __shared__ double sa[COV_KB * COV_LD];
  __shared__ double sb[COV_KB * COV_LD];
  const int ti = pair_i[blockIdx.y], tj = pair_j[blockIdx.y];
  const bool diag = ti == tj;
  const int64_t t_first = (chunk0 + (int64_t)blockIdx.x) * COV_R;
  const int64_t t_end = t_first + COV_R < n ? t_first + COV_R : n;
  const int64_t ca = (int64_t)ti * COV_TILE, cb = (int64_t)tj * COV_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fk = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const double* fa = sa + fk * COV_LD + 32 * wr + fr;               // lane (fr, fk): row 4 q + fk of the slab, column fr
  const double* fb = (diag ? sa : sb) + fk * COV_LD + 32 * wc + fr;  // of the MFMA tile, for both operands

  cov_d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = cov_d4{0.0, 0.0, 0.0, 0.0};

  double ra[COV_PER], rb[COV_PER];
  cov_load(ra, x, rs, cs, by_row, t_first, t_end, ca, m, mean);
  if (!diag) cov_load(rb, x, rs, cs, by_row, t_first, t_end, cb, m, mean);
  for (int64_t t0 = t_first; t0 < t_end; t0 += COV_KB) {
    cov_store(sa, ra, by_row);
    if (!diag) cov_store(sb, rb, by_row);
    __syncthreads();
    if (t0 + COV_KB < t_end) {  // (uniform over the workgroup)
      cov_load(ra, x, rs, cs, by_row, t0 + COV_KB, t_end, ca, m, mean);
      if (!diag) cov_load(rb, x, rs, cs, by_row, t0 + COV_KB, t_end, cb, m, mean);
    }
#pragma unroll
    for (int q = 0; q < COV_KB / 4; ++q) {
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = fa[4 * q * COV_LD + 16 * i];
        b[i] = fb[4 * q * COV_LD + 16 * i];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // accumulator register r of lane (fr, fk): row fk + 4 r, column fr of the 16 x 16 tile
  double* out = part + ((int64_t)blockIdx.x * npair + blockIdx.y) * (COV_TILE * COV_TILE);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(32 * wr + 16 * i + fk + 4 * r) * COV_TILE + 32 * wc + 16 * j + fr] = acc[i][j][r];
}

// Element (blockIdx.x * 256 + threadIdx.x) of tile pair blockIdx.y: run += the group's partial tiles in ascending chunk
// order (run starts at +0 with first != 0); with last != 0 the upper triangle goes to cov, scaled, with its mirror image.
__global__ __launch_bounds__(COV_NT) void cov_reduce(const double* __restrict__ part, int64_t nchunks, int npair,
                                                     const int* __restrict__ pair_i, const int* __restrict__ pair_j,
                                                     double* __restrict__ run, int first, int last, double rinv, int64_t m,
                                                     double* __restrict__ cov) {
  const int e = (int)blockIdx.x * COV_NT + (int)threadIdx.x;  // < 4096
  const int64_t at = (int64_t)blockIdx.y * (COV_TILE * COV_TILE) + e;
  double s = first ? 0.0 : run[at];
#pragma unroll 8
  for (int64_t k = 0; k < nchunks; ++k) s += part[k * npair * (int64_t)(COV_TILE * COV_TILE) + at];
  run[at] = s;
  if (!last) return;
  const int64_t i = (int64_t)pair_i[blockIdx.y] * COV_TILE + (e >> 6), j = (int64_t)pair_j[blockIdx.y] * COV_TILE + (e & 63);
  if (i > j || j >= m) return;  // (i <= j < m)
  const double v = s * rinv;
  cov[i * m + j] = v;
  cov[j * m + i] = v;
}

}  // namespace

extern "C" {

int gpmi_cov_columns(gpmi_ctx* c, int64_t n, int64_t m, int64_t row_stride, int64_t col_stride, const double* sample,
                     int64_t ws_bytes, double* mean, double* cov, int32_t* flag) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, sample && mean && cov && flag, "gpmi_cov_columns: sample, mean, cov and flag must be non-NULL");
  ARGCHK(c, n >= 2 && n <= COV_MAX_N, "gpmi_cov_columns: n out of range (2 .. 2^30)");
  ARGCHK(c, m >= 1 && m <= COV_MAX_M, "gpmi_cov_columns: m out of range (1 .. 512)");
  ARGCHK(c, ws_bytes >= 0, "gpmi_cov_columns: ws_bytes must not be negative");
  // the two dense layouts; a single column is one contiguous run either way
  const bool by_col = row_stride == 1 && (col_stride >= n || m == 1);
  const bool by_row = !by_col && col_stride == 1 && row_stride >= m;
  ARGCHK(c, by_col || by_row,
         "gpmi_cov_columns: the strides must be (ld, 1) with ld >= m or (1, ld) with ld >= n, in elements");
  const int64_t ld = by_col ? (m == 1 ? n : col_stride) : row_stride;
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;

  const int64_t nchunk = (n + COV_R - 1) / COV_R;
  const int64_t nt = (m + COV_TILE - 1) / COV_TILE, mp = nt * COV_TILE;
  const int npair = (int)(nt * (nt + 1) / 2);
  const size_t cap = ws_bytes ? (size_t)ws_bytes : COV_DEFAULT_WS;
  const size_t group_bytes = COV_TILE_BYTES * (size_t)npair;  // the partial tiles of one chunk
  if (cap < group_bytes) {
    c->err = "gpmi_cov_columns: the partial tiles of one chunk of rows of " + std::to_string(m) + " columns need " +
             std::to_string(group_bytes) + " bytes of workspace, more than the cap of " + std::to_string(cap);
    return GPMI_ERR_ARG;
  }
  const int64_t gmax = std::min<int64_t>(nchunk, (int64_t)(cap / group_bytes));  // chunks per group

  // the workspace: the sample, the chunk sums and marks, the means and flags, the covariance, the running tiles, the pair
  // lists and the partial tiles of one group
  const size_t x_b = kde_align256(8 * (size_t)n * (size_t)m);
  const size_t ps_b = kde_align256(8 * (size_t)nchunk * (size_t)mp), pb_b = kde_align256(4 * (size_t)nchunk * (size_t)mp);
  const size_t mean_b = kde_align256(8 * (size_t)mp), flag_b = kde_align256(4 * (size_t)mp);
  const size_t cov_b = kde_align256(8 * (size_t)m * (size_t)m);
  const size_t run_b = kde_align256(group_bytes), pair_b = kde_align256(4 * (size_t)npair);
  const size_t part_b = kde_align256(group_bytes * (size_t)gmax);
  const size_t res_b = mean_b + flag_b + cov_b;  // one run, copied back together
  if (int rc = st->reserve_work(c, x_b + ps_b + pb_b + res_b + run_b + 2 * pair_b + part_b))
    return rc;
  if (int rc = st->reserve_pinned(c, std::max(res_b, 2 * pair_b))) return rc;
  char* w = st->d_work;
  double* d_x = reinterpret_cast<double*>(w);
  double* d_ps = reinterpret_cast<double*>(w + x_b);
  int* d_pb = reinterpret_cast<int*>(w + x_b + ps_b);
  char* d_res = w + x_b + ps_b + pb_b;
  double* d_mean = reinterpret_cast<double*>(d_res);
  int* d_flag = reinterpret_cast<int*>(d_res + mean_b);
  double* d_cov = reinterpret_cast<double*>(d_res + mean_b + flag_b);
  double* d_run = reinterpret_cast<double*>(d_res + res_b);
  int* d_pi = reinterpret_cast<int*>(d_res + res_b + run_b);
  int* d_pj = reinterpret_cast<int*>(d_res + res_b + run_b + pair_b);
  double* d_part = reinterpret_cast<double*>(d_res + res_b + run_b + 2 * pair_b);

  // the pairs of the upper triangle, row by row
  int* h_pi = reinterpret_cast<int*>(st->h_stage.get());
  int* h_pj = reinterpret_cast<int*>(st->h_stage + pair_b);
  int k = 0;
  for (int i = 0; i < (int)nt; ++i)
    for (int j = i; j < (int)nt; ++j) {
      h_pi[k] = i;
      h_pj[k++] = j;
    }
  HIPCHK(c, hipMemcpyAsync(d_pi, h_pi, pair_b + 4 * (size_t)npair, hipMemcpyHostToDevice, st->stream));

  // the sample as it lies on the host, without its padding: n rows of m doubles (by_row), or m runs of n (by_col)
  int64_t rs, cs;
  if (by_row) {
    const size_t width = 8 * (size_t)m;
    if (ld == m) {
      HIPCHK(c, hipMemcpyAsync(d_x, sample, width * (size_t)n, hipMemcpyHostToDevice, st->stream));
    } else {
      HIPCHK(c, hipMemcpy2DAsync(d_x, width, sample, 8 * (size_t)ld, width, (size_t)n, hipMemcpyHostToDevice, st->stream));
    }
    rs = m;
    cs = 1;
  } else {
    const size_t width = 8 * (size_t)n;
    if (ld == n || m == 1) {
      HIPCHK(c, hipMemcpyAsync(d_x, sample, width * (size_t)m, hipMemcpyHostToDevice, st->stream));
    } else {
      HIPCHK(c, hipMemcpy2DAsync(d_x, width, sample, 8 * (size_t)ld, width, (size_t)m, hipMemcpyHostToDevice, st->stream));
    }
    rs = 1;
    cs = n;
  }
  // (the pinned pair lists must have left before the results land in the same staging buffer: the copies below are
  // ordered behind this one on the stream)

  {
    // (bytes: the sample is read twice; flops: the tile pairs computed, both triangles of a diagonal tile included)
    ProfScope ps(c, st->stream, GPMI_PROF_COV, 2.0 * (double)n * COV_TILE * COV_TILE * npair, 16.0 * (double)n * (double)m);
    hipLaunchKernelGGL(cov_colsum, dim3((unsigned)nchunk, (unsigned)nt), dim3(COV_NT), 0, st->stream, d_x, rs, cs, by_row ? 1 : 0,
                       n, m, mp, d_ps, d_pb);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(cov_mean, dim3((unsigned)((mp + COV_NT - 1) / COV_NT)), dim3(COV_NT), 0, st->stream, d_ps, d_pb, nchunk, mp,
                       n, d_mean, d_flag);
    HIPCHK(c, hipGetLastError());
    const double rinv = 1.0 / (double)(n - 1);
    for (int64_t c0 = 0; c0 < nchunk; c0 += gmax) {
      const int64_t g = std::min<int64_t>(gmax, nchunk - c0);
      hipLaunchKernelGGL(cov_tiles, dim3((unsigned)g, (unsigned)npair), dim3(COV_NT), 0, st->stream, d_x, rs, cs, by_row ? 1 : 0, n,
                         m, d_mean, c0, npair, d_pi, d_pj, d_part);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(cov_reduce, dim3(COV_TILE * COV_TILE / COV_NT, (unsigned)npair), dim3(COV_NT), 0, st->stream, d_part, g,
                         npair, d_pi, d_pj, d_run, c0 == 0 ? 1 : 0, c0 + g >= nchunk ? 1 : 0, rinv, m, d_cov);
      HIPCHK(c, hipGetLastError());
    }
  }
  HIPCHK(c, hipMemcpyAsync(st->h_stage, d_res, res_b, hipMemcpyDeviceToHost, st->stream));
  HIPCHK(c, hipStreamSynchronize(st->stream));
  std::memcpy(mean, st->h_stage, 8 * (size_t)m);
  std::memcpy(flag, st->h_stage + mean_b, 4 * (size_t)m);
  std::memcpy(cov, st->h_stage + mean_b + flag_b, 8 * (size_t)m * (size_t)m);
  return GPMI_OK;
}

}  // extern "C"
