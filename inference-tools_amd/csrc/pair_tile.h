// The 64 x 64 pair tile the covariance builders (kbuild.hip) and the contractions of the sparse model (sparse.hip) share:
// 256 threads, two 64-point panels staged in LDS as [dim][point], a 4 x 4 block of point pairs per thread,
// s = sum_k 1/2 dx_k^2 / l_k^2 over the dimensions in ascending order, the covariance function and its profiles (kfun.h)
// in two halves of eight elements, and the column reduction of the kernels that differentiate by a point.  Every kernel
// forms s and the profiles here, so a pair of points has the same bits in all of them; the reductions have a fixed order.
// Device code only; internal.
#pragma once
#include "gpmi_internal.h"
#include "kfun.h"

namespace pair_tile {

constexpr int KT = 64;   // tile edge: points per panel
constexpr int NT = 256;  // threads: thread tid owns rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 of the tile
constexpr int SLOTS = 4;  // (dimension, weight array) column sums per barrier of reduce_columns

__device__ __forceinline__ int thread_row(int tid) { return tid >> 4; }  // ty
__device__ __forceinline__ int thread_col(int tid) { return tid & 15; }  // tx

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// block-wide sum (256 threads), the same value in every thread
__device__ inline double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// f(idx, pt, k) for every (point, dimension) of a panel, idx = pt * d + k strided over the workgroup: the order in which a
// row-major n x d array of points is read and written with consecutive threads on consecutive addresses
template <class F>
__device__ __forceinline__ void for_each_coordinate(int d, F&& f) {
  for (int idx = threadIdx.x; idx < KT * d; idx += NT) {
    const int pt = idx / d, k = idx - pt * d;
    f(idx, pt, k);
  }
}

// coordinate k of point i0 + pt of X (n x d) into the panel s ([dim][point]); zeros at and beyond n
__device__ __forceinline__ void stage_coordinate(double* s, const double* __restrict__ X, int64_t i0, int64_t n, int d, int pt,
                                                 int k) {
  const int64_t gi = i0 + pt;
  s[k * KT + pt] = (gi < n) ? X[gi * d + k] : 0.0;
}

// one panel, or the row and the column panel in one loop.  The caller places the barrier.
__device__ __forceinline__ void stage_panel(double* s, const double* __restrict__ X, int64_t i0, int64_t n, int d) {
  for_each_coordinate(d, [&](int, int pt, int k) { stage_coordinate(s, X, i0, n, d, pt, k); });
}
__device__ __forceinline__ void stage_panels(double* su, const double* __restrict__ U, int64_t i0, int64_t nu, double* sv,
                                             const double* __restrict__ V, int64_t j0, int64_t nv, int d) {
  for_each_coordinate(d, [&](int, int pt, int k) {
    stage_coordinate(su, U, i0, nu, d, pt, k);
    stage_coordinate(sv, V, j0, nv, d, pt, k);
  });
}

// s[r][c] = sum_k 1/2 (u_rk - v_ck)^2 / l_k^2 of the thread's block: distances_k / l_k^2 accumulated (covariance.py:254),
// one fma per dimension in ascending k - every result's bits depend on this chain
__device__ __forceinline__ void accumulate_s(const double* inv_l2, int d, const double* su, const double* sv, int ty, int tx,
                                             double (&s)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) s[r][c] = 0.0;
  for (int k = 0; k < d; ++k) {
    const double il2 = inv_l2[k];
    double ur[4], vc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ur[r] = su[k * KT + ty * 4 + r];
#pragma unroll
    for (int c = 0; c < 4; ++c) vc[c] = sv[k * KT + tx * 4 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double dx = ur[r] - vc[c];
        s[r][c] = fma(0.5 * dx * dx, il2, s[r][c]);
      }
  }
}

// The Periodic kernel's s = sum_k w_k / l_k^2 (GPMI_KERNEL_PER) of rows r0 .. r0 + ROWS - 1 of the thread's block, into the
// ROWS x 4 elements of s8: per dimension a uniform branch between SquaredExponential's term w_k = 1/2 dx_k^2 (the fma of
// accumulate_s) and the warped w_k = 2 sin^2(pi dx_k / p_k), whose sin^2 goes through kmath::sinpi_sq ROWS x 4 elements
// in lockstep.  Which dimensions are periodic is one bit test of the kernel's mask per dimension, and 1 / p_j sits behind
// the d inverse squares (gpmi_internal.h: KParams) - scalar registers, no table in LDS (at d = 56 .. 64 the two panels
// leave no room for one).  dx -> -dx gives the same bits (rint and |.| are even), so K is symmetric bit for bit; dx = 0
// gives w = 0 exactly.
template <int ROWS>
__device__ __forceinline__ void accumulate_s_periodic(const KParams& p, int d, const double* su, const double* sv, int ty,
                                                      int tx, int r0, double (&s8)[ROWS * 4]) {
#pragma unroll
  for (int i = 0; i < ROWS * 4; ++i) s8[i] = 0.0;
  const unsigned mask_lo = __builtin_amdgcn_readfirstlane((unsigned)p.per_mask);
  const unsigned mask_hi = __builtin_amdgcn_readfirstlane((unsigned)(p.per_mask >> 32));
  const unsigned long long mask = ((unsigned long long)mask_hi << 32) | mask_lo;
  int cursor = 0;
  for (int k = 0; k < d; ++k) {
    const double il2 = p.inv_l2[k];
    double ur[ROWS], vc[4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) ur[r] = su[k * KT + ty * 4 + r0 + r];
#pragma unroll
    for (int c = 0; c < 4; ++c) vc[c] = sv[k * KT + tx * 4 + c];
    if (!((mask >> k) & 1ull)) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double dx = ur[r] - vc[c];
          s8[4 * r + c] = fma(0.5 * dx * dx, il2, s8[4 * r + c]);
        }
    } else {
      const double ip = p.inv_l2[d + cursor++];
      double u[ROWS * 4], q[ROWS * 4];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) u[4 * r + c] = (ur[r] - vc[c]) * ip;
      kmath::sinpi_sq(u, q);
#pragma unroll
      for (int i = 0; i < ROWS * 4; ++i) s8[i] = fma(2.0 * q[i], il2, s8[i]);
    }
  }
}

// The covariance function of the block in two halves of eight elements (rows 2h, 2h + 1): 16 at once cost occupancy, 8
// already amortise the constants.  PROFILES: f(r, c, C, g, h) with the value and derivative profiles (kprofiles);
// otherwise f(r, c, C) with kfun<KERNEL> alone (which also serves the kinds KFUN_M32_G / KFUN_M52_G).  f may overwrite
// s[r][c]: a half is read before its elements are handed out.
template <int KERNEL, bool PROFILES, class F>
__device__ __forceinline__ void for_each_profile(const KParams& p, const double (&s)[4][4], F&& f) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    double s8[8], C8[8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) s8[4 * r + c] = s[2 * h + r][c];
    if constexpr (PROFILES) {
      double g8[8], h8[8];
      kprofiles<KERNEL>(p, s8, C8, g8, h8);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) f(2 * h + r, c, C8[4 * r + c], g8[4 * r + c], h8[4 * r + c]);
    } else {
      kfun<KERNEL>(p, s8, C8);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) f(2 * h + r, c, C8[4 * r + c]);
    }
  }
}

// The column reduction of the kernels that differentiate by the column point v_j.  For each of the first nw <= NW weight
// arrays and every dimension k,
//   acc[a][k][j] += sum_i w[a][i][j] (v_jk - u_ik)     over the 64 rows of the tile:
// the thread's four rows by fma in ascending r, two xor shuffles over the four lanes of a wave that own the column, the
// four waves through LDS and a fixed tree into the [d][64] accumulator that one thread per element owns.  SLOTS
// (dimension, array) sums go through the slab per barrier - four dimensions of one array or two of two - and the slab
// red ([2][SLOTS][4 waves][64]) is double-buffered: the other half is written only behind the next barrier, `chunk`
// counts the barriers across the tiles of a run.  A slot's sum does not depend on nw.  The difference is formed from
// the staged coordinates: nothing is divided by a distance, coincident points contribute exact zeros.
template <int NW>
__device__ __forceinline__ void reduce_columns(const double* su, const double* sv, int d, int ty, int tx,
                                               const double (&w)[NW][4][4], int nw, double* const (&acc)[NW], double* red,
                                               int& chunk) {
  static_assert(NW == 1 || NW == 2, "reduce_columns: one or two weight arrays");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool two = NW == 2 && nw == 2;
  const int dims = two ? SLOTS / 2 : SLOTS;  // dimensions per barrier
  for (int k0 = 0; k0 < d; k0 += dims, ++chunk) {
    double* buf = red + (chunk & 1) * (SLOTS * 4 * KT);
    for (int kk = 0; kk < dims && k0 + kk < d; ++kk) {
      const int k = k0 + kk;
      double ur[4], col[NW][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ur[r] = su[k * KT + ty * 4 + r];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double vc = sv[k * KT + tx * 4 + c];
        double a[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) a[j] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double dx = vc - ur[r];
#pragma unroll
          for (int j = 0; j < NW; ++j) a[j] = fma(w[j][r][c], dx, a[j]);
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          if (j == 0 || two) {
            a[j] += __shfl_xor(a[j], 16, 64);
            a[j] += __shfl_xor(a[j], 32, 64);
          }
          col[j][c] = a[j];
        }
      }
      if (lane < 16) {
        const int slot = two ? 2 * kk : kk;
#pragma unroll
        for (int j = 0; j < NW; ++j)
          if (j == 0 || two) {
#pragma unroll
            for (int c = 0; c < 4; ++c) buf[((slot + j) * 4 + wave) * KT + tx * 4 + c] = col[j][c];
          }
      }
    }
    __syncthreads();  // (one barrier per chunk)
    const int slot = tid >> 6;
    const int k = k0 + (two ? slot >> 1 : slot);
    double* a = (two && (slot & 1)) ? acc[NW - 1] : acc[0];
    if (k < d)
      a[k * KT + lane] += (buf[(slot * 4 + 0) * KT + lane] + buf[(slot * 4 + 1) * KT + lane]) +
                          (buf[(slot * 4 + 2) * KT + lane] + buf[(slot * 4 + 3) * KT + lane]);
  }
}

// out[a][(row0 + j) * d + k] = scale[a] / l_k^2 * acc[a][k][j] for the first nw arrays: the accumulators of
// reduce_columns, written point-major.  The caller places the barrier behind the last reduce_columns.
template <int NW>
__device__ __forceinline__ void write_columns(const double* inv_l2, int d, double* const (&acc)[NW], int nw,
                                              const double (&scale)[NW], int64_t row0, double* const (&out)[NW]) {
  for_each_coordinate(d, [&](int, int pt, int k) {
    const int64_t o = (row0 + pt) * d + k;
#pragma unroll
    for (int j = 0; j < NW; ++j)
      if (j < nw) out[j][o] = scale[j] * inv_l2[k] * acc[j][k * KT + pt];
  });
}

// dynamic LDS of a kernel with two panels and NW accumulators behind reduce_columns
constexpr size_t column_lds_bytes(int d, int nw_max) { return sizeof(double) * ((size_t)(2 + nw_max) * d + 2 * SLOTS * 4) * KT; }

}  // namespace pair_tile
