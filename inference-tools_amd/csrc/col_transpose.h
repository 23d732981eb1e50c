// The transpose that brings a C-order block of columns to one contiguous run per column, shared by the entry points
// that walk the columns of a sample (hdi.hip: gpmi_hdi_columns, acf.hip: gpmi_acf_columns).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// raw (n x mb, row-major) -> cols (mb runs of n, ldo >= n elements apart): 32 x 32 tiles through LDS, both sides
// coalesced; rows of tiles on grid.x, columns of tiles on grid.y
static __global__ __launch_bounds__(256) void col_transpose(const double* __restrict__ raw, double* __restrict__ cols,
                                                            int64_t n, int64_t mb, int64_t ldo) {
  __shared__ double tile[32][33];
  const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int u = ty; u < 32; u += 8) {
    const int64_t r = r0 + u, c = c0 + tx;
    if (r < n && c < mb) tile[u][tx] = raw[r * mb + c];
  }
  __syncthreads();
  for (int u = ty; u < 32; u += 8) {
    const int64_t c = c0 + u, r = r0 + tx;
    if (r < n && c < mb) cols[c * ldo + r] = tile[tx][u];
  }
}
