// Column blocks of a panel TRSM beside potrf_diag: the device code shared by the chain launch of the flag-ordered tail
// (potrf_flow.hip: chain_column_kernel) and the fused panel column of the stream-ordered chain (potrf_panel.hip:
// panel_column_kernel).  In both, workgroup 0 runs potrf_diag_body<true> (potrf_diag.h) and counts row block r of the
// inverse in at rows[32 r] (DiagPub); the other workgroups form column block c of X = T invD^T when row block c has landed:
// X_c = sum_{s <= c} T_s invD[c][s]^T needs no other row block (the inverse is lower triangular).
#pragma once
#include "gemm_tiles.h"
#include "potrf_diag.h"

namespace potrf_colblock {

using gemm_tiles::flow_ld;
using gemm_tiles::FLOW_SPIN_LIMIT;
constexpr int NB = GPMI_NB;

// The counters only grow (a factorisation of the tail zeroes them first; the stream-ordered chain never does, and its
// targets wrap with them): "reached" is a comparison of the difference.
__device__ __forceinline__ bool flag_reached(int seen, int target) { return (int)((unsigned)seen - (unsigned)target) >= 0; }

// Every wave that is about to load row block `row` of the inverse calls this: a bounded poll of the row block's counter
// (give_up() after FLOW_SPIN_LIMIT polls, and as soon as somebody else has set the abort word), then the wave's OWN
// agent-scope acquire - the loads that follow must not rest on another wave's invalidation being CU-wide.
template <class GiveUp>
__device__ __forceinline__ void wait_inv_row(const int* rowflag, int target, const int* abortw, GiveUp&& give_up) {
  int spins = 0;
  while (!flag_reached(flow_ld(rowflag), target)) {
    __builtin_amdgcn_s_sleep(2);
    if ((++spins & 63) == 0 && flow_ld(abortw)) break;
    if (spins > FLOW_SPIN_LIMIT) {
      give_up();
      break;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// One wave: column block `row` (16 columns) of a 16-row strip of X = T invD^T, in two halves so that a caller can
// request the next block's operands before the MFMAs of the current one.
// load_inv_rowblock: the B operands - lane (fr, fk): inv[16 row + fr][16 s + 4 fk .. + 3] of the slabs s <= row (`inv`: the
// inverse, row pitch `pitch` - global memory, or a copy in LDS).
// colblock_sums: a_slab(s) returns the wave's A operand of slab s - lane (fr, fk): T[fr][16 s + 4 fk .. + 3] of the strip.
// The sums are those of the register-staged TRSM body (gemm_tiles::staged_tile<..., BTRI>), bit for bit:
// k = 16 s + 4 fk + q at MFMA step q of slab s, slabs in ascending order, the slabs beyond the column block (zeros
// of the lower-triangular inverse) skipped.  Returns the block in the D layout: lane (fr, fk) element r =
// X[fk + 4 r][16 row + fr].
__device__ __forceinline__ void load_inv_rowblock(const double* inv, int pitch, int row, int fr, int fk,
                                                  d4_t (&b)[NB / 16]) {
  const double* brow = inv + (int64_t)(16 * row + fr) * pitch + 4 * fk;
#pragma unroll
  for (int s = 0; s < NB / 16; ++s)
    if (s <= row) b[s] = *reinterpret_cast<const d4_t*>(brow + 16 * s);
}
template <class ASlab>
__device__ __forceinline__ d4_t colblock_sums(int row, ASlab&& a_slab, const d4_t (&b)[NB / 16]) {
  d4_t x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < NB / 16; ++s)
    if (s <= row) {
      const d4_t a = a_slab(s);
#pragma unroll
      for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[s][q], x, 0, 0, 0);
    }
  return x;
}

}  // namespace potrf_colblock
