// One tile column of the stream-ordered panel chain in ONE launch: potrf_diag of tile (k, k) and the panel TRSM of the
// tiles below it (potrf.hip: factor_panel; numpy.linalg.cholesky at regression.py:241, 537, 555).
//
// As two launches the TRSM could not start before the whole inverse of the diagonal block was stored, and started from
// scratch behind the kernel boundary: its operand tiles fetched only then, all of its MFMAs behind the last elimination.
// Here the flag-ordered tail's treatment of its one tile (potrf_flow.hip: chain_column_kernel) is given to the whole column:
//   workgroup 0       potrf_diag (potrf_diag.h, PUB build): every byte of the inverse stored write-through, row block r
//                     counted in at flags[PANEL_FL_INVROW + 32 r] by the four inverse waves once their stores are acknowledged
//   workgroups 1..W   the 128-row tiles T(i, k), i > k, dealt in a fixed strided order (worker w: i = k + 1 + w, + W, ...).
//                     Wave r owns the rows 16 r .. 16 r + 15 of the tile for the whole product: it fetches them into
//                     registers at once - under the elimination -, forms column block c of X = T invD^T when row block c
//                     of the inverse is published (wave c brings the row block into the workgroup's LDS), and stores it
//                     over its own rows of T (nobody else reads or writes them).  After a worker's first tile the
//                     inverse is complete, in LDS, and nothing waits.
// Behind potrf_diag's last elimination there is left, for the resident workers: the last row block of the inverse, the
// hand-off, 32 MFMAs per wave and the store: 6 - 7 us.  A tile beyond the resident set costs its CU 11 us (8.6 of MFMAs).
// The sums are those of gemm_tiles::staged_tile<..., BTRI>, i.e. of the generic TRSM launch at either tile height
// (potrf_colblock.h): the factor, the inverses, the log-determinant and info are bit-identical to the two-launch form
// (GPMI_PANEL_FUSED=0).
//
// Flags: a block of ints the lane owns (Lane::panel_flags), zeroed once at its allocation and never again - the counters
// are monotone: launch number `seq` of the lane (Lane::panel_seq) finds DIAG_INVERSE * seq in every row counter and waits for
// DIAG_INVERSE * (seq + 1).  The launches of a lane are ordered by its streams and events (potrf_lower), so a row
// counter never runs ahead of the launch that reads it.  Workgroup 0 publishes whatever the pivots were - a diagonal
// block that is not positive definite reports through info as always and its workers do not wait for it any longer.
// Deadlock-free with any number of resident workgroups: workgroup 0 is dispatched first and waits for nobody in the
// launch; a worker waits for workgroup 0 only, never for another worker.  Every poll is bounded (FLOW_SPIN_LIMIT): a
// time-out sets the abort word and info = GPMI_INFO_FLOW_TIMEOUT, the host reports GPMI_ERR_INTERNAL, and a handle with
// GPMI_OPT_NO_FLOW set (what the Python layer repeats such a call with) takes the two-launch form.
#include <cstdlib>

#include "gpmi_internal.h"
#include "potrf_colblock.h"
#include "potrf_diag.h"

namespace {

constexpr int NB = GPMI_NB;
constexpr int INV_PITCH = NB + 6;  // the worker's LDS copy of the inverse
using gemm_tiles::flow_ld;

struct PanelColArgs {
  double* Akk;   // tile (k, k); the tiles T(i, k) follow from ld
  double* invD;  // inverse of diagonal block k
  int64_t ld;
  int* info;
  int col0;
  unsigned long long* dbg;    // potrf_diag's 24-word stamp slot (GPMI_CHAIN_TRACE) or nullptr
  unsigned long long* stamp;  // the workers' stamp slot (start of worker 0, last end per XCD) or nullptr
  int* flags;                 // Lane::panel_flags
  unsigned seq;               // launch number of the lane
  int below;                  // tiles below the diagonal block
};

__global__ __launch_bounds__(potrf_diag::DIAG_THREADS) void panel_column_kernel(PanelColArgs g) {
  // (static LDS of every workgroup: one workgroup per CU - which is why a worker owns whole tiles with its 8 waves)
  __shared__ potrf_diag::DiagShared sh;
  if (blockIdx.x == 0) {
    potrf_diag::DiagPub pub;
    pub.rows = g.flags + GPMI_PANEL_FL_INVROW;
    pub.base = (int)(potrf_diag::DIAG_INVERSE * g.seq);
    potrf_diag::potrf_diag_body<true>(g.Akk, g.ld, g.invD, g.info, g.col0, g.dbg, sh, pub);
    return;
  }
  // ------------------------------------------------------------------------------------------------ a worker
  const int w = (int)blockIdx.x - 1, W = (int)gridDim.x - 1;
  const int tid = threadIdx.x, lane = tid & 63, r = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const int fr = lane & 15, fk = lane >> 4;
  const int* rows = g.flags + GPMI_PANEL_FL_INVROW;
  int* abortw = g.flags + GPMI_PANEL_FL_ABORT;
  auto give_up = [&]() {
    if (lane == 0) {
      __hip_atomic_store(abortw, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (g.info) atomicCAS(g.info, 0, GPMI_INFO_FLOW_TIMEOUT);
    }
  };
  if (g.stamp && w == 0 && tid == 0) g.stamp[0] = __builtin_amdgcn_s_memrealtime();
  // the worker's LDS, laid over the block image of workgroup 0's role: a copy of the inverse (row pitch INV_PITCH: the
  // 16-byte reads of a 16-lane row fall into different banks), and the number of its row blocks that are there
  double* inv_lds = reinterpret_cast<double*>(&sh);
  int* seen = reinterpret_cast<int*>(inv_lds + NB * INV_PITCH);
  static_assert(sizeof(double) * NB * INV_PITCH + sizeof(int) <= sizeof(potrf_diag::DiagShared), "the worker's LDS");
  if (tid == 0) *seen = 0;
  __syncthreads();
  const int row_target = (int)(potrf_diag::DIAG_INVERSE * (g.seq + 1u));
  // The wave's 16 rows of a tile T: lane (fr, fk) holds T[16 r + fr][16 s + 4 fk .. + 3] of every slab s (written by
  // launches before this one: visible since the kernel boundary).  The first tile's are requested now and arrive under
  // the elimination - and so are the second tile's: every later tile is fetched while the tile before it is worked on.
  auto fetch = [&](int i, d4_t (&t)[NB / 16]) {
    const double* trow = g.Akk + (int64_t)(i + 1) * NB * g.ld + (int64_t)(16 * r + fr) * g.ld + 4 * fk;
#pragma unroll
    for (int s = 0; s < NB / 16; ++s) t[s] = *reinterpret_cast<const d4_t*>(trow + 16 * s);
  };
  // X over T, block by block: the rows are this wave's alone and all of them are in its registers
  auto store_block = [&](int i, int c, const d4_t& x) {
    double* out = g.Akk + (int64_t)(i + 1) * NB * g.ld + (int64_t)(16 * r + fk) * g.ld + fr;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(int64_t)4 * q * g.ld + 16 * c] = x[q];
  };
  d4_t a[NB / 16], an[NB / 16];
  fetch(w, a);  // (w < below: the launch has no more workers than tiles)
  if (w + W < g.below) fetch(w + W, an);
  // ---- the first tile, beside potrf_diag
#pragma unroll
  for (int c = 0; c < NB / 16; ++c) {
    // Row block c of the inverse comes from global memory ONCE per workgroup: wave c polls its counter, acquires,
    // loads the row block and hands it to the other waves through LDS (with every wave of a full-chip launch polling
    // and loading for itself, a thousand waves read the same 128 KB right behind every publication: 77 us per column
    // on 127 CUs against 40 as two launches).  Wave c is the only wave that loads what workgroup 0 published, and it
    // acquires for itself (wait_inv_row); the others read LDS.
    d4_t b[NB / 16];
    if (r == c) {
      potrf_colblock::wait_inv_row(rows + 32 * c, row_target, abortw, give_up);
      potrf_colblock::load_inv_rowblock(g.invD, NB, c, fr, fk, b);
      double* brow = inv_lds + (16 * c + fr) * INV_PITCH + 4 * fk;
#pragma unroll
      for (int s = 0; s <= c; ++s) *reinterpret_cast<d4_t*>(brow + 16 * s) = b[s];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own LDS writes are done: the count goes behind them
      if (lane == 0) __hip_atomic_store(seen, c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      int polls = 0;
      while (__hip_atomic_load(seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <= c) {
        __builtin_amdgcn_s_sleep(1);
        if ((++polls & 1023) == 0 && flow_ld(abortw)) break;
        if (polls > (1 << 25)) {  // (longer than the polling wave's own limit)
          give_up();
          break;
        }
      }
      asm volatile("" ::: "memory");
      potrf_colblock::load_inv_rowblock(inv_lds, INV_PITCH, c, fr, fk, b);
    }
    store_block(w, c, potrf_colblock::colblock_sums(c, [&](int s) { return a[s]; }, b));
  }
  // ---- the later tiles: the inverse is complete and in LDS, nothing waits
  if (w + W < g.below) {
    __syncthreads();
    for (int i = w + W; i < g.below; i += W) {
#pragma unroll
      for (int s = 0; s < NB / 16; ++s) a[s] = an[s];
      if (i + W < g.below) fetch(i + W, an);
#pragma unroll
      for (int c = 0; c < NB / 16; ++c) {
        d4_t b[NB / 16];
        potrf_colblock::load_inv_rowblock(inv_lds, INV_PITCH, c, fr, fk, b);
        store_block(i, c, potrf_colblock::colblock_sums(c, [&](int s) { return a[s]; }, b));
        // (left alone, the scheduler requests all 36 slabs of the inverse up front: 193 registers spilled)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  if (g.stamp && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    g.stamp[8 + (__builtin_amdgcn_s_getreg(((4 - 1) << 11) | 20) & 7)] = __builtin_amdgcn_s_memrealtime();
  }
}

}  // namespace

// GPMI_PANEL_FUSED=0 keeps the two-launch form (A/B runs, tests); so does a handle with GPMI_OPT_NO_FLOW set - the schedule
// a call is repeated on after a flag-ordered launch gave up - and a lane without a flag block
bool potrf_panel_fused(gpmi_ctx* c, Lane& lane) {
  static const bool on = [] {
    const char* e = std::getenv("GPMI_PANEL_FUSED");
    return !e || std::atoi(e) != 0;
  }();
  return on && !c->no_flow && lane.panel_flags != nullptr;
}

// potrf_diag of tile (k, k) at Akk and the panel TRSM of the `below` > 0 tiles under it, on stream s, which may use `ncu`
// CUs: one worker per tile up to one per CU beside workgroup 0's (GPMI_PANEL_WORKERS=<W>: test-only clamp, so that the
// loop over several tiles per worker runs at small sizes)
void launch_panel_column(Lane& lane, hipStream_t s, double* Akk, int64_t ld, double* invD, int* info, int col0, int below,
                         int ncu, unsigned long long* dbg, unsigned long long* stamp) {
  static const int clamp = [] {
    const char* e = std::getenv("GPMI_PANEL_WORKERS");
    return e ? std::atoi(e) : 0;
  }();
  int W = ncu - 1 < below ? ncu - 1 : below;
  if (clamp > 0 && W > clamp) W = clamp;
  if (W < 1) W = 1;
  PanelColArgs g{Akk, invD, ld, info, col0, dbg, stamp, lane.panel_flags, lane.panel_seq++, below};
  hipLaunchKernelGGL(panel_column_kernel, dim3(1u + (unsigned)W), dim3(potrf_diag::DIAG_THREADS), 0, s, g);
  launch_potrf_diag_fault(s, Akk, ld);
}
