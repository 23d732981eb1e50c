// Two-dimensional Gaussian kernel-density estimation (KDE2D, reference inference/pdf/kde.py:256-280) on the device, with
// the C-ABI entry points gpmi_kde2d_* of include/gpmi.h.  The quantity everywhere is the raw, untruncated sum over the n
// samples (x_j, y_j) of a point (a, b),
//     S(a, b) = sum_j exp(-((x_j - a) q_x)^2 - ((y_j - b) q_y)^2);
// the caller applies norm.  The exponent is formed with the reference's own roundings (no contraction into fma), so a
// term differs from NumPy's only by the two exponentials' last bits.
//
// Direct sums (gpmi_kde2d_eval, gpmi_kde2d_self).  A workgroup takes 256 points (one per thread) and one of `nsplit`
// ranges of the samples, which it walks in tiles of K2_TILE samples staged in LDS as (x, y) pairs: every thread reads the
// same pair (a broadcast ds_read_b128) and evaluates four pairs in lockstep (kmath::exp_neg<4>) into four accumulators.
// The ranges start at multiples of `per_split`, which depends on n alone, and the finish launch adds a point's range
// partials in range order: a point's value depends neither on the other points of the call nor on their number, and
// there is no atomic.
//
// The object keeps the samples binned: sorted by x, cut into strips of whole tiles, each strip sorted by y, so that a
// tile of 256 consecutive samples covers a small box [xlo, xhi] x [ylo, yhi] (computed on the host at creation).
// gpmi_kde2d_self, where the points are the samples themselves (point block I = sample tile I), skips a tile J whose box
// is further from box I than K2_SKIP allows (see the constant).  The scattered evaluation skips nothing: its terms
// beyond an exponent of -745.2 are exact zeros of exp_neg.
//
// Factorised grid (gpmi_kde2d_grid).  On the grid of an x axis (g_x values a) and a y axis (g_y values b) the term
// factorises, exp(-z_x - z_y) = exp(-z_x) exp(-z_y): the grid is the product E_y E_x^T with E_x[a, j] =
// exp(-((x_j - a) q_x)^2), E_y likewise - (g_x + g_y) n exponentials in place of g_x g_y n.  A workgroup (4 waves) owns
// a 64 x 64 block of the grid and one range of j; per chunk of G_KC samples it forms the two 64 x G_KC factor tiles
// straight into LDS (they never reach HBM) and contracts them with v_mfma_f64_16x16x4 (each wave a 32 x 32 quarter, 2 x 2
// MFMA tiles, operand map of gemm_f64.hip: lane (fr, fk) supplies row / column fr at k = fk).  The LDS rows (one per
// sample, 64 factors) are padded to 80 doubles = 640 bytes: the 16 lanes of one k read 128 consecutive bytes and the next
// k starts 640 = 2 x 256 + 128 bytes on, in the other half of the 256-byte bank row, so each 32-lane half of a
// ds_read_b64 is conflict-free (unpadded, rows 512 bytes apart would collide 2-way).  The split of j depends on
// (n, g_x, g_y) alone and the finish launch adds the partial grids in order: a grid is bit-reproducible.
#include "api_internal.h"
#include "kde_state.h"
#include "kmath.h"

#pragma clang fp contract(off)

namespace {

constexpr int K2_TILE = 256;  // points per workgroup, samples per LDS tile and per bounding box
// gpmi_kde2d_self skips a tile whose every term has an exponent below -K2_SKIP.  There the points are the samples, so
// S_i >= 1 (the sample's own term is 1); what a point loses is at most n e^-80 <= 2^31 x 1.8e-35 = 3.9e-26, nine orders
// of magnitude below half an ulp of S_i (1.1e-16): the skipped sum rounds to the same double wherever the partials meet.
constexpr double K2_SKIP = 80.0;
constexpr int K2_MAXSPLIT = 64;      // ranges of the scattered evaluation (its partials: K2_MAXSPLIT x m doubles)
constexpr int64_t K2_BATCH = 1 << 18;  // points per launch of the scattered evaluation
constexpr int G_B = 64;    // grid block per workgroup: G_B x G_B outputs
constexpr int G_KC = 32;   // samples per chunk of the factorised grid
constexpr int G_LD = 80;   // LDS row (one sample, G_B factors) in doubles

// squared scaled distance between two boxes {xlo, xhi, ylo, yhi}: a lower bound of -exponent for every pair of them
__host__ __device__ inline double box_gap(const d4_t& I, const d4_t& J, double qx, double qy) {
  const double gx = fmax(0.0, fmax(J.x - I.y, I.x - J.y)) * qx;
  const double gy = fmax(0.0, fmax(J.z - I.w, I.z - J.w)) * qy;
  return gx * gx + gy * gy;
}

// part[split * m + i] = sum over the split's samples of exp(-((x_j - a_i) q_x)^2 - ((y_j - b_i) q_y)^2)
template <bool SKIP>
__global__ __launch_bounds__(256) void kde2d_partial(const d2_t* __restrict__ s, int64_t n, const d2_t* __restrict__ p,
                                                     int64_t m, int64_t per_split, const d4_t* __restrict__ box, double qx,
                                                     double qy, double* __restrict__ part) {
  __shared__ d2_t sj[K2_TILE];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * K2_TILE + t;
  const d2_t pt = p[i < m ? i : m - 1];
  const int64_t j0 = (int64_t)blockIdx.y * per_split;
  const int64_t j1 = j0 + per_split < n ? j0 + per_split : n;
  d4_t ibox = {0.0, 0.0, 0.0, 0.0};
  if (SKIP) ibox = box[blockIdx.x];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t jb = j0; jb < j1; jb += K2_TILE) {
    if (SKIP && box_gap(ibox, box[jb / K2_TILE], qx, qy) > K2_SKIP) continue;  // uniform over the workgroup
    const int cnt = (int)(jb + K2_TILE < j1 ? K2_TILE : j1 - jb);
    __syncthreads();
    if (t < cnt) sj[t] = s[jb + t];
    __syncthreads();
    for (int k = 0; k < cnt; k += 4) {
      double arg[4], e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const d2_t v = sj[k + u < cnt ? k + u : cnt - 1];
        const double tx = (v.x - pt.x) * qx, ty = (v.y - pt.y) * qy;
        arg[u] = -(tx * tx) - ty * ty;
      }
      kmath::exp_neg<4>(arg, e);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += k + u < cnt ? e[u] : 0.0;
    }
  }
  if (i < m) part[(int64_t)blockIdx.y * m + i] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// one thread per point: its range partials in range order, written to the caller's position (perm[i], or i)
__global__ __launch_bounds__(256) void kde2d_finish(const double* __restrict__ part, int64_t m, int nsplit,
                                                    const int* __restrict__ perm, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double S = 0.0;
  for (int k = 0; k < nsplit; ++k) S += part[(int64_t)k * m + i];
  out[perm ? perm[i] : i] = S;
}

// part[(split * gy + b) * gx + a] = sum over the split's samples of exp(-((x_j - xa[a]) q_x)^2) exp(-((y_j - ya[b]) q_y)^2)
__global__ __launch_bounds__(256) void kde2d_grid_partial(const d2_t* __restrict__ s, int64_t n, int64_t per_split,
                                                          const double* __restrict__ xa, int gx,
                                                          const double* __restrict__ ya, int gy, double qx, double qy,
                                                          double* __restrict__ part) {
  __shared__ double Ex[G_KC * G_LD], Ey[G_KC * G_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int wx = wave & 1, wy = wave >> 1;
  const int a0 = blockIdx.x * G_B, b0 = blockIdx.y * G_B;
  const int64_t j0 = (int64_t)blockIdx.z * per_split;
  const int64_t j1 = j0 + per_split < n ? j0 + per_split : n;
  // this thread forms column `lane` of both factor tiles, for the samples k = wave + 4 u of a chunk
  const double a = xa[a0 + lane < gx ? a0 + lane : gx - 1];
  const double b = ya[b0 + lane < gy ? b0 + lane : gy - 1];
  d4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int64_t jc = j0; jc < j1; jc += G_KC) {
    double ax[G_KC / 4], ay[G_KC / 4], ex[G_KC / 4], ey[G_KC / 4];
#pragma unroll
    for (int u = 0; u < G_KC / 4; ++u) {
      const int64_t j = jc + wave + 4 * u;
      const d2_t v = s[j < j1 ? j : j1 - 1];
      const double tx = (v.x - a) * qx, ty = (v.y - b) * qy;
      ax[u] = -(tx * tx);
      ay[u] = -(ty * ty);
    }
    kmath::exp_neg<G_KC / 4>(ax, ex);
    kmath::exp_neg<G_KC / 4>(ay, ey);
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int u = 0; u < G_KC / 4; ++u) {
      const int k = wave + 4 * u;
      const bool valid = jc + k < j1;
      Ex[k * G_LD + lane] = valid ? ex[u] : 0.0;
      Ey[k * G_LD + lane] = valid ? ey[u] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < G_KC / 4; ++kk) {
      const int row = (4 * kk + fk) * G_LD;
      double af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = Ey[row + wy * 32 + 16 * i + fr];
        bf[i] = Ex[row + wx * 32 + 16 * i + fr];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }
  // result r of lane (fr, fk) of an MFMA tile: row fk + 4 r, column fr
  double* out = part + (int64_t)blockIdx.z * gy * gx;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b0 + wy * 32 + 16 * i + fk + 4 * r, col = a0 + wx * 32 + 16 * j + fr;
        if (row < gy && col < gx) out[(int64_t)row * gx + col] = acc[i][j][r];
      }
}

}  // namespace

// A 2-D density object: the binned samples as (x, y) pairs, the caller's position of each, and the tile boxes.
struct gpmi_kde2d {
  gpmi_ctx* ctx = nullptr;
  int64_t n = 0, ntiles = 0;
  DevBuf<d2_t> s;    // n binned samples (device)
  DevBuf<int> perm;  // perm[i]: the caller's index of binned sample i (device)
  DevBuf<d4_t> box;  // ntiles boxes {xlo, xhi, ylo, yhi} (device)
  std::vector<d4_t> hbox;
};

void kde2d_free(gpmi_kde2d* k) { delete k; }

namespace {

// the object behind a pointer the caller passes, or nullptr when it is not a live object of any handle we can reach:
// the object's own ctx is read only after the pointer has been found in that handle's list
bool kde2d_live(gpmi_kde2d* k, gpmi_ctx* c) {
  KdeState* st = c ? c->kde : nullptr;
  return st && std::find(st->live2d.begin(), st->live2d.end(), k) != st->live2d.end();
}

int check_q(gpmi_ctx* c, double qx, double qy, const char* msg) {
  ARGCHK(c, std::isfinite(qx) && qx > 0.0 && std::isfinite(qy) && qy > 0.0, msg);
  return GPMI_OK;
}

// the scattered sum of m staged points (device pairs d_p) into d_out, all ranges: enqueue only
int enqueue_direct(gpmi_ctx* c, KdeState* st, gpmi_kde2d* k, const d2_t* d_p, int64_t m, double qx, double qy,
                   double* d_part, double* d_out) {
  const int64_t n = k->n;
  // ranges by n alone: at most K2_MAXSPLIT of them, whole tiles, at least 2048 samples each
  int64_t per = std::max<int64_t>(2048, (n + K2_MAXSPLIT - 1) / K2_MAXSPLIT);
  per = (per + K2_TILE - 1) / K2_TILE * K2_TILE;
  const int64_t nsp = (n + per - 1) / per;
  const dim3 grid((unsigned)((m + K2_TILE - 1) / K2_TILE), (unsigned)nsp);
  hipLaunchKernelGGL(kde2d_partial<false>, grid, dim3(256), 0, st->stream, k->s, n, d_p, m, per, nullptr, qx, qy, d_part);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(kde2d_finish, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st->stream, d_part, m, (int)nsp, nullptr,
                     d_out);
  HIPCHK(c, hipGetLastError());
  return GPMI_OK;
}

}  // namespace

extern "C" {

int gpmi_kde2d_create(gpmi_ctx* c, int64_t n, const double* x, const double* y, gpmi_kde2d** out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, out != nullptr, "gpmi_kde2d_create: out is NULL");
  *out = nullptr;
  ARGCHK(c, x && y, "gpmi_kde2d_create: x and y must be non-NULL");
  ARGCHK(c, n >= 1 && n <= INT32_MAX, "gpmi_kde2d_create: n out of range (1 .. 2^31 - 1)");
  for (int64_t i = 0; i < n; ++i)
    ARGCHK(c, std::isfinite(x[i]) && std::isfinite(y[i]), "gpmi_kde2d_create: samples must be finite");
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;

  // bins: by x, strips of whole tiles (about sqrt(ntiles) of them), each strip by y
  const int64_t ntiles = (n + K2_TILE - 1) / K2_TILE;
  const int64_t nstrips = std::max<int64_t>(1, (int64_t)std::llround(std::sqrt((double)ntiles)));
  const int64_t strip = (ntiles + nstrips - 1) / nstrips * K2_TILE;
  std::vector<int> perm(n);
  for (int64_t i = 0; i < n; ++i) perm[i] = (int)i;
  std::sort(perm.begin(), perm.end(), [&](int a, int b) { return x[a] != x[b] ? x[a] < x[b] : a < b; });
  for (int64_t b = 0; b < n; b += strip)
    std::sort(perm.begin() + b, perm.begin() + std::min(n, b + strip),
              [&](int a, int b2) { return y[a] != y[b2] ? y[a] < y[b2] : a < b2; });
  std::vector<d2_t> s(n);
  for (int64_t i = 0; i < n; ++i) s[i] = d2_t{x[perm[i]], y[perm[i]]};
  gpmi_kde2d* k = new gpmi_kde2d();
  k->ctx = c;
  k->n = n;
  k->ntiles = ntiles;
  k->hbox.resize(ntiles);
  for (int64_t tl = 0; tl < ntiles; ++tl) {
    d4_t bx = {s[tl * K2_TILE].x, s[tl * K2_TILE].x, s[tl * K2_TILE].y, s[tl * K2_TILE].y};
    for (int64_t i = tl * K2_TILE; i < std::min(n, (tl + 1) * K2_TILE); ++i) {
      bx.x = std::min(bx.x, s[i].x);
      bx.y = std::max(bx.y, s[i].x);
      bx.z = std::min(bx.z, s[i].y);
      bx.w = std::max(bx.w, s[i].y);
    }
    k->hbox[tl] = bx;
  }
  int rc = kde_upload(c, k->s, s.data(), n, "gpmi_kde2d_create");
  if (!rc) rc = kde_upload(c, k->perm, perm.data(), n, "gpmi_kde2d_create");
  if (!rc) rc = kde_upload(c, k->box, k->hbox.data(), ntiles, "gpmi_kde2d_create");
  if (rc) {
    delete k;
    return rc;
  }
  st->live2d.push_back(k);
  *out = k;
  return GPMI_OK;
}

int gpmi_kde2d_destroy(gpmi_ctx* c, gpmi_kde2d* k) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, k && kde2d_live(k, c), "gpmi_kde2d_destroy: not a live 2-D density object of this handle");
  KdeState* st = c->kde;
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st->stream));
  st->live2d.erase(std::find(st->live2d.begin(), st->live2d.end(), k));
  kde2d_free(k);
  return GPMI_OK;
}

int gpmi_kde2d_eval(gpmi_ctx* c, gpmi_kde2d* k, int64_t m, const double* a, const double* b, double qx, double qy,
                    double* sum) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, k && kde2d_live(k, c), "gpmi_kde2d_eval: not a live 2-D density object of this handle");
  ARGCHK(c, m >= 0 && m <= INT32_MAX, "gpmi_kde2d_eval: m out of range");
  if (int rc = check_q(c, qx, qy, "gpmi_kde2d_eval: q_x and q_y must be finite and positive")) return rc;
  if (m == 0) return GPMI_OK;
  ARGCHK(c, a && b && sum, "gpmi_kde2d_eval: a, b and sum must be non-NULL");
  for (int64_t i = 0; i < m; ++i)
    ARGCHK(c, std::isfinite(a[i]) && std::isfinite(b[i]), "gpmi_kde2d_eval: points must be finite");
  if (int rc = set_device(c)) return rc;
  KdeState* st = c->kde;
  const int64_t mb = std::min(m, K2_BATCH);
  const size_t in_bytes = kde_align256(16 * (size_t)mb), out_bytes = kde_align256(8 * (size_t)mb);
  const size_t part_bytes = kde_align256(8 * (size_t)K2_MAXSPLIT * mb);
  if (int rc = st->reserve_pinned(c, in_bytes + out_bytes)) return rc;
  if (int rc = st->reserve_in(c, in_bytes)) return rc;
  if (int rc = st->reserve_work(c, part_bytes + out_bytes)) return rc;
  d2_t* hp = reinterpret_cast<d2_t*>(st->h_stage.get());
  char* hout = st->h_stage + in_bytes;
  double* d_out = reinterpret_cast<double*>(st->d_work + part_bytes);
  for (int64_t i0 = 0; i0 < m; i0 += K2_BATCH) {
    const int64_t mm = std::min(K2_BATCH, m - i0);
    for (int64_t i = 0; i < mm; ++i) hp[i] = d2_t{a[i0 + i], b[i0 + i]};
    HIPCHK(c, hipMemcpyAsync(st->d_in, hp, 16 * (size_t)mm, hipMemcpyHostToDevice, st->stream));
    if (int rc = enqueue_direct(c, st, k, reinterpret_cast<const d2_t*>(st->d_in.get()), mm, qx, qy, st->work(), d_out)) return rc;
    HIPCHK(c, hipMemcpyAsync(hout, d_out, 8 * (size_t)mm, hipMemcpyDeviceToHost, st->stream));
    HIPCHK(c, hipStreamSynchronize(st->stream));
    std::memcpy(sum + i0, hout, 8 * (size_t)mm);
  }
  return GPMI_OK;
}

int gpmi_kde2d_self(gpmi_ctx* c, gpmi_kde2d* k, double qx, double qy, double* sum, int64_t* tiles) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, k && kde2d_live(k, c), "gpmi_kde2d_self: not a live 2-D density object of this handle");
  if (int rc = check_q(c, qx, qy, "gpmi_kde2d_self: q_x and q_y must be finite and positive")) return rc;
  ARGCHK(c, sum != nullptr, "gpmi_kde2d_self: sum is NULL");
  if (int rc = set_device(c)) return rc;
  KdeState* st = c->kde;
  const int64_t n = k->n, ntiles = k->ntiles;
  // enough workgroups to fill the chip, but at least one tile per range (by n alone)
  const int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>((2048 + ntiles - 1) / ntiles, ntiles));
  const int64_t per = (ntiles + nsplit - 1) / nsplit * K2_TILE;
  const int64_t nsp = (n + per - 1) / per;
  const size_t part_bytes = kde_align256(8 * (size_t)nsp * n), out_bytes = kde_align256(8 * (size_t)n);
  if (int rc = st->reserve_pinned(c, out_bytes)) return rc;
  if (int rc = st->reserve_work(c, part_bytes + out_bytes)) return rc;
  double* d_out = reinterpret_cast<double*>(st->d_work + part_bytes);
  hipLaunchKernelGGL(kde2d_partial<true>, dim3((unsigned)ntiles, (unsigned)nsp), dim3(256), 0, st->stream, k->s, n, k->s, n,
                     per, k->box, qx, qy, st->work());
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(kde2d_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st->stream, st->work(), n, (int)nsp,
                     k->perm, d_out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(st->h_stage, d_out, 8 * (size_t)n, hipMemcpyDeviceToHost, st->stream));
  if (tiles) {  // the kernel's own rule on the host copy of the boxes, while the device works
    int64_t done = 0;
    for (int64_t I = 0; I < ntiles; ++I)
      for (int64_t J = 0; J < ntiles; ++J) done += !(box_gap(k->hbox[I], k->hbox[J], qx, qy) > K2_SKIP);
    tiles[0] = done;
    tiles[1] = ntiles * ntiles;
  }
  HIPCHK(c, hipStreamSynchronize(st->stream));
  std::memcpy(sum, st->h_stage, 8 * (size_t)n);
  return GPMI_OK;
}

int gpmi_kde2d_grid(gpmi_ctx* c, gpmi_kde2d* k, int64_t gx, const double* xa, int64_t gy, const double* ya, double qx,
                    double qy, double* sum) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, k && kde2d_live(k, c), "gpmi_kde2d_grid: not a live 2-D density object of this handle");
  ARGCHK(c, gx >= 0 && gy >= 0 && gx <= 32768 && gy <= 32768, "gpmi_kde2d_grid: axis lengths out of range (0 .. 32768)");
  if (int rc = check_q(c, qx, qy, "gpmi_kde2d_grid: q_x and q_y must be finite and positive")) return rc;
  if (gx == 0 || gy == 0) return GPMI_OK;
  ARGCHK(c, xa && ya && sum, "gpmi_kde2d_grid: the axes and sum must be non-NULL");
  for (int64_t i = 0; i < gx; ++i) ARGCHK(c, std::isfinite(xa[i]), "gpmi_kde2d_grid: axis values must be finite");
  for (int64_t i = 0; i < gy; ++i) ARGCHK(c, std::isfinite(ya[i]), "gpmi_kde2d_grid: axis values must be finite");
  if (int rc = set_device(c)) return rc;
  KdeState* st = c->kde;
  const int64_t n = k->n, cells = gx * gy;
  const int64_t bxn = (gx + G_B - 1) / G_B, byn = (gy + G_B - 1) / G_B;
  // ranges by (n, g_x, g_y) alone: about 1024 workgroups, whole chunks, at least 1024 samples each, partials <= 256 MiB
  int64_t want = std::max<int64_t>(1, 1024 / (bxn * byn));
  want = std::min(want, std::max<int64_t>(1, ((int64_t)1 << 25) / cells));
  int64_t per = std::max<int64_t>(1024, (n + want - 1) / want);
  per = (per + G_KC - 1) / G_KC * G_KC;
  const int64_t nsp = (n + per - 1) / per;
  ARGCHK(c, nsp <= 65535, "gpmi_kde2d_grid: too many ranges");
  const size_t o_y = kde_align256(8 * (size_t)gx), in_bytes = kde_align256(o_y + 8 * (size_t)gy);
  const size_t part_bytes = kde_align256(8 * (size_t)nsp * cells), out_bytes = kde_align256(8 * (size_t)cells);
  if (int rc = st->reserve_pinned(c, in_bytes + out_bytes)) return rc;
  if (int rc = st->reserve_in(c, in_bytes)) return rc;
  if (int rc = st->reserve_work(c, part_bytes + out_bytes)) return rc;
  std::memcpy(st->h_stage, xa, 8 * (size_t)gx);
  std::memcpy(st->h_stage + o_y, ya, 8 * (size_t)gy);
  HIPCHK(c, hipMemcpyAsync(st->d_in, st->h_stage, in_bytes, hipMemcpyHostToDevice, st->stream));
  double* d_out = reinterpret_cast<double*>(st->d_work + part_bytes);
  hipLaunchKernelGGL(kde2d_grid_partial, dim3((unsigned)bxn, (unsigned)byn, (unsigned)nsp), dim3(256), 0, st->stream, k->s, n,
                     per, reinterpret_cast<const double*>(st->d_in.get()), (int)gx, reinterpret_cast<const double*>(st->d_in + o_y),
                     (int)gy, qx, qy, st->work());
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(kde2d_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st->stream, st->work(), cells, (int)nsp,
                     nullptr, d_out);
  HIPCHK(c, hipGetLastError());
  char* hout = st->h_stage + in_bytes;
  HIPCHK(c, hipMemcpyAsync(hout, d_out, 8 * (size_t)cells, hipMemcpyDeviceToHost, st->stream));
  HIPCHK(c, hipStreamSynchronize(st->stream));
  std::memcpy(sum, hout, 8 * (size_t)cells);
  return GPMI_OK;
}

}  // extern "C"
