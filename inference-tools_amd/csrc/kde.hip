// Gaussian kernel-density estimation (GaussianKDE, reference inference/pdf/kde.py) on the device: the truncated slice
// sums behind the pdf and the cdf (kde.py:92-133) and the leave-one-out cross-validation log-probability of the bandwidth
// search (kde.py:195-218), with the C-ABI entry points gpmi_kde_* of include/gpmi.h.
//
// Slice sums.  A point x of region r sums over the sorted samples s_j, j in [lo_r, hi_r):
//     pdf: sum_j exp(-((x - s_j) q)^2)        cdf: sum_j (1 + erf((x - s_j) q))
// The host orders the points by region (points of one region share a slice) and deals them to groups of KDE_PTS
// consecutive points; a work item is (group, chunk of KDE_CHUNK samples at an absolute offset k * KDE_CHUNK) for every
// chunk the group's slices touch.  A workgroup stages its chunk in LDS and runs KDE_LANES lanes per point; lane l takes
// the samples j with (j - chunk start) = l mod KDE_LANES, in increasing order, and the lanes meet in a fixed xor tree.
// A second launch adds a point's chunk partials in chunk order.  Every boundary is absolute, so a point's value does
// not depend on which other points share the call (M = 1 gives the bits of a large batch), and there is no atomic.
//
// Leave-one-out.  For H bandwidths at once, S_i(h) = sum_j exp(-(x_i - x_j)^2 / (2 h^2)) (the self term included, so
// S_i >= 1) over the sorted copy of the samples; a workgroup takes 256 consecutive i and one of `nsplit` ranges of j,
// computes each distance once for all H, and skips a 256-sample tile of j whose every |x_i - x_j| exceeds 38.6 h_max
// (such a term is below the smallest subnormal and cannot change S_i >= 1).  The finish launch adds the splits in
// order and reduces log S_i - log(h n sqrt(2 pi)) + log(1 - c / S_i) over a workgroup in a fixed tree; the host adds the
// workgroup sums in order.
#include "api_internal.h"
#include "kde_state.h"
#include "kmath.h"

namespace {

constexpr int KDE_PTS = 16;      // points per workgroup of the slice sum
constexpr int KDE_LANES = 16;    // lanes per point: KDE_PTS x KDE_LANES = 256 threads
constexpr int KDE_CHUNK = 2048;  // samples per work item (16 KiB of LDS)
constexpr int CV_TILE = 256;     // samples i per workgroup (and samples j per LDS tile) of the leave-one-out sum
constexpr int CV_MAXH = 8;       // bandwidths per leave-one-out launch
constexpr double CV_REACH = 38.6;  // exp(-38.6^2 / 2) < 2^-1074: a term beyond 38.6 h_max is zero to S_i >= 1

// ---- slice sums ----------------------------------------------------------------------------------------------------
template <bool PDF, bool CDF>
__global__ __launch_bounds__(256) void kde_slice_sum(const double* __restrict__ s, int64_t n,
                                                     const double* __restrict__ xs, const int* __restrict__ plo,
                                                     const int* __restrict__ phi, const int* __restrict__ group_pt,
                                                     const int* __restrict__ item_group, const int* __restrict__ item_chunk,
                                                     double q, double* __restrict__ part_pdf, double* __restrict__ part_cdf) {
  __shared__ double tile[KDE_CHUNK];
  const int item = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t g = item_group[item];
  const int64_t c0 = (int64_t)item_chunk[item] * KDE_CHUNK;
  const int64_t c1 = c0 + KDE_CHUNK < n ? c0 + KDE_CHUNK : n;
  for (int64_t k = t; k < c1 - c0; k += 256) tile[k] = s[c0 + k];
  __syncthreads();
  const int p = t / KDE_LANES, lane = t % KDE_LANES;
  const bool valid = p < group_pt[g + 1] - group_pt[g];
  const int64_t pi = (int64_t)group_pt[g] + p;
  double sp = 0.0, sc = 0.0;
  if (valid) {
    const double x = xs[pi];
    const int64_t a = plo[pi] > c0 ? (int64_t)plo[pi] : c0;
    const int64_t b = phi[pi] < c1 ? (int64_t)phi[pi] : c1;
    // first j >= a with (j - c0) = lane (mod KDE_LANES); terms past b are exact zeros (adding them changes nothing)
    int64_t j = a + (((int64_t)lane - (a - c0)) % KDE_LANES + KDE_LANES) % KDE_LANES;
    for (; j < b; j += 4 * KDE_LANES) {
      double tq[4], arg[4], e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t jj = j + u * KDE_LANES;
        tq[u] = jj < b ? (x - tile[jj - c0]) * q : 0.0;
        arg[u] = -(tq[u] * tq[u]);
      }
      if (PDF) {
        kmath::exp_neg<4>(arg, e);
#pragma unroll
        for (int u = 0; u < 4; ++u) sp += (j + u * KDE_LANES < b) ? e[u] : 0.0;
      }
      if (CDF) {
#pragma unroll
        for (int u = 0; u < 4; ++u) sc += (j + u * KDE_LANES < b) ? 1.0 + erf(tq[u]) : 0.0;
      }
    }
  }
#pragma unroll
  for (int off = KDE_LANES / 2; off >= 1; off >>= 1) {
    if (PDF) sp += __shfl_xor(sp, off, KDE_LANES);
    if (CDF) sc += __shfl_xor(sc, off, KDE_LANES);
  }
  if (lane == 0 && valid) {
    if (PDF) part_pdf[(int64_t)item * KDE_PTS + p] = sp;
    if (CDF) part_cdf[(int64_t)item * KDE_PTS + p] = sc;
  }
}

// one thread per (sorted) point: its group's partials in chunk order, written to the caller's position order[pi].  The
// loads of FIN_BATCH partials are issued before they are added (in order): a long slice is not a chain of latencies.
constexpr int FIN_BATCH = 16;
__global__ __launch_bounds__(256) void kde_slice_finish(const double* __restrict__ part_pdf,
                                                        const double* __restrict__ part_cdf,
                                                        const int* __restrict__ group_first, const int* __restrict__ group_pt,
                                                        const int* __restrict__ pt_group, const int* __restrict__ order,
                                                        int64_t m, double* __restrict__ out_pdf, double* __restrict__ out_cdf) {
  const int64_t pi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pi >= m) return;
  const int g = pt_group[pi];
  const int64_t p = pi - group_pt[g];
  const int a = group_first[g], b = group_first[g + 1];
  double sp = 0.0, sc = 0.0;
  for (int it0 = a; it0 < b; it0 += FIN_BATCH) {
    double vp[FIN_BATCH], vc[FIN_BATCH];
#pragma unroll
    for (int u = 0; u < FIN_BATCH; ++u) {
      const int it = it0 + u;
      vp[u] = (part_pdf && it < b) ? part_pdf[(int64_t)it * KDE_PTS + p] : 0.0;
      vc[u] = (part_cdf && it < b) ? part_cdf[(int64_t)it * KDE_PTS + p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < FIN_BATCH; ++u) {
      sp += vp[u];
      sc += vc[u];
    }
  }
  const int64_t o = order[pi];
  if (out_pdf) out_pdf[o] = sp;
  if (out_cdf) out_cdf[o] = sc;
}

// ---- leave-one-out ---------------------------------------------------------------------------------------------------
// part[(split * H + h) * n + i] = sum over the split's j of exp(-(x_i - x_j)^2 rh_h^2 / 2), rh = 1 / h
template <int H>
__global__ __launch_bounds__(256) void kde_cv_partial(const double* __restrict__ s, int64_t n, int64_t per_split,
                                                      const double* __restrict__ rh_dev, double reach,
                                                      double* __restrict__ part) {
  __shared__ double sj[CV_TILE];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * CV_TILE;
  const int64_t i = i0 + t;
  const int64_t i_last = (i0 + CV_TILE < n ? i0 + CV_TILE : n) - 1;
  const int64_t j0 = (int64_t)blockIdx.y * per_split;
  const int64_t j1 = j0 + per_split < n ? j0 + per_split : n;
  const double xi = i < n ? s[i] : s[i_last];
  const double ilo = s[i0], ihi = s[i_last];
  double rh[H], acc[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    rh[h] = rh_dev[h];
    acc[h] = 0.0;
  }
  for (int64_t jb = j0; jb < j1; jb += CV_TILE) {
    const int64_t je = jb + CV_TILE < j1 ? jb + CV_TILE : j1;
    const double jlo = s[jb], jhi = s[je - 1];
    if (jlo - ihi > reach) break;  // sorted: every later tile is further away
    if (ilo - jhi > reach) continue;
    __syncthreads();
    if (jb + t < je) sj[t] = s[jb + t];
    __syncthreads();
    const int cnt = (int)(je - jb);
    for (int k = 0; k < cnt; ++k) {
      const double d = xi - sj[k];
      double arg[H], e[H];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const double z = d * rh[h];
        arg[h] = -0.5 * (z * z);
      }
      kmath::exp_neg<H>(arg, e);
#pragma unroll
      for (int h = 0; h < H; ++h) acc[h] += e[h];
    }
  }
  if (i < n) {
#pragma unroll
    for (int h = 0; h < H; ++h) part[((int64_t)blockIdx.y * H + h) * n + i] = acc[h];
  }
}

// per workgroup and bandwidth: sum over its 256 i of log S_i - lnorm_h + log1p(-c / S_i), in a fixed tree
__global__ __launch_bounds__(256) void kde_cv_finish(const double* __restrict__ part, int64_t n, int nsplit, int H,
                                                     const double* __restrict__ lnorm, double c,
                                                     double* __restrict__ block_sum) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  for (int h = 0; h < H; ++h) {
    double v = 0.0;
    if (i < n) {
      double S = 0.0;
      for (int k = 0; k < nsplit; ++k) S += part[((int64_t)k * H + h) * n + i];
      v = (log(S) - lnorm[h]) + log1p(-c / S);
    }
    red[t] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if (t < w) red[t] += red[t + w];
      __syncthreads();
    }
    if (t == 0) block_sum[(int64_t)blockIdx.x * H + h] = red[0];
    __syncthreads();
  }
}

template <int H>
void launch_cv_partial_h(hipStream_t st, dim3 grid, const double* s, int64_t n, int64_t per, const double* rh, double reach,
                         double* part) {
  hipLaunchKernelGGL(kde_cv_partial<H>, grid, dim3(256), 0, st, s, n, per, rh, reach, part);
}

void launch_cv_partial(int H, hipStream_t st, dim3 grid, const double* s, int64_t n, int64_t per, const double* rh,
                       double reach, double* part) {
  switch (H) {
    case 1: launch_cv_partial_h<1>(st, grid, s, n, per, rh, reach, part); break;
    case 2: launch_cv_partial_h<2>(st, grid, s, n, per, rh, reach, part); break;
    case 3: launch_cv_partial_h<3>(st, grid, s, n, per, rh, reach, part); break;
    case 4: launch_cv_partial_h<4>(st, grid, s, n, per, rh, reach, part); break;
    case 5: launch_cv_partial_h<5>(st, grid, s, n, per, rh, reach, part); break;
    case 6: launch_cv_partial_h<6>(st, grid, s, n, per, rh, reach, part); break;
    case 7: launch_cv_partial_h<7>(st, grid, s, n, per, rh, reach, part); break;
    default: launch_cv_partial_h<8>(st, grid, s, n, per, rh, reach, part); break;
  }
}

}  // namespace

// A density object: the sorted sample and its region table on the device, host copies of the table for the work lists.
struct gpmi_kde {
  gpmi_ctx* ctx = nullptr;
  int64_t n = 0, n_regions = 0;
  DevBuf<double> s;  // n sorted samples (device)
  std::vector<int> lo, hi;
};

// Per-handle state of the density entry points (KdeState, kde_state.h), shared with kde2d.hip
int kde_state(gpmi_ctx* c, KdeState*& st) {
  if (!c->kde) c->kde = new KdeState();
  st = c->kde;
  if (!st->stream) HIPCHK(c, hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
  return GPMI_OK;
}

namespace {
size_t align256(size_t b) { return kde_align256(b); }
}  // namespace

void kde_release_all(gpmi_ctx* c) {
  KdeState* st = c->kde;
  if (!st) return;
  if (st->stream) (void)hipStreamSynchronize(st->stream);
  for (gpmi_kde* k : st->live) delete k;
  st->live.clear();
  for (gpmi_kde2d* k : st->live2d) kde2d_free(k);
  st->live2d.clear();
  for (gpmi_unimodal* k : st->live_uni) unimodal_free(k);
  st->live_uni.clear();
  st->h_stage.release();
  st->d_in.release();
  st->d_work.release();
  if (st->stream) (void)hipStreamDestroy(st->stream);
  delete st;
  c->kde = nullptr;
}

extern "C" {

int gpmi_kde_create(gpmi_ctx* c, int64_t n, const double* sample, int64_t n_regions, const int64_t* lo,
                    const int64_t* hi, gpmi_kde** out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, out != nullptr, "gpmi_kde_create: out is NULL");
  *out = nullptr;
  ARGCHK(c, sample && lo && hi, "gpmi_kde_create: sample, lo and hi must be non-NULL");
  ARGCHK(c, n >= 1 && n <= INT32_MAX, "gpmi_kde_create: n out of range (1 .. 2^31 - 1)");
  ARGCHK(c, n_regions >= 1 && n_regions <= INT32_MAX, "gpmi_kde_create: n_regions out of range");
  for (int64_t r = 0; r < n_regions; ++r)
    ARGCHK(c, lo[r] >= 0 && lo[r] <= hi[r] && hi[r] <= n, "gpmi_kde_create: a region slice is outside [0, n]");
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;
  gpmi_kde* k = new gpmi_kde();
  k->ctx = c;
  k->n = n;
  k->n_regions = n_regions;
  k->lo.assign(lo, lo + n_regions);
  k->hi.assign(hi, hi + n_regions);
  if (int rc = kde_upload(c, k->s, sample, n, "gpmi_kde_create")) {
    delete k;
    return rc;
  }
  st->live.push_back(k);
  *out = k;
  return GPMI_OK;
}

int gpmi_kde_destroy(gpmi_kde* k) {
  if (!k) return GPMI_ERR_ARG;
  gpmi_ctx* c = k->ctx;
  KdeState* st = c->kde;
  auto it = st ? std::find(st->live.begin(), st->live.end(), k) : std::vector<gpmi_kde*>::iterator();
  ARGCHK(c, st && it != st->live.end(), "gpmi_kde_destroy: not a live density object of this handle");
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st->stream));
  st->live.erase(it);
  delete k;
  return GPMI_OK;
}

int gpmi_kde_eval(gpmi_kde* k, int64_t m, const double* x, const int64_t* region, double q, double* pdf_sum,
                  double* cdf_sum) {
  if (!k) return GPMI_ERR_ARG;
  gpmi_ctx* c = k->ctx;
  ARGCHK(c, m >= 0 && m <= INT32_MAX / 2, "gpmi_kde_eval: m out of range");
  ARGCHK(c, pdf_sum || cdf_sum, "gpmi_kde_eval: both outputs are NULL");
  ARGCHK(c, std::isfinite(q) && q > 0.0, "gpmi_kde_eval: q must be finite and positive");
  if (m == 0) return GPMI_OK;
  ARGCHK(c, x && region, "gpmi_kde_eval: x and region must be non-NULL");
  for (int64_t i = 0; i < m; ++i)
    ARGCHK(c, region[i] >= 0 && region[i] < k->n_regions, "gpmi_kde_eval: a region index is out of range");
  if (int rc = set_device(c)) return rc;
  KdeState* st = c->kde;

  // points in region order (ties by x): the slices of a group then nearly coincide
  std::vector<int> order(m);
  for (int64_t i = 0; i < m; ++i) order[i] = (int)i;
  bool sorted = true;
  for (int64_t i = 1; i < m && sorted; ++i)
    sorted = region[i - 1] < region[i] || (region[i - 1] == region[i] && !(x[i] < x[i - 1]));
  if (!sorted)
    std::sort(order.begin(), order.end(), [&](int a, int b) {
      if (region[a] != region[b]) return region[a] < region[b];
      if (x[a] != x[b]) return x[a] < x[b];
      return a < b;
    });
  // groups: up to KDE_PTS consecutive points; a point whose slice starts at or after the end of the group's union starts
  // a new group, so that distant points (the two ends of an interval) do not share the chunks between them.  A point's
  // partials outside its own slice are exact zeros, so the grouping changes no value.
  std::vector<int> group_pt(1, 0), pt_group(m), group_first(1, 0), item_group, item_chunk;
  int64_t A = k->n, B = 0;
  auto close_group = [&]() {
    for (int64_t ch = (B > A ? A / KDE_CHUNK : 0); B > A && ch <= (B - 1) / KDE_CHUNK; ++ch) {
      item_group.push_back((int)group_pt.size() - 1);
      item_chunk.push_back((int)ch);
    }
    group_first.push_back((int)item_group.size());
    A = k->n;
    B = 0;
  };
  for (int64_t pi = 0; pi < m; ++pi) {
    const int64_t r = region[order[pi]];
    const int64_t lo_p = k->lo[r], hi_p = k->hi[r];
    const int64_t in_group = pi - group_pt.back();
    if (in_group == KDE_PTS || (in_group > 0 && B > A && lo_p < hi_p && lo_p >= B)) {
      close_group();
      group_pt.push_back((int)pi);
    }
    pt_group[pi] = (int)group_pt.size() - 1;
    if (lo_p < hi_p) {
      A = std::min(A, lo_p);
      B = std::max(B, hi_p);
    }
  }
  close_group();
  group_pt.push_back((int)m);
  const int64_t ngroups = (int64_t)group_pt.size() - 1;
  const int64_t items = (int64_t)item_group.size();
  ARGCHK(c, items < INT32_MAX, "gpmi_kde_eval: too many work items");

  // staged inputs: xs | plo | phi | order | pt_group | group_pt | group_first | item_group | item_chunk ; outputs: pdf | cdf
  const size_t o_x = 0, o_lo = align256(o_x + 8 * m), o_hi = align256(o_lo + 4 * m), o_ord = align256(o_hi + 4 * m),
               o_pg = align256(o_ord + 4 * m), o_gp = align256(o_pg + 4 * m), o_gf = align256(o_gp + 4 * (ngroups + 1)),
               o_ig = align256(o_gf + 4 * (ngroups + 1)), o_ic = align256(o_ig + 4 * items),
               in_bytes = align256(o_ic + 4 * items);
  const size_t out_bytes = 2 * align256(8 * m);
  if (int rc = st->reserve_pinned(c, in_bytes + out_bytes)) return rc;
  char* h = st->h_stage;
  double* hx = reinterpret_cast<double*>(h + o_x);
  int* hlo = reinterpret_cast<int*>(h + o_lo);
  int* hhi = reinterpret_cast<int*>(h + o_hi);
  for (int64_t pi = 0; pi < m; ++pi) {
    const int64_t r = region[order[pi]];
    hx[pi] = x[order[pi]];
    hlo[pi] = k->lo[r];
    hhi[pi] = k->hi[r];
  }
  std::memcpy(h + o_ord, order.data(), 4 * m);
  std::memcpy(h + o_pg, pt_group.data(), 4 * m);
  std::memcpy(h + o_gp, group_pt.data(), 4 * (ngroups + 1));
  std::memcpy(h + o_gf, group_first.data(), 4 * (ngroups + 1));
  if (items) {
    std::memcpy(h + o_ig, item_group.data(), 4 * items);
    std::memcpy(h + o_ic, item_chunk.data(), 4 * items);
  }
  const bool want_pdf = pdf_sum != nullptr, want_cdf = cdf_sum != nullptr;
  const size_t part = align256(8 * (size_t)std::max<int64_t>(items, 1) * KDE_PTS);
  const size_t outv = align256(8 * m);
  if (int rc = st->reserve_in(c, in_bytes)) return rc;
  if (int rc = st->reserve_work(c, 2 * part + 2 * outv)) return rc;
  char* d = st->d_in;
  char* w = st->d_work;
  double* d_ppdf = want_pdf ? reinterpret_cast<double*>(w) : nullptr;
  double* d_pcdf = want_cdf ? reinterpret_cast<double*>(w + part) : nullptr;
  double* d_opdf = want_pdf ? reinterpret_cast<double*>(w + 2 * part) : nullptr;
  double* d_ocdf = want_cdf ? reinterpret_cast<double*>(w + 2 * part + outv) : nullptr;
  HIPCHK(c, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st->stream));
  const double* dx = reinterpret_cast<const double*>(d + o_x);
  const int* dlo = reinterpret_cast<const int*>(d + o_lo);
  const int* dhi = reinterpret_cast<const int*>(d + o_hi);
  const int* dord = reinterpret_cast<const int*>(d + o_ord);
  const int* dpg = reinterpret_cast<const int*>(d + o_pg);
  const int* dgp = reinterpret_cast<const int*>(d + o_gp);
  const int* dgf = reinterpret_cast<const int*>(d + o_gf);
  const int* dig = reinterpret_cast<const int*>(d + o_ig);
  const int* dic = reinterpret_cast<const int*>(d + o_ic);
  if (items) {
    if (want_pdf && want_cdf)
      hipLaunchKernelGGL((kde_slice_sum<true, true>), dim3((unsigned)items), dim3(256), 0, st->stream, k->s, k->n, dx, dlo,
                         dhi, dgp, dig, dic, q, d_ppdf, d_pcdf);
    else if (want_pdf)
      hipLaunchKernelGGL((kde_slice_sum<true, false>), dim3((unsigned)items), dim3(256), 0, st->stream, k->s, k->n, dx, dlo,
                         dhi, dgp, dig, dic, q, d_ppdf, d_pcdf);
    else
      hipLaunchKernelGGL((kde_slice_sum<false, true>), dim3((unsigned)items), dim3(256), 0, st->stream, k->s, k->n, dx, dlo,
                         dhi, dgp, dig, dic, q, d_ppdf, d_pcdf);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(kde_slice_finish, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st->stream, d_ppdf, d_pcdf, dgf,
                     dgp, dpg, dord, m, d_opdf, d_ocdf);
  HIPCHK(c, hipGetLastError());
  char* hout = h + in_bytes;
  if (want_pdf) HIPCHK(c, hipMemcpyAsync(hout, d_opdf, 8 * m, hipMemcpyDeviceToHost, st->stream));
  if (want_cdf) HIPCHK(c, hipMemcpyAsync(hout + outv, d_ocdf, 8 * m, hipMemcpyDeviceToHost, st->stream));
  HIPCHK(c, hipStreamSynchronize(st->stream));
  if (want_pdf) std::memcpy(pdf_sum, hout, 8 * m);
  if (want_cdf) std::memcpy(cdf_sum, hout + outv, 8 * m);
  return GPMI_OK;
}

int gpmi_kde_cv_logprob(gpmi_ctx* c, int64_t n, const double* samples, int n_widths, const double* widths, double cc,
                        double* logprob) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, samples && widths && logprob, "gpmi_kde_cv_logprob: samples, widths and logprob must be non-NULL");
  ARGCHK(c, n >= 1 && n <= INT32_MAX, "gpmi_kde_cv_logprob: n out of range (1 .. 2^31 - 1)");
  ARGCHK(c, n_widths >= 1, "gpmi_kde_cv_logprob: n_widths must be positive");
  for (int h = 0; h < n_widths; ++h)
    ARGCHK(c, std::isfinite(widths[h]) && widths[h] > 0.0, "gpmi_kde_cv_logprob: widths must be finite and positive");
  ARGCHK(c, std::isfinite(cc) && cc > 0.0 && cc < 1.0, "gpmi_kde_cv_logprob: c must lie in (0, 1)");
  for (int64_t i = 0; i < n; ++i)
    ARGCHK(c, std::isfinite(samples[i]), "gpmi_kde_cv_logprob: samples must be finite");
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;

  const int64_t ntiles = (n + CV_TILE - 1) / CV_TILE;
  // enough workgroups to fill the chip, but at least one LDS tile of j per split
  const int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>((2048 + ntiles - 1) / ntiles, ntiles));
  const int64_t per = (ntiles + nsplit - 1) / nsplit * CV_TILE;
  const int64_t nsp = (n + per - 1) / per;
  const int HB = std::min(n_widths, CV_MAXH);
  // staged: sorted samples | rh | lnorm ; device work: partials | block sums
  const size_t o_s = 0, o_rh = align256(8 * n), o_ln = align256(o_rh + 8 * CV_MAXH), in_bytes = align256(o_ln + 8 * CV_MAXH);
  const size_t part_bytes = align256(8 * (size_t)nsp * HB * n), bs_bytes = align256(8 * (size_t)ntiles * HB);
  if (int rc = st->reserve_pinned(c, in_bytes + bs_bytes)) return rc;
  if (int rc = st->reserve_in(c, in_bytes)) return rc;
  if (int rc = st->reserve_work(c, part_bytes + bs_bytes)) return rc;
  char* h = st->h_stage;
  double* hs = reinterpret_cast<double*>(h + o_s);
  std::memcpy(hs, samples, 8 * n);
  std::sort(hs, hs + n);
  const double* d_s = reinterpret_cast<const double*>(st->d_in + o_s);
  double* d_rh = reinterpret_cast<double*>(st->d_in + o_rh);
  double* d_ln = reinterpret_cast<double*>(st->d_in + o_ln);
  double* d_part = st->work();
  double* d_bs = reinterpret_cast<double*>(st->d_work + part_bytes);
  const double* hbs = reinterpret_cast<const double*>(h + in_bytes);
  const double sqrt2pi = std::sqrt(2.0 * 3.14159265358979323846);
  bool first = true;
  for (int h0 = 0; h0 < n_widths; h0 += CV_MAXH) {
    const int H = std::min(CV_MAXH, n_widths - h0);
    double* hrh = reinterpret_cast<double*>(h + o_rh);
    double* hln = reinterpret_cast<double*>(h + o_ln);
    double hmax = 0.0;
    for (int k = 0; k < H; ++k) {
      const double w = widths[h0 + k];
      hrh[k] = 1.0 / w;
      hln[k] = std::log(w * (double)n * sqrt2pi);
      hmax = std::max(hmax, w);
    }
    // the samples travel once; later passes only replace the bandwidth block
    const size_t off = first ? 0 : o_rh;
    HIPCHK(c, hipMemcpyAsync(st->d_in + off, h + off, in_bytes - off, hipMemcpyHostToDevice, st->stream));
    first = false;
    launch_cv_partial(H, st->stream, dim3((unsigned)ntiles, (unsigned)nsp), d_s, n, per, d_rh, CV_REACH * hmax, d_part);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(kde_cv_finish, dim3((unsigned)ntiles), dim3(256), 0, st->stream, d_part, n, (int)nsp, H, d_ln, cc,
                       d_bs);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h + in_bytes, d_bs, 8 * (size_t)ntiles * H, hipMemcpyDeviceToHost, st->stream));
    HIPCHK(c, hipStreamSynchronize(st->stream));
    for (int k = 0; k < H; ++k) {
      double sum = 0.0;
      for (int64_t b = 0; b < ntiles; ++b) sum += hbs[b * H + k];
      logprob[h0 + k] = sum;
    }
  }
  return GPMI_OK;
}

}  // extern "C"
