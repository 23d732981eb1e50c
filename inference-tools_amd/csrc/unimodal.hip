// Sample sums of the unimodal density model (UnimodalPdf, reference inference/pdf/unimodal.py) on the device, with the
// C-ABI entry points gpmi_unimodal_* of include/gpmi.h.  For theta = (x0, s0, ln v, f, k, q) the log-density of a sample
// x is (unimodal.py:144-151)
//     z0 = (x - x0) / s0,   z = z0 exp(-f tanh(z0 / k)),   -(1 + v) / 2 * log(1 + |z|^q / v),   v = exp(ln v),
// and the fit asks 1100 - 1800 times for its sum over the sample (unimodal.py:132-134), or over every stride-th sample.
//
// The fitted samples (positions p = 0 .. n_fit - 1, sample p * stride) are cut into chunks of 256 * ipt positions, where
// ipt depends on n_fit alone (at most UNI_MAXCHUNKS chunks).  A workgroup takes one (chunk, theta): thread t adds the
// positions chunk start + t + 256 u, u = 0 .. ipt - 1, in that order, and the 256 threads meet in a fixed tree; the
// chunk's partial goes to a workspace.  A second launch (one workgroup per theta) adds the partials: thread t its run of
// consecutive chunks in index order, then the runs in the same fixed tree.  Neither the partition nor either order
// depends on the number of theta of the call, so one theta alone gives the bits it gives inside a batch, and there is
// no atomic.  The arithmetic is the reference's, operation for operation (division, no contraction into fma, pow for
// |z|^q, log(1 + .) rather than log1p), with the compiler's tanh / exp / pow / log: about five transcendentals per
// (sample, theta), so their accuracy matters and their speed hardly does.  |0|^q = 0 makes the term 0 at z = 0; a
// non-finite theta gives what IEEE arithmetic gives (NaN in, NaN out).
//
// The call is latency-bound: the theta of a launch (up to UNI_ARGS of them, v = exp(ln v) taken on the host) travel as
// kernel arguments, not through a copy, and the sums return through one pinned buffer and one stream synchronisation.
#include "api_internal.h"
#include "kde_state.h"

#pragma clang fp contract(off)

namespace {

constexpr int UNI_ARGS = 72;          // theta per launch, passed by value (72 x 6 x 8 B = 3456 B of kernel arguments): the guesses
constexpr int UNI_MAXCHUNKS = 1024;   // chunks of the fitted samples at most (the second launch: 4 per thread)

struct UniTheta {
  double p[UNI_ARGS][6];  // x0, s0, v, f, k, q
};

__device__ __forceinline__ double block_tree_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  return red[0];
}

// part[theta * nchunks + chunk] = sum over the chunk's positions of the log-density
__global__ __launch_bounds__(256) void unimodal_partial(const double* __restrict__ s, int64_t n_fit, int64_t stride, int ipt,
                                                        UniTheta th, int64_t nchunks, double* __restrict__ part) {
  __shared__ double red[256];
  const double* p = th.p[blockIdx.y];
  const double x0 = p[0], s0 = p[1], v = p[2], f = p[3], k = p[4], q = p[5];
  const double scale = -(0.5 * (1.0 + v));
  const int64_t first = (int64_t)blockIdx.x * 256 * ipt + threadIdx.x;
  double acc = 0.0;
  for (int u = 0; u < ipt; ++u) {
    const int64_t pos = first + (int64_t)u * 256;
    if (pos < n_fit) {
      const double z0 = (s[pos * stride] - x0) / s0;
      const double z = z0 * exp(-f * tanh(z0 / k));
      acc += scale * log(1.0 + pow(fabs(z), q) / v);
    }
  }
  const double sum = block_tree_sum(acc, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * nchunks + blockIdx.x] = sum;
}

// out[theta] = the partials of theta: thread t adds chunks [t * per, (t + 1) * per) in index order, then the fixed tree
__global__ __launch_bounds__(256) void unimodal_finish(const double* __restrict__ part, int64_t nchunks, int per,
                                                       double* __restrict__ out) {
  __shared__ double red[256];
  const double* p = part + (int64_t)blockIdx.x * nchunks;
  const int64_t a = (int64_t)threadIdx.x * per;
  double acc = 0.0;
  for (int u = 0; u < per; ++u) acc += a + u < nchunks ? p[a + u] : 0.0;
  const double sum = block_tree_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

bool unimodal_live(gpmi_unimodal* k, gpmi_ctx* c) {
  KdeState* st = c ? c->kde : nullptr;
  return st && std::find(st->live_uni.begin(), st->live_uni.end(), k) != st->live_uni.end();
}

}  // namespace

// The sample, in the order given, on the device
struct gpmi_unimodal {
  gpmi_ctx* ctx = nullptr;
  int64_t n = 0;
  DevBuf<double> s;
};

void unimodal_free(gpmi_unimodal* k) { delete k; }

extern "C" {

int gpmi_unimodal_create(gpmi_ctx* c, int64_t n, const double* sample, gpmi_unimodal** out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, out != nullptr, "gpmi_unimodal_create: out is NULL");
  *out = nullptr;
  ARGCHK(c, sample != nullptr, "gpmi_unimodal_create: sample is NULL");
  ARGCHK(c, n >= 1 && n <= INT32_MAX, "gpmi_unimodal_create: n out of range (1 .. 2^31 - 1)");
  if (int rc = set_device(c)) return rc;
  KdeState* st = nullptr;
  if (int rc = kde_state(c, st)) return rc;
  gpmi_unimodal* k = new gpmi_unimodal();
  k->ctx = c;
  k->n = n;
  if (int rc = kde_upload(c, k->s, sample, n, "gpmi_unimodal_create")) {
    delete k;
    return rc;
  }
  st->live_uni.push_back(k);
  *out = k;
  return GPMI_OK;
}

int gpmi_unimodal_destroy(gpmi_ctx* c, gpmi_unimodal* k) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, k && unimodal_live(k, c), "gpmi_unimodal_destroy: not a live unimodal object of this handle");
  KdeState* st = c->kde;
  if (int rc = set_device(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st->stream));
  st->live_uni.erase(std::find(st->live_uni.begin(), st->live_uni.end(), k));
  unimodal_free(k);
  return GPMI_OK;
}

int gpmi_unimodal_logpdf_sums(gpmi_ctx* c, gpmi_unimodal* k, int64_t stride, int n_theta, const double* theta,
                              double* out) {
  if (!c) return GPMI_ERR_ARG;
  ARGCHK(c, k && unimodal_live(k, c), "gpmi_unimodal_logpdf_sums: not a live unimodal object of this handle");
  ARGCHK(c, stride >= 1, "gpmi_unimodal_logpdf_sums: stride must be positive");
  ARGCHK(c, n_theta >= 1, "gpmi_unimodal_logpdf_sums: n_theta must be positive");
  ARGCHK(c, theta && out, "gpmi_unimodal_logpdf_sums: theta and out must be non-NULL");
  if (int rc = set_device(c)) return rc;
  KdeState* st = c->kde;
  // the partition, by n_fit alone
  const int64_t n_fit = (k->n + stride - 1) / stride;
  const int ipt = (int)std::max<int64_t>(1, (n_fit + 256 * (int64_t)UNI_MAXCHUNKS - 1) / (256 * (int64_t)UNI_MAXCHUNKS));
  const int64_t nchunks = (n_fit + 256 * (int64_t)ipt - 1) / (256 * (int64_t)ipt);
  const int per = (int)((nchunks + 255) / 256);
  const size_t part_bytes = kde_align256(8 * (size_t)nchunks * UNI_ARGS), out_bytes = kde_align256(8 * (size_t)n_theta);
  if (int rc = st->reserve_pinned(c, out_bytes)) return rc;
  if (int rc = st->reserve_work(c, part_bytes + out_bytes)) return rc;
  double* d_part = st->work();
  double* d_out = reinterpret_cast<double*>(st->d_work + part_bytes);
  UniTheta th;
  std::memset(&th, 0, sizeof(th));
  for (int t0 = 0; t0 < n_theta; t0 += UNI_ARGS) {
    const int nt = std::min(UNI_ARGS, n_theta - t0);
    for (int t = 0; t < nt; ++t) {
      std::memcpy(th.p[t], theta + 6 * (size_t)(t0 + t), 6 * sizeof(double));
      th.p[t][2] = std::exp(th.p[t][2]);
    }
    hipLaunchKernelGGL(unimodal_partial, dim3((unsigned)nchunks, (unsigned)nt), dim3(256), 0, st->stream, k->s, n_fit, stride,
                       ipt, th, nchunks, d_part);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(unimodal_finish, dim3((unsigned)nt), dim3(256), 0, st->stream, d_part, nchunks, per, d_out + t0);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(st->h_stage, d_out, 8 * (size_t)n_theta, hipMemcpyDeviceToHost, st->stream));
  HIPCHK(c, hipStreamSynchronize(st->stream));
  std::memcpy(out, st->h_stage, 8 * (size_t)n_theta);
  return GPMI_OK;
}

}  // extern "C"
