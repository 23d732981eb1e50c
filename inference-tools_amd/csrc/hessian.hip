// Kernels of the exact Hessian of the log-marginal likelihood (gpmi_lml_hessian, api_hessian.hip; gfx950).
//
// With D_i = dK / d theta_i, D_ij the second derivatives, G_i = K^-1 D_i, z_i = G_i alpha and Q = alpha alpha^T - K^-1,
//     H_ij = 1/2 sum_ab Q_ab (D_ij)_ab  -  (D_i alpha)^T z_j  +  1/2 tr(G_i G_j).
// Four stages on top of the gradient's K^-1 (mirrored to both triangles):
//   (a) hess_dbuild_kernel      the dense D_i of a group of parameters, on the tile body of the covariance builders
//                               (pair_tile.h) and their lockstep exp / log1p - HBM-write bound, 8 bytes per element and i;
//                               D_i alpha by the row-dot kernel of solve.hip
//   (b) G_i = K^-1 D_i          the fp64-MFMA GEMM of gemm_f64.hip (both operands symmetric: the NT form), z_i by row dots
//   (c) hess_pair_trace_kernel  T_ij = sum_ab G_i[a][b] G_j[b][a]: a workgroup owns a 64-row block of a, one i and four j;
//                               per 64-column block the tile of G_i is transposed through LDS once and multiplied with the
//                               four tiles of G_j read in their own row order, so every global read is coalesced.  One
//                               partial per (i, j, row block), summed in ascending order by hess_trace_sum_kernel
//   (d) hess_contract_kernel    1/2 sum Q o D_ij for the second-derivative profiles that are not multiples of first
//                               derivatives: like lml_grad_body it recomputes the profiles per lower 64 x 64 tile of K^-1
//                               and counts off-diagonal elements twice.  The length-scale block sum_ab W_ab q_k q_m is
//                               register-tiled: a thread keeps W q_k of its 4 x 4 elements and runs over m >= k; a sum
//                               costs one wave reduction, the four waves meet in an LDS slab with one barrier per 256
//                               sums.  Partials per tile, summed in a fixed order by hess_entry_sum_kernel.
// No atomics; every sum has an order fixed by (N, d, kernel), so a repeated call returns the same bits, and the grouping
// of the parameters (GPMI_HESS_GIB) does not change them either: a partial of (c) depends on its two matrices alone.
#include "api_internal.h"
#include "pair_tile.h"

namespace {

using pair_tile::KT;

// second-derivative profiles of eight elements.  With K = a^2 C(s), s = 1/2 sum_k q_k, q_k = dx_k^2 / l_k^2:
//   d2K / d ln l_k d ln l_m = a^2 (g2 q_k q_m - 2 delta_km g q_k)
//   SE        g2 = C
//   Matern32  g2 = 9 e^-t / t = 3 g / t, t = sqrt(6 s); exactly 0 at t = 0, where every q_k is 0 (never inf x 0)
//   Matern52  g2 = 25/3 e^-t = 5 g / (1 + t), t = sqrt(10 s)
//   RQ        F = 1 + s / kappa, A = kappa ln F - s / F:  g2 = C (1 + 1 / kappa) / F^2,
//             d2K / d ln kappa^2 = a^2 hkk, hkk = C (A^2 - A + s^2 / (kappa F^2)),
//             d2K / d ln kappa d ln l_k = a^2 hkl q_k, hkl = C (s / kappa - A F) / F^2
// (hkk = hkl = 0 for the other kernels).  C comes from the same lockstep exp / log1p as the builders' value.
template <int KERNEL>
__device__ __forceinline__ void second_profiles(const KParams& p, const double (&s)[8], double (&g2)[8], double (&hkk)[8],
                                                double (&hkl)[8]) {
  double C[8], g[8], h[8];
  kprofiles<KERNEL>(p, s, C, g, h);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hkk[i] = 0.0;
    hkl[i] = 0.0;
    if (KERNEL == GPMI_KERNEL_SE) {
      g2[i] = C[i];
    } else if (KERNEL == GPMI_KERNEL_M32) {
      const double r = sqrt(6.0 * s[i]);
      const double t = r > 1000.0 ? 1000.0 : r;
      g2[i] = t > 0.0 ? 3.0 * g[i] / t : 0.0;
    } else if (KERNEL == GPMI_KERNEL_M52) {
      const double r = sqrt(10.0 * s[i]);
      const double t = r > 1000.0 ? 1000.0 : r;
      g2[i] = 5.0 * g[i] / (1.0 + t);
    } else {
      const double ik = 1.0 / p.kappa;
      const double z = s[i] * ik, F = 1.0 + z;
      // h = -C A (kfun.h); where C has underflowed A is of no consequence
      const double A = C[i] > 0.0 ? -h[i] / C[i] : 0.0;
      const double iF2 = 1.0 / (F * F);
      g2[i] = C[i] * (1.0 + ik) * iF2;
      hkk[i] = C[i] * (A * A - A + s[i] * z * iF2);
      hkl[i] = C[i] * (z - A * F) * iF2;
    }
  }
}

// (a) D[m] = dK / d parameter (p0 + m): tile (blockIdx.y, blockIdx.x) of all cnt matrices.  The element (a, b) and the
// element (b, a) come from the same chain of fmas (the difference changes its sign, the square does not), so D is
// symmetric bit for bit.
template <int KERNEL>
__global__ __launch_bounds__(256) void hess_dbuild_kernel(KParams p, int n_theta, int p0, int cnt, const double* __restrict__ x,
                                                          int64_t n, double* __restrict__ D, int64_t ld, int64_t sMat) {
  extern __shared__ double hb_lds[];  // two panels of d x 64 doubles (64 KiB at d = 64, as the builders)
  const int tid = threadIdx.x, d = p.d;
  double* su = hb_lds;
  double* sv = hb_lds + d * KT;
  const int64_t i0 = (int64_t)blockIdx.y * KT, j0 = (int64_t)blockIdx.x * KT;
  pair_tile::stage_panels(su, x, i0, n, sv, x, j0, n, d);
  __syncthreads();
  const int ty = pair_tile::thread_row(tid), tx = pair_tile::thread_col(tid);
  double s[4][4], C[4][4], g[4][4], h[4][4];
  pair_tile::accumulate_s(p.inv_l2, d, su, sv, ty, tx, s);
  pair_tile::for_each_profile<KERNEL, true>(p, s, [&](int r, int c, double Cv, double gv, double hv) {
    C[r][c] = Cv;
    g[r][c] = gv;
    h[r][c] = hv;
  });
  constexpr int off = (KERNEL == GPMI_KERNEL_RQ) ? 2 : 1;
  for (int m = 0; m < cnt; ++m) {
    const int pi = p0 + m;  // (uniform)
    double* out = D + (int64_t)m * sMat;
    const int k = pi - off;
    const double il2 = (k >= 0 && k < d) ? p.inv_l2[k] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t gi = i0 + ty * 4 + r;
      double v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t gj = j0 + tx * 4 + c;
        double val = 0.0;
        if (gi < n && gj < n) {
          if (pi == n_theta) {  // ln sigma: 2 sigma^2 I
            val = (gi == gj) ? 2.0 * p.extra_diag : 0.0;
          } else if (pi == 0) {  // ln a: twice the a^2 part, jitter included, not the noise
            val = 2.0 * (p.a2 * ((gi == gj) ? C[r][c] + 1e-12 : C[r][c]));
          } else if (off == 2 && pi == 1) {  // ln kappa
            val = p.a2 * h[r][c];
          } else {  // ln l_k
            const double dx = su[k * KT + ty * 4 + r] - sv[k * KT + tx * 4 + c];
            val = p.a2 * g[r][c] * (dx * dx * il2);
          }
        }
        v[c] = val;
      }
      double* dst = out + gi * ld + j0 + tx * 4;
      *reinterpret_cast<d2_t*>(dst) = d2_t{v[0], v[1]};
      *reinterpret_cast<d2_t*>(dst + 2) = d2_t{v[2], v[3]};
    }
  }
}

// (c) blockIdx.x: the 64-row block ta; blockIdx.y = i * ceil(nB / 4) + jc: matrix i of GA against matrices 4 jc .. 4 jc + 3
// of GB, those with iA0 + i <= jB0 + j.  Thread (ty, tx) takes rows ty, ty + 4, .. of a tile of G_j (coalesced along tx)
// and the transposed elements of G_i from LDS (row stride 65: no bank conflicts).
__global__ __launch_bounds__(256) void hess_pair_trace_kernel(const double* __restrict__ GA, int iA0, int nA,
                                                              const double* __restrict__ GB, int jB0, int nB, int nt64,
                                                              int64_t ld, int64_t sMat, int PT, double* __restrict__ part) {
  __shared__ double t[64][65];
  __shared__ double red[4];
  const int ta = blockIdx.x;
  const int njc = (nB + 3) / 4;
  const int il = blockIdx.y / njc, jc = blockIdx.y - il * njc;
  const int gi = iA0 + il;
  bool valid[4];
  bool any = false;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int jl = jc * 4 + jj;
    valid[jj] = jl < nB && jB0 + jl >= gi;
    any = any || valid[jj];
  }
  if (!any) return;  // (uniform)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const double* Gi = GA + (int64_t)il * sMat;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int tb = 0; tb < nt64; ++tb) {
    for (int r = ty; r < 64; r += 4) t[r][tx] = Gi[((int64_t)ta * 64 + r) * ld + (int64_t)tb * 64 + tx];
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      if (!valid[jj]) continue;
      const double* Gj = GB + (int64_t)(jc * 4 + jj) * sMat + ((int64_t)tb * 64) * ld + (int64_t)ta * 64 + tx;
      double a = acc[jj];
      for (int r = ty; r < 64; r += 4) a = fma(Gj[(int64_t)r * ld], t[tx][r], a);  // G_j[b][a] G_i[a][b]
      acc[jj] = a;
    }
    __syncthreads();
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    if (!valid[jj]) continue;
    const double v = pair_tile::block_sum(acc[jj], red);
    if (threadIdx.x == 0) part[((int64_t)gi * PT + (jB0 + jc * 4 + jj)) * nt64 + ta] = v;
  }
}

// out[i PT + j] = sum_ta part[(i PT + j) nt64 + ta], i <= j, one chain in ascending ta
__global__ void hess_trace_sum_kernel(const double* __restrict__ part, int PT, int nt64, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= PT * PT) return;
  const int i = e / PT, j = e - i * PT;
  if (j < i) return;
  double s = 0.0;
  for (int ta = 0; ta < nt64; ++ta) s += part[(int64_t)e * nt64 + ta];
  out[e] = s;
}

// out[i nv + j] = U_i . V_j: thread-strided chains over the np values, then the block's tree
__global__ __launch_bounds__(256) void hess_dots_kernel(const double* __restrict__ U, const double* __restrict__ V, int nv,
                                                        int64_t np, int upper, double* __restrict__ out) {
  __shared__ double red[4];
  const int i = blockIdx.y, j = blockIdx.x;
  if (upper && j < i) return;
  const double* u = U + (int64_t)i * np;
  const double* v = V + (int64_t)j * np;
  double acc = 0.0;
  for (int64_t a = threadIdx.x; a < np; a += 256) acc = fma(u[a], v[a], acc);
  const double sum = pair_tile::block_sum(acc, red);
  if (threadIdx.x == 0) out[(int64_t)i * nv + j] = sum;
}

// (d) one partial per lower tile and entry: ws[tile * nent + e]
template <int KERNEL>
__global__ __launch_bounds__(256) void hess_contract_kernel(KParams p, const double* __restrict__ x, int64_t n,
                                                            const double* __restrict__ iK, int64_t ld,
                                                            const double* __restrict__ alpha, int nent,
                                                            double* __restrict__ ws) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti) return;
  extern __shared__ double hc_lds[];  // two panels of d x 64 doubles, then the slab of 256 sums x 4 waves
  const int tid = threadIdx.x, d = p.d, wave = tid >> 6, lane = tid & 63;
  double* su = hc_lds;
  double* sv = hc_lds + d * KT;
  double* slab = hc_lds + 2 * d * KT;
  const int64_t i0 = (int64_t)ti * KT, j0 = (int64_t)tj * KT;
  pair_tile::stage_panels(su, x, i0, n, sv, x, j0, n, d);
  __syncthreads();
  const int ty = pair_tile::thread_row(tid), tx = pair_tile::thread_col(tid);
  double s[4][4];
  pair_tile::accumulate_s(p.inv_l2, d, su, sv, ty, tx, s);
  // w2 = 1/2 * multiplicity * Q_ab * a^2 g2 (as lml_grad_body forms its weights); RQ: wkl with hkl, and the sum with hkk
  double w2[4][4], wkl[4][4];
  double skk = 0.0;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    double s8[8], g2[8], hkk[8], hkl[8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) s8[4 * r + c] = s[2 * hh + r][c];
    second_profiles<KERNEL>(p, s8, g2, hkk, hkl);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t ga = i0 + ty * 4 + 2 * hh + r;
      const double aa = (ga < n) ? alpha[ga] : 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t gb = j0 + tx * 4 + c;
        double w = 0.0;
        if (ga < n && gb <= ga) {
          const double q = aa * alpha[gb] - iK[ga * ld + gb];
          w = (ga == gb) ? 0.5 * q : q;
        }
        w *= p.a2;
        w2[2 * hh + r][c] = w * g2[4 * r + c];
        wkl[2 * hh + r][c] = w * hkl[4 * r + c];
        skk = fma(w, hkk[4 * r + c], skk);
      }
    }
  }
  const int64_t tile = (int64_t)ti * (ti + 1) / 2 + tj;
  double* out = ws + tile * nent;
  int cnt = 0, base = 0;
  auto flush = [&]() {
    __syncthreads();
    if (tid < cnt) out[base + tid] = (slab[tid * 4] + slab[tid * 4 + 1]) + (slab[tid * 4 + 2] + slab[tid * 4 + 3]);
    __syncthreads();
    base += cnt;
    cnt = 0;
  };
  auto emit = [&](double v) {  // (cnt and base are uniform: every thread takes every step)
    v = pair_tile::wave_sum(v);
    if (lane == 0) slab[cnt * 4 + wave] = v;
    if (++cnt == 256) flush();
  };
  for (int k = 0; k < d; ++k) {
    const double ilk = p.inv_l2[k];
    double wq[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double dx = su[k * KT + ty * 4 + r] - sv[k * KT + tx * 4 + c];
        wq[r][c] = w2[r][c] * (dx * dx * ilk);
      }
    for (int m = k; m < d; ++m) {
      double ur[4], vc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ur[r] = su[m * KT + ty * 4 + r];
#pragma unroll
      for (int c = 0; c < 4; ++c) vc[c] = sv[m * KT + tx * 4 + c];
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double dx = ur[r] - vc[c];
          acc = fma(wq[r][c], dx * dx, acc);
        }
      emit(acc * p.inv_l2[m]);
    }
  }
  if (KERNEL == GPMI_KERNEL_RQ) {
    for (int k = 0; k < d; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double dx = su[k * KT + ty * 4 + r] - sv[k * KT + tx * 4 + c];
          acc = fma(wkl[r][c], dx * dx, acc);
        }
      emit(acc * p.inv_l2[k]);
    }
    emit(skk);
  }
  if (cnt) flush();
}

// out[e] = sum over tiles of ws[tile * nent + e]: thread-strided chains, then the block's tree
__global__ __launch_bounds__(256) void hess_entry_sum_kernel(const double* __restrict__ ws, int64_t ntiles, int nent,
                                                             double* __restrict__ out) {
  __shared__ double red[4];
  const int e = blockIdx.x;
  double acc = 0.0;
  for (int64_t t = threadIdx.x; t < ntiles; t += 256) acc += ws[t * nent + e];
  const double v = pair_tile::block_sum(acc, red);
  if (threadIdx.x == 0) out[e] = v;
}

size_t contract_lds_bytes(int d) { return sizeof(double) * (2 * (size_t)d * KT + 4 * 256); }

}  // namespace

void launch_hess_dbuild(hipStream_t s, const KParams& p, int n_theta, int p0, int cnt, const double* x, int64_t n, int64_t np,
                        double* D, int64_t ld, int64_t sMat) {
  const dim3 grid((unsigned)(np / KT), (unsigned)(np / KT));
  const size_t lds = sizeof(double) * 2 * (size_t)p.d * KT;
  with_stationary_kernel(p.kernel, [&](auto K) {
    hipLaunchKernelGGL(hess_dbuild_kernel<decltype(K)::value>, grid, dim3(256), lds, s, p, n_theta, p0, cnt, x, n, D, ld, sMat);
  });
}

void launch_hess_pair_trace(hipStream_t s, const double* GA, int iA0, int nA, const double* GB, int jB0, int nB, int64_t np,
                            int64_t ld, int64_t sMat, int PT, double* part) {
  const int nt64 = (int)(np / 64);
  const dim3 grid((unsigned)nt64, (unsigned)(nA * ((nB + 3) / 4)));
  hipLaunchKernelGGL(hess_pair_trace_kernel, grid, dim3(256), 0, s, GA, iA0, nA, GB, jB0, nB, nt64, ld, sMat, PT, part);
}

void launch_hess_trace_sum(hipStream_t s, const double* part, int PT, int64_t np, double* out) {
  hipLaunchKernelGGL(hess_trace_sum_kernel, dim3((unsigned)((PT * PT + 255) / 256)), dim3(256), 0, s, part, PT, (int)(np / 64),
                     out);
}

void launch_hess_dots(hipStream_t s, const double* U, int nu, const double* V, int nv, int64_t np, bool upper, double* out) {
  hipLaunchKernelGGL(hess_dots_kernel, dim3((unsigned)nv, (unsigned)nu), dim3(256), 0, s, U, V, nv, np, upper ? 1 : 0, out);
}

int hess_contract_entries(int kernel, int d) { return d * (d + 1) / 2 + (kernel == GPMI_KERNEL_RQ ? d + 1 : 0); }

int64_t hess_contract_ws_doubles(int64_t np, int kernel, int d) {
  const int64_t t = np / KT;
  return t * (t + 1) / 2 * hess_contract_entries(kernel, d);
}

int launch_hess_contract(gpmi_ctx* c, hipStream_t s, const KParams& p, const double* x, int64_t n, int64_t np, const double* iK,
                         int64_t ld, const double* alpha, double* ws, double* out) {
  const int64_t t = np / KT;
  const dim3 grid((unsigned)t, (unsigned)t);
  const int nent = hess_contract_entries(p.kernel, p.d);
  const size_t lds = contract_lds_bytes(p.d);
  int rc = GPMI_OK;
  with_stationary_kernel(p.kernel, [&](auto K) {
    auto kernel = hess_contract_kernel<decltype(K)::value>;
    if (lds > 65536) {  // above 64 KiB a kernel has to opt in first
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {
        c->err = std::string("hipFuncSetAttribute (hess_contract_kernel): ") + hipGetErrorString(e);
        rc = GPMI_ERR_HIP;
        return;
      }
    }
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, p, x, n, iK, ld, alpha, nent, ws);
  });
  if (rc != GPMI_OK) return rc;
  hipLaunchKernelGGL(hess_entry_sum_kernel, dim3((unsigned)nent), dim3(256), 0, s, ws, t * (t + 1) / 2, nent, out);
  return GPMI_OK;
}
