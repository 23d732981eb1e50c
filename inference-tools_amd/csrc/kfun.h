// Covariance functions of the stationary kernels, N elements at a time on the lockstep exp / log1p of kmath.h: the value
// profile the builders write (kbuild.hip) and, for the contraction of the sparse model (sparse.hip), value and derivative
// profiles together.  Device code only; internal.
#pragma once
#include "gpmi_internal.h"
#include "kmath.h"

// kinds of kfun beyond the public kernel ids: the Matern derivative profiles g (kmath.h: matern_profile; the cross build
// of a^2 g for the predictive-gradient kernels, launch_kbuild_cross_dprofile)
constexpr int KFUN_M32_G = 0x100 | GPMI_KERNEL_M32;
constexpr int KFUN_M52_G = 0x100 | GPMI_KERNEL_M52;

// Covariance function of N elements at once (kmath.h: a thread's elements go through exp / log1p in lockstep, so a
// polynomial coefficient is fetched once per N FMAs; the library's exp() inlined per element re-materialised its
// constants at every use - as many v_mov_b32 as arithmetic - and its pow() is ~300 instructions per element).
// KERNEL is a template parameter of the builders: one covariance function per kernel keeps the code within the
// instruction cache two CUs share.   s = sum_k 0.5 * dx_k^2 / l_k^2  (>= 0)
// GPMI_KERNEL_PER is SquaredExponential's exp of the warped s the caller formed (pair_tile.h: accumulate_s_periodic).
template <int KERNEL, int N>
__device__ inline void kfun(const KParams& p, const double (&s)[N], double (&out)[N]) {
  static_assert(KERNEL == GPMI_KERNEL_SE || KERNEL == GPMI_KERNEL_RQ || KERNEL == GPMI_KERNEL_M32 ||
                    KERNEL == GPMI_KERNEL_M52 || KERNEL == KFUN_M32_G || KERNEL == KFUN_M52_G || KERNEL == GPMI_KERNEL_PER,
                "kfun: no covariance function of this kind");
  if (KERNEL == GPMI_KERNEL_M32 || KERNEL == GPMI_KERNEL_M52 || KERNEL == KFUN_M32_G || KERNEL == KFUN_M52_G) {
    // Matern 3/2, 5/2: (1 + t) e^-t, (1 + t + t^2 / 3) e^-t with t = sqrt(4 nu s) - or their derivative profiles
    constexpr int TWO_NU = (KERNEL == GPMI_KERNEL_M32 || KERNEL == KFUN_M32_G) ? 3 : 5;
    double other[N];
    if (KERNEL == KFUN_M32_G || KERNEL == KFUN_M52_G)
      kmath::matern_profile<TWO_NU>(s, other, out);
    else
      kmath::matern_profile<TWO_NU>(s, out, other);
    return;
  }
  double e[N];
  if (KERNEL == GPMI_KERNEL_SE || KERNEL == GPMI_KERNEL_PER) {  // exp(-s)  (covariance.py:254; Periodic: of its own s)
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = -s[i];
  } else {  // GPMI_KERNEL_RQ: (1 + s / kappa)^-kappa = exp(-kappa log1p(s / kappa))  (covariance.py:348)
    const double ik = 1.0 / p.kappa;
    double z[N], l[N];
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = s[i] * ik;
    kmath::log1p_pos(z, l);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = -p.kappa * l[i];
  }
  kmath::exp_neg(e, out);
}

// Value and derivative profiles of N elements: with K = a^2 C,
//   dK / d ln l_k = a^2 g dx_k^2 / l_k^2     and, RationalQuadratic only,     dK / d ln kappa = a^2 h   (else h = 0)
//   SE, Periodic: g = C = e^-s;   RQ: F = 1 + s / kappa, C = F^-kappa, g = C / F, h = -C (kappa ln F - s / F)   (covariance.py:356-364);
//   Matern: C and g of kmath.h (matern_profile).  The same lockstep exp / log1p as kfun: C is bit for bit the builders' value.
template <int KERNEL, int N>
__device__ inline void kprofiles(const KParams& p, const double (&s)[N], double (&C)[N], double (&g)[N], double (&h)[N]) {
  static_assert(KERNEL == GPMI_KERNEL_SE || KERNEL == GPMI_KERNEL_RQ || KERNEL == GPMI_KERNEL_M32 ||
                    KERNEL == GPMI_KERNEL_M52 || KERNEL == GPMI_KERNEL_PER,
                "kprofiles: no covariance function of this kind");
  if (KERNEL == GPMI_KERNEL_M32 || KERNEL == GPMI_KERNEL_M52) {
    kmath::matern_profile<(KERNEL == GPMI_KERNEL_M32) ? 3 : 5>(s, C, g);
#pragma unroll
    for (int i = 0; i < N; ++i) h[i] = 0.0;
  } else if (KERNEL == GPMI_KERNEL_SE || KERNEL == GPMI_KERNEL_PER) {
    double e[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = -s[i];
    kmath::exp_neg(e, C);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      g[i] = C[i];
      h[i] = 0.0;
    }
  } else {
    const double ik = 1.0 / p.kappa;
    double z[N], l[N], e[N];
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = s[i] * ik;
    kmath::log1p_pos(z, l);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = -p.kappa * l[i];
    kmath::exp_neg(e, C);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double F = 1.0 + z[i];
      g[i] = C[i] / F;
      h[i] = -C[i] * (p.kappa * l[i] - s[i] / F);
    }
  }
}
