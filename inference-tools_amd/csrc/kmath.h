// exp and log1p for the covariance kernels (kbuild.hip): K = a^2 exp(-s) (SquaredExponential, covariance.py:254)
// and K = a^2 (1 + s / kappa)^-kappa = a^2 exp(-kappa log1p(s / kappa)) (RationalQuadratic, covariance.py:348), evaluated
// for the N^2 elements of every covariance build.
//
// Why not the library's exp / pow: inlined once per element they re-materialise their 64-bit constants with two
// v_mov_b32 each at every use (323 v_mov_b32 for the 16 elements of a thread - as many VALU slots as the arithmetic),
// and pow() is ~300 instructions per element.  Here a thread's elements are evaluated in LOCKSTEP (N at a time, the
// coefficient loop outermost), so a coefficient is fetched once per N FMAs, and the power is one log1p + one exp.
//
// Accuracy (tools/kmath_check.cpp, against long double on the host, 10^7 arguments each): see the numbers that program
// prints - exp_neg and log1p_pos within 1 ulp, the RationalQuadratic power within a few 1e-16 x (1 + kappa log1p(s / kappa))
// relative; the tests hold K to 1e-13 of the reference's NumPy values.
// Plain fma / rint / ldexp / frexp arithmetic: the same source compiles for the host check.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define KMATH_HD __host__ __device__ __forceinline__
#else
#define KMATH_HD inline
#endif

namespace kmath {

// seed of a reciprocal (v_rcp_f64: ~2^-26 relative; the host check takes the exact quotient - the Newton steps behind it
// make the result insensitive to the seed)
KMATH_HD double rcp_seed(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcp(d);
#else
  return 1.0 / d;
#endif
}
// a / d to within an ulp without the IEEE division sequence (v_div_scale / v_div_fmas / v_div_fixup: 12 instructions
// and three scalar-mask dependencies per quotient): two Newton steps on the reciprocal, one correction of the quotient.
// d in [1.7, 2.5] here, a of moderate size: no scaling needed.
KMATH_HD double div_newton(double a, double d) {
  double y = rcp_seed(d);
  y = fma(fma(-d, y, 1.0), y, y);
  y = fma(fma(-d, y, 1.0), y, y);
  const double q = a * y;
  return fma(fma(-d, q, a), y, q);
}

// exp(x) = p 2^n for x <= 0 (any finite x): x = n ln2 + r, |r| <= ln2 / 2, p the Taylor polynomial of degree 13 in Horner
// form on r.  The two parts are handed out separately for callers that multiply p before scaling (matern_profile: one
// rounding in the subnormal range instead of a rounded exp times a large factor).
template <int N>
KMATH_HD void exp_neg_parts(const double (&x)[N], double (&p)[N], double (&n)[N]) {
  const double LOG2E = 1.4426950408889634074;
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const double C[14] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0,
                        1.0 / 40320.0,      1.0 / 5040.0,      1.0 / 720.0,      1.0 / 120.0,     1.0 / 24.0,
                        1.0 / 6.0,          0.5,               1.0,              1.0};
  double r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double xc = x[i] < -1000.0 ? -1000.0 : x[i];
    n[i] = rint(xc * LOG2E);
    r[i] = fma(-n[i], LN2_HI, xc);
    r[i] = fma(-n[i], LN2_LO, r[i]);
    p[i] = C[0];
  }
#pragma unroll
  for (int k = 1; k < 14; ++k) {
    const double c = C[k];
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = fma(p[i], r[i], c);
  }
}

// exp(x) for x <= 0 (any finite x; x < -745.2 gives 0): the polynomial of exp_neg_parts scaled by 2^n.
template <int N>
KMATH_HD void exp_neg(const double (&x)[N], double (&out)[N]) {
  double n[N], p[N];
  exp_neg_parts(x, p, n);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = ldexp(p[i], (int)n[i]);
}

// log1p(z) for z >= 0:  u = fl(1 + z), c = (1 + z) - u exactly; log1p(z) = log(u) + c / u.
// log(u): u = 2^e m, m in [sqrt(1/2), sqrt(2)); f = m - 1, t = f / (2 + f), log(m) = f - (hfsq - t (hfsq + R)),
// hfsq = f^2 / 2, R = t^2 (L1 + t^2 (L2 + ...)) - the classic fdlibm arrangement.
template <int N>
KMATH_HD void log1p_pos(const double (&z)[N], double (&out)[N]) {
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const double L[7] = {1.479819860511658591e-01, 1.531383769920937332e-01, 1.818357216161805012e-01,
                       2.222219843214978396e-01, 2.857142874366239149e-01, 3.999999999940941908e-01,
                       6.666666666666735130e-01};
  double f[N], t[N], w[N], R[N], corr[N], ke[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double u = 1.0 + z[i];
    // rounding error of 1 + z (Fast2Sum with the larger operand first)
    const double c = z[i] < 1.0 ? z[i] - (u - 1.0) : 1.0 - (u - z[i]);
    int e;
    double m = frexp(u, &e);  // m in [1/2, 1)
    if (m < 0.70710678118654752440) {
      m *= 2.0;
      e -= 1;
    }
    ke[i] = (double)e;
    f[i] = m - 1.0;
    t[i] = div_newton(f[i], 2.0 + f[i]);
    corr[i] = c * rcp_seed(u);  // a term of at most half an ulp of u: the seed's 26 bits are plenty
    w[i] = t[i] * t[i];
    R[i] = L[0];
  }
#pragma unroll
  for (int k = 1; k < 7; ++k) {
    const double c = L[k];
#pragma unroll
    for (int i = 0; i < N; ++i) R[i] = fma(R[i], w[i], c);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double hfsq = 0.5 * f[i] * f[i];
    const double Rw = R[i] * w[i];
    // log(u) + c / u = e ln2_hi + (f - (hfsq - (t (hfsq + R) + (e ln2_lo + c / u))))
    const double lo = fma(t[i], hfsq + Rw, fma(ke[i], LN2_LO, corr[i]));
    out[i] = fma(ke[i], LN2_HI, f[i] - (hfsq - lo));
  }
}

// Matern covariance profiles of half-integer order nu = TWO_NU / 2 (3/2 or 5/2) in the builders' variable
// s = 1/2 sum_k dx_k^2 / l_k^2 (>= 0):  t = sqrt(2 nu) r = sqrt(4 nu s),
//   TWO_NU = 3:  C = (1 + t) e^-t              g = 3 e^-t
//   TWO_NU = 5:  C = (1 + t + t^2 / 3) e^-t    g = 5/3 (1 + t) e^-t
// C is the value profile (K = a^2 C) and g the derivative profile: dK / d ln l_k = a^2 g dx_k^2 / l_k^2 and
// dK(q, x) / dq_k = a^2 g (x - q)_k / l_k^2 - no division by r, finite and correct at coincident points.
// s = 0 gives C = 1 exactly (t = 0, e^0 = 1 x 2^0); t is held at 1000, far beyond the underflow of exp (745.2), so an
// overflowed s gives 0 x finite = 0.0 and never inf x 0.
// Accuracy (tools/kmath_matern_check.cpp, against long double, 10^7 values of s log-uniform over [1e-30, 1e5]): the
// relative errors stay within (8 + 2 t) 2^-53 - t carries <= 1 ulp, which exp turns into t ulp plus its own 1 ulp, the
// polynomial factor and the product add <= 3 ulp.  Measured maxima of err / ((8 + 2 t) 2^-53):
//   Matern32  C 0.74  g 0.74      Matern52  C 0.74  g 0.74   (attained at small t, where the bound is 8 x 2^-53)
template <int TWO_NU, int N>
KMATH_HD void matern_profile(const double (&s)[N], double (&C)[N], double (&g)[N]) {
  static_assert(TWO_NU == 3 || TWO_NU == 5, "Matern 3/2 and 5/2 only");
  double t[N], x[N], p[N], n[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double r = sqrt((2.0 * TWO_NU) * s[i]);
    t[i] = r > 1000.0 ? 1000.0 : r;
    x[i] = -t[i];
  }
  exp_neg_parts(x, p, n);  // e^-t = p 2^n, scaled after the polynomial factor
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (TWO_NU == 3) {
      C[i] = ldexp((1.0 + t[i]) * p[i], (int)n[i]);
      g[i] = ldexp(3.0 * p[i], (int)n[i]);
    } else {
      C[i] = ldexp(fma(t[i], fma(t[i], 1.0 / 3.0, 1.0), 1.0) * p[i], (int)n[i]);
      g[i] = ldexp((5.0 / 3.0) * ((1.0 + t[i]) * p[i]), (int)n[i]);
    }
  }
}

// sin^2(pi u) for the Periodic kernel's warped distance w = 2 sin^2(pi dx / p): u is the separation in units of the
// period, so the reduction r = u - rint(u), |r| <= 1/2, is exact (no Payne-Hanek, no multiple of pi subtracted), and
// sin^2 has period 1 in u.  |r| is then folded about 1/4 - t = |r| for |r| <= 1/4 and t = 1/2 - |r| beyond (exact:
// Sterbenz) - and sin(pi t) = t (pi + t^2 Q(t^2)) is the Taylor polynomial of degree 17 on |t| <= 1/4 (next term
// 1.2e-19 relative), pi carried as PI_HI + PI_LO so that the leading product rounds once.  The result is sin^2 = S^2 on
// the near side and cos^2 = 1 - S^2 (one fma) on the far side: the polynomial's correction is at most 11% of S on
// |t| <= 1/4, where a polynomial of sin^2 in r^2 over the whole of |r| <= 1/2 cancels 2.5 against 1.5.  The two
// sides are selects, the coefficient loop is outermost: N elements go through in lockstep, as in exp_neg_parts.
//   r = 0 gives exactly 0; |r| = 1/2 (either tie of rint) gives t = 0 and exactly 1; NaN stays NaN.
//   |u| >= 2^51 gives r = 0 (result 0): from 2^52 on every double is an integer, and in [2^51, 2^52) the spacing of
//   the doubles is the half period itself - there is no phase left to evaluate.  This includes u = +-inf (a period that
//   underflowed against a separation that did not).
// Accuracy (tools/kmath_periodic_check.cpp, against long double, r exact): S carries <= 1.5 x 2^-53 relative, the
// square or the fma <= 4 x 2^-53 at |r| = 1/4 and less elsewhere; bound 4 x 2^-53.  Measured maxima of err / (4 x 2^-53):
//   10^7 r uniform in [-1/2, 1/2] 0.77   10^6 r log-uniform over [1e-300, 1/2] 0.74   whole periods added: the same bits
template <int N>
KMATH_HD void sinpi_sq(const double (&u)[N], double (&out)[N]) {
  const double PI_HI = 3.141592653589793116, PI_LO = 1.2246467991473532e-16;
  // (-1)^n pi^(2n+1) / (2n+1)!, n = 8 .. 1
  const double Q[8] = {7.952054001475513e-07,  -2.1915353447830217e-05, 0.00046630280576761255, -0.0073704309457143504,
                       0.08214588661112823,    -0.5992645293207921,     2.5501640398773455,     -5.16771278004997};
  double t[N], w[N], q[N];
  bool far[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double r = fabs(u[i]) >= 2251799813685248.0 ? 0.0 : fabs(u[i] - rint(u[i]));
    far[i] = r > 0.25;
    t[i] = far[i] ? 0.5 - r : r;
    w[i] = t[i] * t[i];
    q[i] = Q[0];
  }
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const double c = Q[k];
#pragma unroll
    for (int i = 0; i < N; ++i) q[i] = fma(q[i], w[i], c);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double S = fma(t[i], PI_HI, t[i] * fma(w[i], q[i], PI_LO));
    out[i] = far[i] ? fma(-S, S, 1.0) : S * S;
  }
}

}  // namespace kmath
