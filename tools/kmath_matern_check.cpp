// Host-side accuracy check of kmath::matern_profile (csrc/kmath.h) against long double:
//   g++ -O2 -std=c++17 -mfma -ffp-contract=off -I inference-tools_amd/csrc tools/kmath_matern_check.cpp -o /tmp/kmath_matern_check && /tmp/kmath_matern_check
//
// The value profile C and the derivative profile g of Matern 3/2 and 5/2 at 10^7 values of s, log-uniform over
// [1e-30, 1e5], plus s = 0 and the underflow edge.  Exit status 1 if a relative error exceeds (8 + 2 t) 2^-53:
// t = sqrt(4 nu s) carries <= 1 ulp, exp turns that into t ulp plus its own 1 ulp, the polynomial factor and the product
// add <= 3 ulp, and the margin is about 2 x.  Where the true value is a subnormal double (t > 708) no double has that
// relative accuracy: there the same bound holds relative to the smallest normal double, plus the one subnormal quantum
// of the final rounding.  Also fails when C(0) != 1 or anything is NaN.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <random>

#include "kmath.h"

namespace {

struct Worst {
  double c = 0.0, g = 0.0;  // max of error / bound
  bool nan = false;
};

template <int TWO_NU>
void reference(double s, long double& C, long double& g, long double& t) {
  t = sqrtl((long double)(2.0 * TWO_NU) * (long double)s);
  const long double e = expl(-t);
  if (TWO_NU == 3) {
    C = (1.0L + t) * e;
    g = 3.0L * e;
  } else {
    C = (1.0L + t + t * t / 3.0L) * e;
    g = 5.0L / 3.0L * (1.0L + t) * e;
  }
}

// error of `got` as a fraction of the bound at this t
double scaled_err(double got, long double want, long double t) {
  const long double bound = (8.0L + 2.0L * t) * 0x1p-53L;
  const long double err = fabsl((long double)got - want);
  if (want >= (long double)DBL_MIN) return (double)(err / want / bound);
  return (double)(err / (bound * (long double)DBL_MIN + 0x1p-1074L));
}

template <int TWO_NU>
Worst sweep(int total) {
  std::mt19937_64 gen(TWO_NU);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double lo = std::log(1e-30), hi = std::log(1e5);
  Worst w;
  for (int n = 0; n < total; n += 8) {
    double s[8], C[8], g[8];
    for (int i = 0; i < 8; ++i) s[i] = std::exp(lo + (hi - lo) * U(gen));
    kmath::matern_profile<TWO_NU>(s, C, g);
    for (int i = 0; i < 8; ++i) {
      long double Cw, gw, t;
      reference<TWO_NU>(s[i], Cw, gw, t);
      if (std::isnan(C[i]) || std::isnan(g[i])) w.nan = true;
      w.c = std::fmax(w.c, scaled_err(C[i], Cw, t));
      w.g = std::fmax(w.g, scaled_err(g[i], gw, t));
    }
  }
  return w;
}

// s = 0, the underflow edge (subnormal values from t = 708; the last non-zero ones near t = 750) and far beyond it, an
// overflowed s included
template <int TWO_NU>
bool edges(Worst& w) {
  bool ok = true;
  double s[8], C[8], g[8];
  const double tt[8] = {0.0, 700.0, 708.0, 720.0, 744.0, 746.0, 1e4, INFINITY};
  for (int i = 0; i < 8; ++i) s[i] = tt[i] * tt[i] / (2.0 * TWO_NU);
  kmath::matern_profile<TWO_NU>(s, C, g);
  for (int i = 0; i < 8; ++i) {
    if (std::isnan(C[i]) || std::isnan(g[i])) w.nan = true;
    if (i >= 6 && (C[i] != 0.0 || g[i] != 0.0)) ok = false;  // far beyond the underflow: 0.0
    if (i >= 1 && i < 6) {
      long double Cw, gw, t;
      reference<TWO_NU>(s[i], Cw, gw, t);
      w.c = std::fmax(w.c, scaled_err(C[i], Cw, t));
      w.g = std::fmax(w.g, scaled_err(g[i], gw, t));
    }
  }
  if (C[0] != 1.0 || g[0] != (TWO_NU == 3 ? 3.0 : 5.0 / 3.0)) ok = false;
  std::printf("Matern%d2 edges: C(0) = %.17g g(0) = %.17g C(t=744) = %g C(t=746) = %g C(t=1e4) = %g C(s=inf) = %g\n", TWO_NU,
              C[0], g[0], C[4], C[5], C[6], C[7]);
  return ok;
}

}  // namespace

int main() {
  const int T = 10000000;
  Worst w3 = sweep<3>(T), w5 = sweep<5>(T);
  const bool e3 = edges<3>(w3), e5 = edges<5>(w5);
  std::printf("max error / ((8 + 2 t) 2^-53):  Matern32 C %.3f g %.3f   Matern52 C %.3f g %.3f\n", w3.c, w3.g, w5.c, w5.g);
  const bool ok = e3 && e5 && !w3.nan && !w5.nan && w3.c <= 1.0 && w3.g <= 1.0 && w5.c <= 1.0 && w5.g <= 1.0;
  return ok ? 0 : 1;
}
