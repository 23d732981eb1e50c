// Host-side accuracy check of kmath::sinpi_sq (csrc/kmath.h) against long double:
//   g++ -O2 -std=c++17 -mfma -ffp-contract=off -I inference-tools_amd/csrc tools/kmath_periodic_check.cpp -o /tmp/kmath_periodic_check && /tmp/kmath_periodic_check
//
// sin^2(pi r) at 10^7 values of r uniform in [-1/2, 1/2], at 10^6 values log-uniform over [1e-300, 1/2] with random
// sign, at r = 0 and the ties r = +-1/2, and at whole periods added to r (the reduction).  r is exact, so the error is the
// function's own.  Exit status 1 if a relative error exceeds 4 x 2^-53 (kmath.h has the derivation: sin(pi t) on
// |t| <= 1/4 within 1.5 x 2^-53, squared or taken from 1 by one fma).  Where the true value is a subnormal double
// (|r| < 5e-155) no double has that relative accuracy: there the same bound holds relative to the smallest normal
// double, plus the one subnormal quantum of the final rounding.  Also fails when sinpi_sq(0) != 0, sinpi_sq(+-1/2) != 1,
// |u| >= 2^51 does not give 0, a NaN does not stay one, or anything else is NaN.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <random>

#include "kmath.h"

namespace {

constexpr long double BOUND = 4.0L * 0x1p-53L;
const long double PI_L = 3.14159265358979323846264338327950288L;

long double reference(double r) {
  const long double s = sinl(PI_L * (long double)r);
  return s * s;
}

// error of `got` as a fraction of the bound
double scaled_err(double got, long double want) {
  const long double err = fabsl((long double)got - want);
  if (want >= (long double)DBL_MIN) return (double)(err / want / BOUND);
  return (double)(err / (BOUND * (long double)DBL_MIN + 0x1p-1074L));
}

struct Worst {
  double err = 0.0, at = 0.0;
  bool nan = false;
  void take(double r, double got) {
    if (std::isnan(got)) nan = true;
    const double e = scaled_err(got, reference(r));
    if (e > err) {
      err = e;
      at = r;
    }
  }
};

template <class Draw>
Worst sweep(int total, Draw&& draw) {
  Worst w;
  for (int n = 0; n < total; n += 8) {
    double r[8], out[8];
    for (int i = 0; i < 8; ++i) r[i] = draw();
    kmath::sinpi_sq(r, out);
    for (int i = 0; i < 8; ++i) w.take(r[i], out[i]);
  }
  return w;
}

}  // namespace

int main() {
  std::mt19937_64 gen(5);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const Worst uni = sweep(10000000, [&] { return U(gen) - 0.5; });
  const double lo = std::log(1e-300), hi = std::log(0.5);
  const Worst lg = sweep(1000000, [&] {
    const double r = std::exp(lo + (hi - lo) * U(gen));
    return U(gen) < 0.5 ? -r : r;
  });
  // whole periods added: u = k + r is exact for r a multiple of 2^-20 and |k| < 2^30, and the result is that of r, bit for bit
  bool shift_ok = true;
  for (int n = 0; n < 100000; n += 8) {
    double r[8], u[8], a[8], b[8];
    for (int i = 0; i < 8; ++i) {
      r[i] = std::ldexp(std::floor(U(gen) * 1048576.0) - 524288.0, -20);
      u[i] = r[i] + std::floor((U(gen) - 0.5) * 2147483648.0);
    }
    kmath::sinpi_sq(r, a);
    kmath::sinpi_sq(u, b);
    for (int i = 0; i < 8; ++i) shift_ok = shift_ok && a[i] == b[i];
  }
  const double e[8] = {0.0, -0.0, 0.5, -0.5, 1.5, 0x1p51, -INFINITY, NAN};
  double out[8];
  kmath::sinpi_sq(e, out);
  const bool edges = out[0] == 0.0 && out[1] == 0.0 && out[2] == 1.0 && out[3] == 1.0 && out[4] == 1.0 && out[5] == 0.0 &&
                     out[6] == 0.0 && std::isnan(out[7]);
  std::printf("sinpi_sq edges: f(0) = %g f(1/2) = %.17g f(-1/2) = %.17g f(3/2) = %.17g f(2^51) = %g f(-inf) = %g f(nan) = %g\n",
              out[0], out[2], out[3], out[4], out[5], out[6], out[7]);
  std::printf("max error / (4 x 2^-53):  uniform %.3f (r = %.17g)   log-uniform %.3f (r = %.17g)   whole periods %s\n", uni.err,
              uni.at, lg.err, lg.at, shift_ok ? "exact" : "DIFFER");
  const bool ok = edges && shift_ok && !uni.nan && !lg.nan && uni.err <= 1.0 && lg.err <= 1.0;
  return ok ? 0 : 1;
}
