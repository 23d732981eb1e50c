"""
Timings of the Periodic device kernel next to SquaredExponential, all in one process:

    python tools/periodic_bench.py [--out profiles/r25_periodic.txt]

for SE, `Periodic([1])` (one periodic dimension of two) and `Periodic()` (both), at d = 2:

  * the square K-build at N = 16384 (HIP events around the build launches of one likelihood evaluation, the library's
    PROF_KBUILD class);
  * LML and LML + gradient at N = 8192 (wall time of the device-synchronised call);
  * `marginal_likelihood_batch` evaluations per second at N = 2048, 512 hyper-parameter vectors per call;
  * `spatial_derivatives_batch` at N = 4096, 1000 points.

Every figure is taken after one warm-up call and is the median of three.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as wl  # noqa: E402
from inference_amd import _lib  # noqa: E402
from inference_amd._engine import GpEngine  # noqa: E402
from inference_amd.gp import GpRegressor, Periodic, SquaredExponential  # noqa: E402

D = 2
# (name, kernel id, periodic dimensions or None for SE, a fresh covariance object)
KERNELS = [("SE", _lib.KERNEL_SE, None, SquaredExponential),
           ("Periodic([1])", _lib.KERNEL_PER, [1], lambda: Periodic(periodic_dims=[1])),
           ("Periodic()", _lib.KERNEL_PER, [0, 1], Periodic)]


def theta_of(dims):
    scales = np.log(np.linspace(0.8, 1.6, D))
    periods = [] if dims is None else np.log(np.linspace(1.3, 2.1, len(dims)))
    return np.concatenate([[0.2], scales, periods])


def med3(fn):
    fn()  # warm-up (allocations, first launches)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def kbuild_ms(eng, kid, dims, mu):
    def one():
        eng.profile_reset()
        eng.lml(kid, theta_of(dims), 0.0, mu)
        return eng.profile_read(_lib.PROF_KBUILD)["ms"]

    one()
    return float(np.median([one() for _ in range(3)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_periodic.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = 16384
    x, y, e = wl.synthetic_dataset(3, n, D)
    mu = np.full(n, float(np.mean(y)))
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        eng.profile_enable(2 << _lib.PROF_KBUILD)
        say(f"square K-build, N = {n}, d = {D} (HIP events around the build launches of one LML evaluation; median of 3)")
        for name, kid, dims, _ in KERNELS:
            if dims is not None:
                eng.set_periodic(dims)
            say(f"  {name:14s} {kbuild_ms(eng, kid, dims, mu):8.3f} ms")
        eng.profile_enable(0)
    finally:
        eng.close()

    n = 8192
    x, y, e = wl.synthetic_dataset(3, n, D)
    mu = np.full(n, float(np.mean(y)))
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        say(f"LML and LML + gradient, N = {n}, d = {D} (wall time of the synchronised call; median of 3)")
        for name, kid, dims, _ in KERNELS:
            if dims is not None:
                eng.set_periodic(dims)
            th = theta_of(dims)
            say(f"  {name:14s} lml {med3(lambda: eng.lml(kid, th, 0.0, mu)):8.3f} ms   "
                f"lml + gradient {med3(lambda: eng.lml_grad(kid, th, 0.0, mu)):8.3f} ms")
    finally:
        eng.close()

    n, T = 2048, 512
    x, y, e = wl.synthetic_dataset(3, n, D)
    say(f"marginal_likelihood_batch, N = {n}, d = {D}, {T} hyper-parameter vectors per call (median of 3)")
    rng = np.random.default_rng(1)
    for name, kid, dims, make in KERNELS:
        th = np.concatenate([[float(np.mean(y))], theta_of(dims)])
        gp = GpRegressor(x, y, y_err=e, kernel=make(), hyperpars=th)
        thetas = th[None, :] + 0.01 * rng.standard_normal((T, th.size))
        ms = med3(lambda: gp.marginal_likelihood_batch(thetas))
        say(f"  {name:14s} {ms:9.2f} ms per call   {T / ms * 1e3:9.0f} evaluations / s")
        gp.engine.close()

    n, m = 4096, 1000
    x, y, e = wl.synthetic_dataset(3, n, D)
    pts = wl.query_points(2, m, D)
    say(f"spatial_derivatives_batch, N = {n}, d = {D}, {m} points (median of 3)")
    for name, kid, dims, make in KERNELS:
        th = np.concatenate([[float(np.mean(y))], theta_of(dims)])
        gp = GpRegressor(x, y, y_err=e, kernel=make(), hyperpars=th)
        say(f"  {name:14s} {med3(lambda: gp.spatial_derivatives_batch(pts)):8.3f} ms")
        gp.engine.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
