"""
Timings of the Matern32 / Matern52 device kernels next to SquaredExponential and RationalQuadratic, all in one process:

    python tools/matern_bench.py [--out profiles/r14_matern.txt]

  * the square K-build at N = 16384, d = 8 (HIP events around the build launches of one likelihood evaluation, the
    library's PROF_KBUILD class) for SE, RQ, Matern32, Matern52;
  * LML and LML + gradient at N = 8192 (wall time of the device-synchronised call);
  * `marginal_likelihood_batch` evaluations per second at N = 2048, 512 hyper-parameter vectors per call;
  * `spatial_derivatives_batch` at N = 4096, 1000 points, for SE and Matern52.

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
from inference_amd.gp import GpRegressor, Matern32, Matern52, RationalQuadratic, SquaredExponential  # noqa: E402

D = 8
KERNELS = [("SE", _lib.KERNEL_SE, SquaredExponential), ("RQ", _lib.KERNEL_RQ, RationalQuadratic),
           ("Matern32", _lib.KERNEL_M32, Matern32), ("Matern52", _lib.KERNEL_M52, Matern52)]


def theta_of(kid):
    scales = np.log(np.linspace(0.8, 1.6, D))
    return np.concatenate([[0.2, 0.3], scales]) if kid == _lib.KERNEL_RQ else np.concatenate([[0.2], scales])


def med3(fn):
    fn()  # warm-up (allocations, first launches)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def kbuild_ms(eng, kid, mu):
    def one():
        eng.profile_reset()
        eng.lml(kid, theta_of(kid), 0.0, mu)
        return eng.profile_read(_lib.PROF_KBUILD)["ms"]

    one()
    return float(np.median([one() for _ in range(3)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_matern.txt"))
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
        for name, kid, _ in KERNELS:
            say(f"  {name:9s} {kbuild_ms(eng, kid, mu):8.3f} ms")
        eng.profile_enable(0)
    finally:
        eng.close()

    n = 8192
    x, y, e = wl.synthetic_dataset(3, n, D)
    mu = np.full(n, float(np.mean(y)))
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        say(f"LML and LML + gradient, N = {n}, d = {D} (wall time of the synchronised call; median of 3)")
        for name, kid, _ in KERNELS:
            th = theta_of(kid)
            say(f"  {name:9s} lml {med3(lambda: eng.lml(kid, th, 0.0, mu)):8.3f} ms   "
                f"lml + gradient {med3(lambda: eng.lml_grad(kid, th, 0.0, mu)):8.3f} ms")
    finally:
        eng.close()

    n, T = 2048, 512
    x, y, e = wl.synthetic_dataset(3, n, D)
    say(f"marginal_likelihood_batch, N = {n}, d = {D}, {T} hyper-parameter vectors per call (median of 3)")
    rng = np.random.default_rng(1)
    for name, kid, cls in KERNELS:
        th = np.concatenate([[float(np.mean(y))], theta_of(kid)])
        gp = GpRegressor(x, y, y_err=e, kernel=cls(), hyperpars=th)
        thetas = th[None, :] + 0.01 * rng.standard_normal((T, th.size))
        ms = med3(lambda: gp.marginal_likelihood_batch(thetas))
        say(f"  {name:9s} {ms:9.2f} ms per call   {T / ms * 1e3:9.0f} evaluations / s")
        gp.engine.close()

    n, m = 4096, 1000
    x, y, e = wl.synthetic_dataset(3, n, D)
    pts = wl.query_points(2, m, D)
    say(f"spatial_derivatives_batch, N = {n}, d = {D}, {m} points (median of 3)")
    for name, kid, cls in (KERNELS[0], KERNELS[3]):
        th = np.concatenate([[float(np.mean(y))], theta_of(kid)])
        gp = GpRegressor(x, y, y_err=e, kernel=cls(), hyperpars=th)
        say(f"  {name:9s} {med3(lambda: gp.spatial_derivatives_batch(pts)):8.3f} ms")
        gp.engine.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
