"""
Timings of sums of stationary kernels (GPMI_KERNEL_SUM) against the single-kernel path, the mixture entry points with
unit window weights (the same model through per-component builds) and the dense host-composition path.

    python tools/sum_time.py [--reps 5] [--sizes 4096,8192,16384] [--json out.json]

Every figure is the median of `reps` device-synchronised calls after one warm-up call (each entry point synchronises
its stream before it returns).  Rows: fit, LML and LML + gradient of SE + RQ and of RQ alone at N = 4096, 8192, 16384
(d = 8); fit / LML / LML + gradient through gpmi_*_mix with all weights 1 at N = 8192; and the LML + gradient of the
dense path (the sum's host-built K and gradient matrices, what GpRegressor did before the fused path) at N = 4096;
the lockstep batches (64 evaluations of LML and of LML + gradient at N = 2048, the batched fused kernels).
Kernel times of the fused build and contraction: run under `rocprofv3 --kernel-trace --stats -- python tools/sum_time.py
--sizes 8192 --no-dense` in a command of its own and read ksum_kernel / sum_grad_kernel from the stats.
"""
import argparse
import json
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

D = 8


def med(fn, reps):
    fn()  # warm-up (allocations, first launches)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def thetas():
    th_se = np.concatenate([[0.2], np.log(np.linspace(0.8, 1.6, D))])
    th_rq = np.concatenate([[-0.5, 0.3], np.log(np.linspace(0.3, 0.6, D))])
    return th_se, th_rq


def time_size(n, reps, rows, mix=False, dense=False):
    x, y, e = wl.synthetic_dataset(3, n, D)
    mu = np.full(n, float(np.mean(y)))
    th_se, th_rq = thetas()
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        eng.set_sum([_lib.KERNEL_SE, _lib.KERNEL_RQ])
        th = np.concatenate([th_se, th_rq])
        for name, kid, t in (("SE+RQ", _lib.KERNEL_SUM, th), ("RQ", _lib.KERNEL_RQ, th_rq)):
            rows.append({"model": name, "n": n, "what": "fit", "ms": med(lambda: eng.fit(kid, t, 0.0, mu), reps)})
            rows.append({"model": name, "n": n, "what": "lml", "ms": med(lambda: eng.lml(kid, t, 0.0, mu), reps)})
            rows.append({"model": name, "n": n, "what": "lml+grad", "ms": med(lambda: eng.lml_grad(kid, t, 0.0, mu), reps)})
        if mix:
            ks, g = [_lib.KERNEL_SE, _lib.KERNEL_RQ], np.ones((2, n))
            name = "SE+RQ mix(ones)"
            rows.append({"model": name, "n": n, "what": "fit",
                         "ms": med(lambda: eng.fit_mix(ks, [th_se, th_rq], g, 0.0, mu), reps)})
            rows.append({"model": name, "n": n, "what": "lml",
                         "ms": med(lambda: eng.lml_mix(ks, [th_se, th_rq], g, 0.0, mu), reps)})
            rows.append({"model": name, "n": n, "what": "lml+grad",
                         "ms": med(lambda: eng.lml_grad_mix(ks, [th_se, th_rq], g, 0.0, mu), reps)})
    finally:
        eng.close()
    if dense:
        # the path GpRegressor took for a sum before the fused one: per-component device builds downloaded and added on
        # the host, the gradient from the components' dense N x N matrices contracted on the host with K^-1
        from inference_amd.gp import GpRegressor, RationalQuadratic, SquaredExponential

        hp = np.concatenate([[float(np.mean(y))], th_se, th_rq])
        gp = GpRegressor(x, y, y_err=e, kernel=SquaredExponential() + RationalQuadratic(), hyperpars=hp)
        gp._generic = True  # force the plugin (dense) path of the same model
        gp._mix = None
        rows.append({"model": "SE+RQ dense path", "n": n, "what": "lml+grad",
                     "ms": med(lambda: gp.marginal_likelihood_gradient(hp), max(1, reps // 2))})


def time_lockstep(n, T, reps, rows):
    """The lockstep batches (N <= 4096: the fused sum build / contraction over blockIdx.z): T evaluations per call."""
    x, y, e = wl.synthetic_dataset(3, n, D)
    th_se, th_rq = thetas()
    rng = np.random.default_rng(1)
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        eng.set_sum([_lib.KERNEL_SE, _lib.KERNEL_RQ])
        mc = np.full(T, float(np.mean(y)))
        for name, kid, t in (("SE+RQ", _lib.KERNEL_SUM, np.concatenate([th_se, th_rq])), ("RQ", _lib.KERNEL_RQ, th_rq)):
            ths = t[None, :] + 0.01 * rng.standard_normal((T, t.size))
            ex = np.zeros(T)
            rows.append({"model": name, "n": n, "what": f"lml x{T}",
                         "ms": med(lambda: eng.lml_batch(kid, ths, ex, mu_const=mc), reps)})
            rows.append({"model": name, "n": n, "what": f"grad x{T}",
                         "ms": med(lambda: eng.lml_grad_batch(kid, ths, ex, mu_const=mc), reps)})
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,8192,16384")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--no-lockstep", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        time_size(n, a.reps, rows, mix=(n == 8192), dense=(n == 4096 and not a.no_dense))
    if not a.no_lockstep:
        time_lockstep(2048, 64, a.reps, rows)
    for r in rows:
        print(f"{r['model']:>18s}  N={r['n']:6d}  {r['what']:>9s}  {r['ms']:9.3f} ms")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
