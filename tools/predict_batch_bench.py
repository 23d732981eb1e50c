"""
End-to-end time of `GpRegressor.predict_marginalised` (gpmi_predict_batch) beside the loop it replaces.

    python tools/predict_batch_bench.py [--reps 3] [--tiny] [--out profiles/r13_predict_batch.txt] [--json out.json]

The workload: SE, N = 2048, d = 8, T = 512 hyper-parameter vectors around the timing hyper-parameters, m = 1024 points.
Timed, each after one discarded run and as the median of `reps` runs, in one process:
  batch        predict_marginalised(points, thetas): mean and standard deviation of the mixture
  batch means  predict_marginalised(points, thetas, mean_only=True): no inverse factor, no product, no square sums
  loop         for theta in thetas: set_hyperparameters(theta); gp(points)  - followed by the host mixture and the re-fit at
               the original hyper-parameters: the only way to the same result without the batched entry point
and the largest relative difference between the two results.  `--tiny` runs a small problem (the smoke run of this tool).
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
from inference_amd.gp import GpRegressor, SquaredExponential  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, d, T, m = (128, 2, 8, 64) if a.tiny else (2048, 8, 512, 1024)

    x, y, e = wl.synthetic_dataset(5, n, d)
    theta0 = wl.timing_theta(wl.SE, y, d)
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta0, kernel=SquaredExponential)
    thetas = theta0 + 0.05 * np.random.default_rng(13).normal(size=(T, theta0.size))
    points = wl.query_points(5, m, d)

    def loop():
        saved = gp.hyperpars
        means, variances = np.empty((T, m)), np.empty((T, m))
        try:
            for t, theta in enumerate(thetas):
                gp.set_hyperparameters(theta)
                mu, sd = gp(points)
                means[t], variances[t] = mu, sd**2
        finally:
            gp.set_hyperparameters(saved)
        mean = means.mean(axis=0)
        return mean, np.sqrt((variances + (means - mean) ** 2).mean(axis=0))

    def timed(fn):
        out, ts = None, []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if rep:
                ts.append(dt)
        return out, ts

    (b_mean, b_std), t_batch = timed(lambda: gp.predict_marginalised(points, thetas))
    b_only, t_means = timed(lambda: gp.predict_marginalised(points, thetas, mean_only=True))
    (l_mean, l_std), t_loop = timed(loop)

    def rel(u, v):
        return float(np.abs(u - v).max() / np.abs(v).max())

    med = {k: float(np.median(v)) for k, v in (("batch", t_batch), ("batch_means", t_means), ("loop", t_loop))}
    lines = [
        f"# tools/predict_batch_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: SE, N = {n}, d = {d}, T = {T} "
        f"hyper-parameter vectors, m = {m} points; medians of {a.reps} runs after one discarded, one process",
        f"batch        {med['batch'] * 1e3:10.1f} ms   predict_marginalised (mean and standard deviation): "
        f"{T / med['batch']:.0f} vectors / s",
        f"batch means  {med['batch_means'] * 1e3:10.1f} ms   predict_marginalised(mean_only=True): {T / med['batch_means']:.0f} vectors / s",
        f"loop         {med['loop'] * 1e3:10.1f} ms   set_hyperparameters + __call__ per vector, host mixture, re-fit: "
        f"{T / med['loop']:.0f} vectors / s",
        f"loop / batch {med['loop'] / med['batch']:10.2f}",
        f"batch against loop: mean {rel(b_mean, l_mean):.2e}, standard deviation {rel(b_std, l_std):.2e} (relative, max|a-b| / max|b|); "
        f"mean_only against batch: {rel(b_only, b_mean):.1e}",
    ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out = {"tool": "predict_batch_bench", "tiny": a.tiny, "reps": a.reps, "n": n, "d": d, "T": T, "m": m,
           "batch_s": t_batch, "batch_means_s": t_means, "loop_s": t_loop}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
