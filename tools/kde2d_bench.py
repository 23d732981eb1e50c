"""
Timings of the 2-D density estimator (inference_amd.pdf.KDE2D over csrc/kde2d.hip) and of matrix_plot_data.

    python tools/kde2d_bench.py [--reps 3] [--tiny] [--json out.json]

Rows (n = sample size; every figure is the median of `reps` runs after one warm-up run; every entry point synchronises
its stream before it returns, and the times include the transfers of the points and of the results):
  grid_50_<n>, grid_200_<n>   a 50 x 50 / 200 x 200 grid at n = 10^5 and 10^6: the factorised kernel (gpmi_kde2d_grid) and
                              the direct sum of the grid's points (gpmi_kde2d_eval) side by side (KDE2D.grid takes the
                              factorised kernel: this comparison is what decided it)
  eval_10k                    10^4 scattered points at n = 10^6 (gpmi_kde2d_eval)
  self_100k, self_1m          the density at every sample (gpmi_kde2d_self): `pairs` counts the 256 x 256 tile pairs its
                              skip rule keeps (the count the library returns), `nominal` is n^2
  matrix_6                    matrix_plot_data of 6 parameters at n = 10^5, "contour" and "hdi", end to end (no pair count)
The samples are two-Gaussian mixtures with correlated columns.  `--tiny` runs every row at a small size (the GPU test of
this tool).  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/kde2d_bench.py` in a command of
its own.
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

from inference_amd.pdf import KDE2D  # noqa: E402
from inference_amd.plotting import matrix_plot_data  # noqa: E402


def mixture(n, seed, columns=2):
    """`columns` columns of a two-component mixture; neighbouring columns are correlated."""
    rng = np.random.default_rng(seed)
    k = int(0.6 * n)
    z = rng.normal(size=(columns + 1, n))
    shift = np.where(np.arange(n) < k, 0.0, 3.0)
    scale = np.where(np.arange(n) < k, 1.0, 0.5)
    cols = [shift * (1 if c % 2 == 0 else -0.5) + scale * (0.8 * z[c] + 0.6 * z[c + 1]) for c in range(columns)]
    p = rng.permutation(n)
    return [c[p] for c in cols]


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def row(name, ms, pairs, extra="", nominal=None):
    rate = pairs / (ms * 1e-3) if pairs else 0.0
    nom = f"   (nominal {nominal:.3e} = {nominal / (ms * 1e-3):.3e}/s)" if nominal else ""
    print(f"{name:22s} {ms:10.3f} ms   {pairs:.3e} pairs   {rate:.3e} pairs/s{nom}   {extra}", flush=True)
    out = {"name": name, "ms": ms, "pairs": float(pairs), "pairs_per_s": rate}
    if nominal:
        out["nominal_pairs"] = float(nominal)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n_small, n_big, n_pts, g_small, g_big = (3000, 20_000, 500, 20, 70) if a.tiny else (100_000, 1_000_000, 10_000, 50, 200)
    rows = []
    pdfs = {}
    for n in (n_small, n_big):
        x, y = mixture(n, 1)
        ms, pdfs[n] = timed(lambda: KDE2D(x, y), a.reps)
        rows.append(row(f"create_{n}", ms, 0, "KDE2D(x, y): bandwidths, binning, upload"))

    for n in (n_small, n_big):
        pdf = pdfs[n]
        d = pdf._density
        for g in (g_small, g_big):
            gx = np.linspace(pdf.x.min(), pdf.x.max(), g)
            gy = np.linspace(pdf.y.min(), pdf.y.max(), g)
            X, Y = np.meshgrid(gx, gy)
            X, Y = X.ravel(), Y.ravel()
            ms_f, f = timed(lambda: d.grid_sums(gx, gy, pdf.q_x, pdf.q_y), a.reps)
            ms_d, s = timed(lambda: d.sums(X, Y, pdf.q_x, pdf.q_y), a.reps)
            worst = float(np.max(np.abs(f.ravel() - s) / np.maximum(s, 1e-300)))
            rows.append(row(f"grid_{g}_{n}_fact", ms_f, float(g) * g * n, "factorised (the kernel KDE2D.grid takes)"))
            rows.append(row(f"grid_{g}_{n}_direct", ms_d, float(g) * g * n,
                            f"direct; factorised is {ms_d / ms_f:.2f}x faster, max rel. difference {worst:.1e}"))

    pdf = pdfs[n_big]
    rng = np.random.default_rng(3)
    pa, pb = rng.uniform(pdf.x.min(), pdf.x.max(), n_pts), rng.uniform(pdf.y.min(), pdf.y.max(), n_pts)
    ms, _ = timed(lambda: pdf(pa, pb), a.reps)
    rows.append(row("eval_10k", ms, float(n_pts) * n_big, f"{n_pts} scattered points, n = {n_big}"))

    for name, n in (("self_100k", n_small), ("self_1m", n_big)):
        pdf = pdfs[n]
        ms, _ = timed(pdf.at_samples, a.reps)
        _, (done, total) = pdf._density.self_sums(pdf.q_x, pdf.q_y, count_tiles=True)
        rows.append(row(name, ms, done * 65536.0, f"n = {n}: {done} of {total} tile pairs kept ({done / total:.3f})",
                        nominal=float(n) ** 2))

    samples = mixture(n_small, 5, columns=6)
    for style in ("contour", "hdi"):
        ms, _ = timed(lambda: matrix_plot_data(samples, plot_style=style), a.reps)
        rows.append(row(f"matrix_6_{style}", ms, 0, f"6 parameters, 15 pairs, n = {n_small}, end to end"))

    line = {"tool": "kde2d_bench", "tiny": a.tiny, "reps": a.reps, "rows": rows}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
