"""
Timings of the device density estimator (inference_amd.pdf.GaussianKDE over csrc/kde.hip).

    python tools/kde_bench.py [--reps 3] [--tiny] [--json out.json]

Rows (n = sample size; every figure is the median of `reps` runs after one warm-up run; every entry point synchronises
its stream before it returns):
  cv_20k         GaussianKDE(s, cross_validation=True) at n = 20 000 (default cap: a subsample of 5000), end to end
  cv_200k_50k    the same at n = 200 000 with max_cv_samples = 50 000
  cv_200k_200k   the same at n = 200 000 with max_cv_samples = 200 000 (every sample)
  pdfcdf_1m      pdf + cdf at 10^4 points on 10^6 samples: two calls, kde(x) and kde.cdf(x)
  build_1m       GaussianKDE(s) at 10^6 samples: region table, upload and the mode search
  interval_1m    kde.interval(0.95) at 10^6 samples (Nelder-Mead, one pdf + cdf call per cost evaluation)
Pair evaluations of the cross-validation: `pairs` counts those the kernel computes - per launch of up to 8 bandwidths,
the 256 x 256 tiles of the sorted sample that its skip test (every |x_i - x_j| > 38.6 h_max) does not drop, times the
launch's bandwidths - and `nominal` counts n_cv^2 per bandwidth; both are counted after the timed runs from the
requests of the last one.  Slice sums: the slice lengths of the points, once for the pdf and once for the cdf (no skip).
The samples are two-Gaussian mixtures.  `--tiny` runs every row at a small size (the GPU test of this tool).
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/kde_bench.py` in a command of its own.
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

from inference_amd.pdf import GaussianKDE  # noqa: E402
from inference_amd.pdf import _device  # noqa: E402
from inference_amd.pdf import kde as kde_mod  # noqa: E402

CV_TILE, CV_MAXH, CV_REACH = 256, 8, 38.6  # csrc/kde.hip
REQUESTS = []  # (samples, widths) of the cross-validation calls of the current run
_cv = _device.cv_logprob


def recorded_cv(samples, widths, c=0.99, device=None):
    REQUESTS.append((samples, widths))
    return _cv(samples, widths, c=c, device=device)


_device.cv_logprob = recorded_cv


def tile_pairs(s, reach):
    """Pairs in the 256 x 256 tiles of the sorted sample s that kde_cv_partial computes for this reach."""
    starts = np.arange(0, s.size, CV_TILE)
    lo, hi = s[starts], s[np.minimum(starts + CV_TILE, s.size) - 1]
    size = np.minimum(CV_TILE, s.size - starts).astype(np.float64)
    ok = (lo[None, :] - hi[:, None] <= reach) & (lo[:, None] - hi[None, :] <= reach)
    return float(size @ (ok @ size))


def cv_pairs():
    """(computed, nominal) pair-bandwidth evaluations of the recorded requests."""
    done = nominal = 0.0
    for samples, widths in REQUESTS:
        s = np.sort(np.asarray(samples, dtype=np.float64))
        w = np.asarray(widths, dtype=np.float64)
        w = w[np.isfinite(w) & (w > 0)]
        for k in range(0, w.size, CV_MAXH):
            chunk = w[k:k + CV_MAXH]
            done += chunk.size * tile_pairs(s, CV_REACH * chunk.max())
            nominal += chunk.size * float(s.size) ** 2
    return done, nominal


def mixture(n, seed):
    rng = np.random.default_rng(seed)
    k = int(0.6 * n)
    return np.concatenate([rng.normal(0.0, 1.0, k), rng.normal(3.0, 0.5, n - k)])


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        REQUESTS.clear()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def row(name, ms, pairs, extra="", nominal=None):
    rate = pairs / (ms * 1e-3) if pairs else 0.0
    nom = f"   (nominal {nominal:.3e} = {nominal / (ms * 1e-3):.3e}/s)" if nominal else ""
    print(f"{name:14s} {ms:10.3f} ms   {pairs:.3e} pairs   {rate:.3e} pairs/s{nom}   {extra}", flush=True)
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
    n_cv, n_big, n_pts, n_1m = (2000, 5000, 500, 20_000) if a.tiny else (20_000, 200_000, 10_000, 1_000_000)
    rows = []

    for name, n, cap in (("cv_20k", n_cv, 5000), ("cv_200k_50k", n_big, n_big // 4), ("cv_200k_200k", n_big, n_big)):
        s = mixture(n, 1)
        np.random.seed(0)
        ms, kde = timed(lambda: GaussianKDE(s, cross_validation=True, max_cv_samples=cap), a.reps)
        done, nominal = cv_pairs()
        rows.append(row(name, ms, done, f"n = {n}, max_cv_samples = {cap}, h = {kde.h:.6g}", nominal=nominal))

    s = mixture(n_1m, 2)
    ms, kde = timed(lambda: GaussianKDE(s), a.reps)
    rows.append(row("build_1m", ms, 0, f"n = {n_1m}, {kde.lwr_inds.size} regions, mode = {kde.mode:.6g}"))

    x = np.random.default_rng(3).uniform(kde.sample[0], kde.sample[-1], n_pts)
    r = kde_mod.region_of(kde.edges, kde.regions, x)
    slice_pairs = float(np.sum(kde.upr_inds[r] - kde.lwr_inds[r]))
    ms, _ = timed(lambda: (kde(x), kde.cdf(x)), a.reps)
    rows.append(row("pdfcdf_1m", ms, 2 * slice_pairs, f"{n_pts} points, mean slice {slice_pairs / n_pts:.0f} samples"))

    ms, iv = timed(lambda: kde.interval(0.95), a.reps)
    rows.append(row("interval_1m", ms, 0, f"interval(0.95) = ({iv[0]:.6g}, {iv[1]:.6g})"))

    line = {"tool": "kde_bench", "tiny": a.tiny, "reps": a.reps, "rows": rows}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
