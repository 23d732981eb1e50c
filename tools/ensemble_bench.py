"""
Throughput of `EnsembleSampler` (inference_amd.mcmc) on the batched device likelihood against bare `marginal_likelihood_batch`
calls.

    python tools/ensemble_bench.py [--reps 3] [--iterations 2] [--tiny] [--out profiles/r21_ensemble.txt] [--json out.json]

The model: SE, N = 2048, d = 8; the walkers start scattered around the timing theta and are bounded by `hp_bounds`.
  split      ONE ensemble of 1024 walkers with update="split": `advance(iterations)`, rounds of up to 512 rows
  lockstep   64 serial ensembles of 16 walkers through `advance_lockstep_ensembles`: rounds of 64 rows
  bare       `marginal_likelihood_batch` on 512 rows (walker positions), timed in the same process
Reported, as the median of `reps` runs after one discarded run: rows per second of each, the ratios to bare, and where the
time of a call goes - inside the batched calls, in the sampler / driver around them - and how full the rounds were (the
retry rounds of a half-sweep carry only the walkers that have not accepted yet).  `--tiny` runs a small problem (the smoke
run of this tool).
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
from inference_amd.mcmc import EnsembleSampler, advance_lockstep_ensembles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, d, big, n_small, small, bare_rows = (128, 2, 32, 4, 8, 16) if a.tiny else (2048, 8, 1024, 64, 16, 512)

    x, y, e = wl.synthetic_dataset(5, n, d)
    theta0 = wl.timing_theta(wl.SE, y, d)
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta0, kernel=SquaredExponential)
    bounds = (np.array([b[0] for b in gp.hp_bounds], dtype=float), np.array([b[1] for b in gp.hp_bounds], dtype=float))
    gp.batch_independent_values(True)

    inside = []  # (rows, seconds) of every batched call of the current run

    def batch(thetas):
        t0 = time.perf_counter()
        out = gp.marginal_likelihood_batch(thetas)
        inside.append((len(thetas), time.perf_counter() - t0))
        return out

    rng = np.random.default_rng(21)

    def scattered(walkers):
        return np.clip(theta0 + 0.05 * rng.normal(size=(walkers, theta0.size)), bounds[0] + 1e-3, bounds[1] - 1e-3)

    split = EnsembleSampler(None, scattered(big), bounds=bounds, display_progress=False, update="split",
                            batch_posterior=batch, seed=1)
    serial = [EnsembleSampler(None, scattered(small), bounds=bounds, display_progress=False, batch_posterior=batch,
                              seed=100 + k) for k in range(n_small)]

    def proposals(samplers):
        return int(sum(np.array(s.total_proposals).sum() for s in samplers))

    def timed(samplers, call):
        del inside[:]
        before = proposals(samplers)
        t0 = time.perf_counter()
        call()
        wall = time.perf_counter() - t0
        rows, device = proposals(samplers) - before, sum(s for _, s in inside)
        assert rows == sum(r for r, _ in inside)
        return {"rows": rows, "wall_s": wall, "rounds": len(inside), "in_batch_s": device, "host_s": wall - device,
                "mean_rows": rows / len(inside), "rows_per_s": rows / wall, "rows_per_s_in_batch": rows / device}

    runs = []
    for rep in range(a.reps + 1):
        run = {"split": timed([split], lambda: split.advance(a.iterations)),
               "lockstep": timed(serial, lambda: advance_lockstep_ensembles(serial, a.iterations, batch))}
        positions = split.walker_positions[:bare_rows]
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            gp.marginal_likelihood_batch(positions)
            ts.append(time.perf_counter() - t0)
        run["bare_per_s"] = len(positions) / min(ts)
        print(("discarded " if rep == 0 else f"run {rep}     ") + json.dumps(run), flush=True)
        if rep:
            runs.append(run)

    def med(case, key):
        return float(np.median([r[case][key] for r in runs]))

    bare = float(np.median([r["bare_per_s"] for r in runs]))
    lines = [
        f"# tools/ensemble_bench.py --reps {a.reps} --iterations {a.iterations}{' --tiny' if a.tiny else ''}: SE, N = {n}, d = {d}; "
        f"medians of {a.reps} runs after one discarded",
        f"bare       {bare:10.1f} rows / s of marginal_likelihood_batch on {bare_rows} rows",
    ]
    for case, what in (("split", f"one split ensemble of {big} walkers, advance"),
                       ("lockstep", f"{n_small} serial ensembles of {small} walkers, advance_lockstep_ensembles")):
        lines += [
            f"{case:10s} {med(case, 'rows_per_s'):10.1f} rows / s ({what}); ratio to bare {med(case, 'rows_per_s') / bare:.3f}",
            f"           {med(case, 'rows'):.0f} rows in {med(case, 'rounds'):.0f} rounds ({med(case, 'mean_rows'):.1f} rows per round), "
            f"{med(case, 'wall_s'):.2f} s: {med(case, 'in_batch_s'):.2f} s inside the batched calls, {med(case, 'host_s') * 1e3:.1f} ms around them "
            f"({med(case, 'host_s') / med(case, 'rounds') * 1e3:.2f} ms per round); rows / s inside the batched calls over bare "
            f"{med(case, 'rows_per_s_in_batch') / bare:.3f} (what thin rounds cost)",
        ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out = {"tool": "ensemble_bench", "tiny": a.tiny, "reps": a.reps, "iterations": a.iterations, "runs": runs}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
