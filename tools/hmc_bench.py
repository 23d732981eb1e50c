"""
Throughput of `advance_lockstep_hmc` (inference_amd.mcmc) against bare `marginal_likelihood_gradient_batch` calls.

    python tools/hmc_bench.py [--reps 3] [--steps 1] [--tiny] [--out profiles/r12_hmc.txt] [--json out.json]

The workload: SE, N = 2048, d = 8; 512 chains = 64 ladders x 8 temperatures (1 .. 20, geometric), every chain bounded by
the model's `hp_bounds`, `steps = 50` leapfrog steps per trajectory.  A timed run advances all chains by `--steps` HMC
steps in one `advance_lockstep_hmc` call and then lets every ladder propose its swaps.  Reported, as the median of `reps`
runs after one discarded run:
  lockstep   gradient evaluations per second through the driver (rows evaluated / wall time of the call)
  bare       evaluations per second of `marginal_likelihood_gradient_batch` on 512 rows (the chains' positions), same run
  ratio      lockstep / bare
and where the time of a round goes: inside the batched call, in the driver around it, and how full the rounds were (chains
make 45 .. 54 leapfrog steps and retry rejected trajectories, so the last rounds of a call carry few rows; a bare call
always carries 512).  `--tiny` runs a small problem (the smoke run of this tool).
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as wl  # noqa: E402
from inference_amd.gp import GpRegressor, SquaredExponential  # noqa: E402
from inference_amd.mcmc import HamiltonianChain, ParallelTempering, advance_lockstep_hmc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, d, n_ladders, n_temps, leapfrog = (128, 2, 2, 4, 8) if a.tiny else (2048, 8, 64, 8, 50)

    x, y, e = wl.synthetic_dataset(5, n, d)
    theta0 = wl.timing_theta(wl.SE, y, d)
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta0, kernel=SquaredExponential)
    bounds = (np.array([b[0] for b in gp.hp_bounds], dtype=float), np.array([b[1] for b in gp.hp_bounds], dtype=float))
    gp.batch_independent_values(True)

    def one(t):
        return gp.marginal_likelihood_gradient_batch(t[None, :])

    rng = np.random.default_rng(12)
    temps = np.geomspace(1.0, 20.0, n_temps)
    starts = np.clip(theta0 + 0.05 * rng.normal(size=(n_ladders, n_temps, theta0.size)), bounds[0] + 1e-3, bounds[1] - 1e-3)
    known = dict(zip((s.tobytes() for s in starts.reshape(-1, theta0.size)),
                     gp.marginal_likelihood_gradient_batch(starts.reshape(-1, theta0.size))[0]))

    def posterior(t):  # (the constructor asks for the value at the start: all starts were evaluated in one batch)
        value = known.get(t.tobytes())
        return float(one(t)[0][0] if value is None else value)

    ladders = []
    for lad in range(n_ladders):
        chains = []
        for k, T in enumerate(temps):
            ch = HamiltonianChain(posterior, starts[lad, k], grad=lambda t: one(t)[1][0], epsilon=0.02,
                                  temperature=float(T), bounds=bounds, display_progress=False)
            ch.rng = np.random.default_rng(1000 * lad + k)
            ch.steps = leapfrog
            chains.append(ch)
        ladder = ParallelTempering(chains, batch_value_and_grad=gp.marginal_likelihood_gradient_batch)
        ladder.rng = np.random.default_rng(50_000 + lad)
        ladder.pair_choice = random.Random(60_000 + lad).choice
        ladders.append(ladder)
    chains = [c for lad in ladders for c in lad.chains]

    inside = []  # (rows, seconds) of every batched call of the current run

    def batch(thetas):
        t0 = time.perf_counter()
        out = gp.marginal_likelihood_gradient_batch(thetas)
        inside.append((len(thetas), time.perf_counter() - t0))
        return out

    runs = []
    for rep in range(a.reps + 1):
        del inside[:]
        t0 = time.perf_counter()
        evals = advance_lockstep_hmc(chains, a.steps, batch)
        wall = time.perf_counter() - t0
        for lad in ladders:
            lad.swap()
        positions = np.array([c.get_last() for c in chains])
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            gp.marginal_likelihood_gradient_batch(positions)
            ts.append(time.perf_counter() - t0)
        bare = len(chains) / min(ts)
        device = sum(s for _, s in inside)
        run = {"evals": evals, "wall_s": wall, "rounds": len(inside), "in_batch_s": device, "driver_s": wall - device,
               "mean_rows": evals / len(inside), "lockstep_per_s": evals / wall, "bare_per_s": bare,
               "ratio": evals / wall / bare, "full_round_ratio": (evals / device) / bare,
               "epsilon_median": float(np.median([c.ES.epsilon for c in chains]))}
        print(("discarded " if rep == 0 else f"run {rep}     ") + json.dumps(run), flush=True)
        if rep:
            runs.append(run)

    def med(key):
        return float(np.median([r[key] for r in runs]))

    lines = [
        f"# tools/hmc_bench.py --reps {a.reps} --steps {a.steps}{' --tiny' if a.tiny else ''}: SE, N = {n}, d = {d}, "
        f"{len(chains)} chains ({n_ladders} ladders x {n_temps} temperatures), steps = {leapfrog}; medians of {a.reps} runs after one discarded",
        f"lockstep   {med('lockstep_per_s'):10.1f} gradient evaluations / s through advance_lockstep_hmc",
        f"bare       {med('bare_per_s'):10.1f} evaluations / s of marginal_likelihood_gradient_batch on {len(chains)} rows",
        f"ratio      {med('ratio'):10.3f}",
        f"per call   {med('evals'):10.0f} rows in {med('rounds'):.0f} rounds ({med('mean_rows'):.1f} rows per round of {len(chains)}), "
        f"{med('wall_s'):.2f} s: {med('in_batch_s'):.2f} s inside the batched calls, {med('driver_s') * 1e3:.1f} ms in the driver around them "
        f"({med('driver_s') / med('rounds') * 1e3:.2f} ms per round)",
        f"rows / s inside the batched calls over the bare rate: {med('full_round_ratio'):.3f} (what thin rounds cost)",
    ]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out = {"tool": "hmc_bench", "tiny": a.tiny, "reps": a.reps, "steps": a.steps, "runs": runs}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
