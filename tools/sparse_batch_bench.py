"""
Lockstep batches of the sparse model (gpmi_sgp_bound_batch) next to a loop of single evaluations (gpmi_sgp_bound).

    python tools/sparse_batch_bench.py [--reps 3] [--tiny] [--limit 300] [--parent DIR] [--out profiles/r22_sparse_batch.txt]

Model and shapes of tools/sparse_bench.py: SquaredExponential + WhiteNoise, d = 8, inducing inputs a random subset of x,
N = 1e5, m in {512, 1024, 2048}; T in {1, 8, 32, 64} hyper-parameter vectors: the fixed theta in row 0, the others with
every kernel parameter moved by up to +-0.05 (seeded); the constant mean is the same in every row, so the loop of single
calls sends no residual again.  Each configuration runs in a child process of its own under a time limit of `--limit`
seconds (the first one that fails or runs out of time ends the run).  After one discarded call each, `reps` calls - every
repetition is written down, the median is marked - of
  batch F       marginal_likelihood_batch(thetas)                    one gpmi_sgp_bound_batch
  loop F        [marginal_likelihood(t) for t in thetas]             T gpmi_sgp_bound
  batch F+grad  marginal_likelihood_gradient_batch(thetas)
  loop F+grad   [marginal_likelihood_gradient(t) for t in thetas]
in rows per second, then the four GPMI_PROF_SGP_* stage times (HIP events, a run of their own) of ONE chunk of the gradient
batch, with the chunk size gpmi_sgp_batch_schedule reports, beside those of one single gradient call.
`--parent DIR`: a checkout of the parent commit with its library built; its single bound and bound + gradient (T = 1) are
measured by this script in a child process that imports the package from DIR, in the same session, and F is compared bit
for bit.  `--tiny` runs small shapes (a check of the tool itself).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
D = 8
STAGES = ("build", "gram", "factor", "grad")


def data(n):
    rng = np.random.default_rng(17)
    x = rng.uniform(0.0, 1.0, size=(n, D))
    y = np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(2.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    theta = np.array([float(y.mean()), 0.0] + [np.log(0.8)] * D + [np.log(0.1)])
    return x, y, theta


def rows_of(theta, T):
    rng = np.random.default_rng(23)
    rows = np.repeat(theta[None, :], T, axis=0)
    rows[1:, 1:] += rng.uniform(-0.05, 0.05, size=(T - 1, theta.size - 1))
    return rows


def times_ms(fn, reps):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def one(n, m, T, reps, tree):
    sys.path.insert(0, os.path.join(tree, "inference-tools_amd"))
    from inference_amd.gp import SparseGpRegressor, SquaredExponential, WhiteNoise

    x, y, theta = data(n)
    gp = SparseGpRegressor(x, y, inducing_points=m, kernel=SquaredExponential() + WhiteNoise(), hyperpars=theta, seed=17)
    eng = gp.engine
    rows = rows_of(theta, T)

    def stages(fn):
        eng.profile_stages(True)
        fn()
        eng.stage_ms()
        fn()
        out = {k: v["ms"] for k, v in eng.stage_ms().items()}
        eng.profile_stages(False)
        return out

    row = {"n": n, "m": m, "T": T, "F": gp.marginal_likelihood(theta),
           "loop_F_ms": times_ms(lambda: [gp.marginal_likelihood(t) for t in rows], reps),
           "loop_grad_ms": times_ms(lambda: [gp.marginal_likelihood_gradient(t) for t in rows], reps),
           "single_stage_ms": stages(lambda: gp.marginal_likelihood_gradient(theta))}
    if hasattr(gp, "marginal_likelihood_batch"):
        from inference_amd._engine import sgp_batch_schedule

        sched = sgp_batch_schedule(n, m, D, T, want_grad=True)
        row["chunk"], row["chunks"] = sched["chunk"], sched["chunks"]
        row["batch_F_ms"] = times_ms(lambda: gp.marginal_likelihood_batch(rows), reps)
        row["batch_grad_ms"] = times_ms(lambda: gp.marginal_likelihood_gradient_batch(rows), reps)
        row["chunk_stage_ms"] = stages(lambda: gp.marginal_likelihood_gradient_batch(rows[:sched["chunk"]]))
        Fb = gp.marginal_likelihood_batch(rows)
        row["batch_F0"] = float(Fb[0])
        row["max_rel_batch_vs_loop"] = float(np.max(np.abs(Fb - np.array([gp.marginal_likelihood(t) for t in rows])) / np.abs(Fb)))
    print(json.dumps(row), flush=True)


def fmt(v, T):
    """rows per second: median [every repetition]"""
    rate = [T / (t * 1e-3) for t in v]
    return f"{float(np.median(rate)):9.1f}  [" + " ".join(f"{r:.1f}" for r in rate) + "]"


def fmt_ms(v):
    return f"{float(np.median(v)):8.2f}  [" + " ".join(f"{t:.2f}" for t in v) + "]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, type=int, default=None)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.one[2], a.reps, os.path.abspath(a.tree))
    shapes = [(3000, 64), (5000, 200)] if a.tiny else [(100000, m) for m in (512, 1024, 2048)]
    batches = (1, 4) if a.tiny else (1, 8, 32, 64)
    lines = [f"# tools/sparse_batch_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: SquaredExponential + WhiteNoise, d = {D}; "
             "rows per second (ms for the single calls): median [every repetition], after one discarded call; stages in ms "
             "from HIP events in runs of their own"]

    def child(n, m, T, tree):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(n), str(m), str(T), "--reps", str(a.reps), "--tree", tree]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            return None, f"no result within {a.limit:.0f} s"
        if out.returncode != 0:
            return None, f"exit status {out.returncode}: {out.stderr.strip().splitlines()[-1:]}"
        return json.loads(out.stdout.strip().splitlines()[-1]), None

    def finish(ok):
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return 0 if ok else 1

    for n, m in shapes:
        lines.append(f"N = {n}, m = {m}")
        single = {}
        for label, tree in (("parent", a.parent), ("this  ", ROOT)):
            if tree is None:
                continue
            row, why = child(n, m, 1, os.path.abspath(tree))
            if row is None:
                lines.append(f"  {label} single: {why}; the run ends here")
                return finish(False)
            single[label] = row
            st = row["single_stage_ms"]
            lines.append(f"  {label} single  bound {fmt_ms(row['loop_F_ms'])} ms   bound+grad {fmt_ms(row['loop_grad_ms'])} ms   stages "
                         + " ".join(f"{k} {st[k]:.2f}" for k in STAGES) + f"   F = {row['F']!r}")
        if len(single) == 2:
            lines.append(f"  F of the single evaluation bit-identical to the parent's: {single['parent']['F'] == single['this  ']['F']}")
        for T in batches:
            row, why = child(n, m, T, ROOT)
            if row is None:
                lines.append(f"  T = {T}: {why}; the run ends here")
                return finish(False)
            st = row["chunk_stage_ms"]
            lines.append(f"  T = {T:3d} (chunks of {row['chunk']}: {row['chunks']})")
            lines.append(f"    F       batch {fmt(row['batch_F_ms'], T)} rows/s   loop {fmt(row['loop_F_ms'], T)} rows/s   "
                         f"ratio {np.median(row['loop_F_ms']) / np.median(row['batch_F_ms']):.2f}")
            lines.append(f"    F+grad  batch {fmt(row['batch_grad_ms'], T)} rows/s   loop {fmt(row['loop_grad_ms'], T)} rows/s   "
                         f"ratio {np.median(row['loop_grad_ms']) / np.median(row['batch_grad_ms']):.2f}")
            lines.append(f"    one chunk of {row['chunk']}, ms per row: " + " ".join(f"{k} {st[k] / row['chunk']:.2f}" for k in STAGES)
                         + f"   (rows against the loop: {row['max_rel_batch_vs_loop']:.1e} relative in F)")
    return finish(True)


if __name__ == "__main__":
    sys.exit(main())
