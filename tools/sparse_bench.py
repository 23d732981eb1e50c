"""
Timings of SparseGpRegressor (the variational inducing-point model on the device: csrc/sparse.hip around the cross build,
the fp64-MFMA GEMM and the small-problem factorisation).

    python tools/sparse_bench.py [--reps 3] [--tiny] [--limit 240] [--out profiles/r17_sparse.txt]

Model: SquaredExponential + WhiteNoise, d = 8, fixed hyper-parameters, inducing inputs a random subset of x.  For
N in {1e5, 1e6} and m in {512, 1024, 2048}, each configuration in a child process of its own under a time limit of
`--limit` seconds (the first one that fails or runs out of time ends the run).  After one discarded call each, the
medians of `reps` calls of
  bound       marginal_likelihood(theta)            pass 1 and the m x m algebra
  bound+grad  marginal_likelihood_gradient(theta)   ... and the gradient (pass 2), alpha back to the host
  fit         set_hyperparameters(theta)
  predict     1024 points
  build / gram / factor / grad
              the four device stages of one bound + gradient from HIP events (profile classes GPMI_PROF_SGP_*), in runs
              of their own; `gram TF/s` is the rate of the tall-skinny Gram product (lower tiles: N m (m + 128) FLOP)
At N = 1e5, m = 512 the NumPy mirror's bound (tests/sparse_host.py) is timed in the same process and compared; the exact
GpRegressor's fit at N = 16384 is timed for scale.  `--tiny` runs small shapes (a check of the tool itself).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 8


def median_ms(fn, reps):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def data(n):
    rng = np.random.default_rng(17)
    x = rng.uniform(0.0, 1.0, size=(n, D))
    y = np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(2.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    theta = np.array([float(y.mean()), 0.0] + [np.log(0.8)] * D + [np.log(0.1)])
    return x, y, theta


def one(n, m, reps, with_mirror):
    from inference_amd.gp import SparseGpRegressor, SquaredExponential, WhiteNoise

    x, y, theta = data(n)
    gp = SparseGpRegressor(x, y, inducing_points=m, kernel=SquaredExponential() + WhiteNoise(), hyperpars=theta, seed=17)
    pts = np.random.default_rng(18).uniform(0.0, 1.0, size=(1024, D))
    row = {"n": n, "m": m,
           "bound_ms": median_ms(lambda: gp.marginal_likelihood(theta), reps),
           "grad_ms": median_ms(lambda: gp.marginal_likelihood_gradient(theta), reps),
           "fit_ms": median_ms(lambda: gp.set_hyperparameters(theta), reps),
           "predict_ms": median_ms(lambda: gp(pts), reps)}
    eng = gp.engine
    eng.profile_stages(True)
    per = {k: [] for k in ("build", "gram", "factor", "grad")}
    rate = []
    for _ in range(reps):
        gp.marginal_likelihood_gradient(theta)
        st = eng.stage_ms()
        for k in per:
            per[k].append(st[k]["ms"])
        rate.append(st["gram"]["flops"] / max(st["gram"]["ms"], 1e-9) * 1e-9)
    eng.profile_stages(False)
    row["stages_ms"] = {k: float(np.median(v)) for k, v in per.items()}
    row["gram_tflops"] = float(np.median(rate))
    row["F"] = gp.marginal_likelihood(theta)
    if with_mirror:
        import sparse_host as sh

        mir = sh.SparseMirror("se", x, gp.inducing_points)
        t0 = time.perf_counter()
        F = mir.bound(theta[1:-1], float(np.exp(2.0 * theta[-1])), y - theta[0], None)
        row["mirror_bound_ms"] = (time.perf_counter() - t0) * 1e3
        row["mirror_F"] = F
    print(json.dumps(row), flush=True)


def exact_fit(reps):
    import workloads as wl
    from inference_amd.gp import GpRegressor, SquaredExponential

    x, y, e = wl.synthetic_dataset(17, 16384, D)
    theta = wl.timing_theta(wl.SE, y, D)
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    print(json.dumps({"exact_fit_ms": median_ms(lambda: gp.set_hyperparameters(theta), reps), "n": 16384}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=2, type=int, default=None)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--mirror", action="store_true")
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.reps, a.mirror)
    if a.exact:
        return exact_fit(a.reps)
    shapes = [(3000, 64), (5000, 200)] if a.tiny else [(n, m) for n in (100000, 1000000) for m in (512, 1024, 2048)]
    lines = [f"# tools/sparse_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: SquaredExponential + WhiteNoise, d = {D}; milliseconds, "
             "medians after one discarded call; stages from HIP events in runs of their own",
             f"# {'N':>8s} {'m':>5s} {'bound':>9s} {'bound+grad':>10s} {'fit':>9s} {'predict':>9s} | {'build':>9s} {'gram':>9s} {'factor':>9s} "
             f"{'grad':>9s} | {'gram TF/s':>9s}"]
    print("\n".join(lines), flush=True)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)]
    for i, (n, m) in enumerate(shapes):
        cmd = me + ["--one", str(n), str(m)] + (["--mirror"] if (n, m) in ((100000, 512), (3000, 64)) else [])
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"# N = {n}, m = {m}: no result within {a.limit:.0f} s; the run ends here")
            print(lines[-1], flush=True)
            break
        if res.returncode != 0:
            lines.append(f"# N = {n}, m = {m}: exit status {res.returncode}; the run ends here")
            print(lines[-1], res.stderr[-2000:], flush=True)
            break
        r = json.loads(res.stdout.strip().splitlines()[-1])
        s = r["stages_ms"]
        lines.append(f"{n:10d} {m:5d} {r['bound_ms']:9.2f} {r['grad_ms']:10.2f} {r['fit_ms']:9.2f} {r['predict_ms']:9.2f} | "
                     f"{s['build']:9.2f} {s['gram']:9.2f} {s['factor']:9.2f} {s['grad']:9.2f} | {r['gram_tflops']:9.1f}")
        if "mirror_F" in r:
            lines.append(f"#   NumPy mirror, same process: bound {r['mirror_bound_ms']:.0f} ms; F device {r['F']:.9g}, mirror {r['mirror_F']:.9g}")
        print("\n".join(lines[-2:] if "mirror_F" in r else lines[-1:]), flush=True)
    else:
        if not a.tiny:
            try:
                res = subprocess.run(me + ["--exact"], capture_output=True, text=True, timeout=a.limit)
                if res.returncode == 0:
                    r = json.loads(res.stdout.strip().splitlines()[-1])
                    lines.append(f"# for scale: the exact GpRegressor's fit (set_hyperparameters) at N = 16384, d = {D}: {r['exact_fit_ms']:.2f} ms")
                    print(lines[-1], flush=True)
            except subprocess.TimeoutExpired:
                pass
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
