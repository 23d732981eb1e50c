"""
Timings of the greedy inducing-point selection (gpmi_select_points: csrc/select.hip) and what it gains over a random
subset.

    python tools/select_bench.py [--reps 3] [--limit 300] [--out profiles/r20_select.txt]

Model: SquaredExponential + WhiteNoise, d = 8, fixed hyper-parameters (those of tools/sparse_post_bench.py); N = 1e5 with
m in {512, 1024, 2048}, and N = 1e6 with m = 512; each configuration in a child process of its own under a time limit of
`--limit` seconds; the first child that fails or runs out of time ends the run: nothing more is started on the device
behind it.  After one discarded call each, `reps` calls are timed; every repetition is written down, the median first.
  select, end to end      select_inducing_points(x, m, ...): a handle of its own, upload, allocation, launches, read-back
  select, gpmi_timer      gpmi_timer_start / gpmi_select_points / gpmi_timer_stop on one handle: the whole call without
                          the handle; GB/s = 8 N m^2 / 2 bytes (the rows of V a selection reads) over that time, next
                          to the streamed-HBM figure of 6.0e3 GB/s - the call's upload and allocation are inside it, so
                          the fraction is a lower bound of the sweep's
  bound + gradient        marginal_likelihood_gradient at the greedy Z, same process
  F                       the bound at the greedy Z and at five random subsets (seeds 0 .. 4), same theta
`--tiny` runs small shapes (a check of the tool itself).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HBM_GBS = 6.0e3  # streamed HBM reads, GB/s
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def times_ms(fn, reps):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t))] + [float(v) for v in t]


def data(n, d):
    rng = np.random.default_rng(17)
    x = rng.uniform(0.0, 1.0, size=(n, d))
    y = np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(2.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    theta = np.array([float(y.mean()), 0.0] + [np.log(0.8 * np.sqrt(d / 8.0))] * d + [np.log(0.1)])
    return x, y, theta


def timer_ms(x, theta_stat, m, reps):
    """gpmi_timer around gpmi_select_points on one handle (the timer needs a data set: two dummy points)."""
    from inference_amd import _lib

    h = _lib.Handle()
    two = np.zeros((2, x.shape[1]))
    two[1] = 1.0
    h.call("gpmi_set_data", _lib.dptr(two), _lib.dptr(np.zeros(2)), _lib.dptr(np.ones(2)), None, 2, x.shape[1])
    index, trace, pv, count = np.zeros(m, dtype=np.int64), np.zeros(m + 1), np.zeros(m), C.c_int64(0)
    out = []
    for _ in range(reps + 1):
        ms = C.c_float(0.0)
        h.call("gpmi_timer_start")
        h.call("gpmi_select_points", x.shape[0], x.shape[1], _lib.dptr(x), None, _lib.KERNEL_SE, _lib.dptr(theta_stat),
               theta_stat.size, m, 1e-8, 0.0, index.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(trace), _lib.dptr(pv),
               C.byref(count))
        h.call("gpmi_timer_stop", C.byref(ms))
        out.append(float(ms.value))
    h.close()
    return [float(np.median(out[1:]))] + out[1:], int(count.value)


def one(n, d, m, reps):
    from inference_amd.gp import SparseGpRegressor, SquaredExponential, WhiteNoise, select_inducing_points

    x, y, theta = data(n, d)
    kernel = SquaredExponential() + WhiteNoise()
    row = {"n": n, "d": d, "m": m}
    row["select_ms"] = times_ms(lambda: select_inducing_points(x, m, kernel, theta[1:]), reps)
    row["timer_ms"], row["count"] = timer_ms(x, np.ascontiguousarray(theta[1:-1]), m, reps)
    row["gbs"] = 8.0 * n * m * m / 2.0 / (row["timer_ms"][0] * 1e-3) / 1e9
    gp = SparseGpRegressor(x, y, inducing_points=m, kernel=kernel, hyperpars=theta, inducing_method="greedy")
    row["F_greedy"] = gp.bound
    row["grad_ms"] = times_ms(lambda: gp.marginal_likelihood_gradient(theta), reps)
    row["F_random"] = []
    for seed in range(5):
        rows = np.sort(np.random.default_rng(seed).choice(n, gp.inducing_points.shape[0], replace=False))
        try:
            gp.set_inducing_points(x[rows].copy())
            row["F_random"].append(gp.bound)
        except np.linalg.LinAlgError:  # (K_mm of this subset did not factorise)
            row["F_random"].append(float("nan"))
    print(json.dumps(row), flush=True)


def fmt(v):
    return f"{v[0]:9.2f} (" + " ".join(f"{t:.2f}" for t in v[1:]) + ")"


def child(args, limit):
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"no result within {limit:.0f} s"
    if res.returncode != 0:
        return None, f"exit status {res.returncode}: {res.stderr[-1500:]}"
    return json.loads(res.stdout.strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, type=int, default=None)  # n d m
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.one[2], a.reps)
    shapes = [(4000, 64), (4000, 200)] if a.tiny else [(100000, 512), (100000, 1024), (100000, 2048), (1000000, 512)]
    lines = [f"# tools/select_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: SquaredExponential + WhiteNoise, d = 8; milliseconds: "
             "median (every repetition) after one discarded call; GB/s = 8 N m^2 / 2 bytes over the gpmi_timer time, "
             f"streamed HBM {HBM_GBS:.0f} GB/s"]
    print(lines[0], flush=True)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for n, m in shapes:
        r, err = child(["--reps", str(a.reps), "--one", str(n), "8", str(m)], a.limit)
        if err:
            say(f"# N = {n}, m = {m}: {err}; not measured, the run ends here")
            break
        say(f"N = {n}, m = {m} (selected {r['count']})")
        say(f"  select, end to end {fmt(r['select_ms'])}   by gpmi_timer {fmt(r['timer_ms'])}   {r['gbs']:.0f} GB/s = "
            f"{100.0 * r['gbs'] / HBM_GBS:.0f} % of streamed HBM")
        say(f"  bound + gradient at the greedy Z {fmt(r['grad_ms'])}")
        say(f"  F: greedy {r['F_greedy']:.9g}   random subsets " + " ".join(f"{F:.9g}" for F in r["F_random"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
