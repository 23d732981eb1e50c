"""
Times the exact Hessian of the log-marginal likelihood beside what a user had to do without it.

    python tools/hessian_bench.py [--sizes 2048,4096,8192] [--d 8] [--reps 3] [--out profiles/r07_hessian.txt]

SquaredExponential, d = 8, ConstantMean, `workloads.synthetic_dataset`, all sizes in one process.  Per size, after one
discarded call of each, the median of `--reps` calls (every repetition is listed):

  exact      GpRegressor.marginal_likelihood_hessian(theta, method="exact")   one factorisation (gpmi_lml_hessian)
  2P grads   2 P calls of marginal_likelihood_gradient at shifted theta - central differences of the gradient, each call a
             factorisation of its own (P = d + 2 with the mean)
  stages     HIP events of the four stages of gpmi_lml_hessian (GPMI_PROF_HESS_BUILD / _GEMM / _TRACE / _CONTRACT), in a run of
             their own (the events perturb the overlap), with the GEMM's rate from its 2 N_pad^3 FLOP per parameter

No gate: the numbers go to the README and DESIGN.md.
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
from inference_amd.gp import GpRegressor, SquaredExponential  # noqa: E402

STAGES = (("build", _lib.PROF_HESS_BUILD), ("gemm", _lib.PROF_HESS_GEMM), ("trace", _lib.PROF_HESS_TRACE),
          ("contract", _lib.PROF_HESS_CONTRACT))


def times_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stage_events(gp, fn, reps):
    eng = gp.engine
    mask = 0
    for _, k in STAGES:
        mask |= 2 << k
    eng.profile_enable(mask)
    eng.profile_reset()
    rows = []
    for _ in range(reps):
        fn()
        rows.append({name: eng.profile_read(k) for name, k in STAGES})
        eng.profile_reset()
    eng.profile_enable(0)
    return rows


def one(n, d, reps):
    x, y, e = wl.synthetic_dataset(1, n, d)
    theta = wl.timing_theta(wl.SE, y, d)
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    P = theta.size

    def exact():
        return gp.marginal_likelihood_hessian(theta, method="exact")

    def grads():
        for i in range(P):
            for sgn in (1.0, -1.0):
                t = theta.copy()
                t[i] += sgn * 1e-4
                gp.marginal_likelihood_gradient(t)

    t_exact = times_ms(exact, reps)
    t_grads = times_ms(grads, reps)
    H = exact()[2]
    H_fd = gp.marginal_likelihood_hessian(theta, method="fd")[2]
    ev = stage_events(gp, exact, reps)
    gp.engine.close()
    return dict(n=n, P=P, exact=t_exact, grads=t_grads, ev=ev,
                fd_diff=float(np.abs(H - H_fd).max() / np.abs(H).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_hessian.txt"))
    args = ap.parse_args()
    lines = [f"hessian_bench: SquaredExponential, d = {args.d}, ConstantMean; milliseconds, median of {args.reps} after one "
             "discarded call (every repetition in brackets); stages: HIP events in runs of their own"]

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for n in [int(v) for v in args.sizes.split(",")]:
        r = one(n, args.d, args.reps)
        fmt = lambda v: "[" + ", ".join(f"{t:.2f}" for t in v) + "]"  # noqa: E731
        say(f"N = {r['n']}, P = {r['P']}: exact {np.median(r['exact']):.2f} {fmt(r['exact'])}   2P gradients "
            f"{np.median(r['grads']):.2f} {fmt(r['grads'])}   ratio {np.median(r['grads']) / np.median(r['exact']):.2f}   "
            f"max |H - H_fd| / max |H| = {r['fd_diff']:.1e}")
        for name, _ in STAGES:
            ms = [row[name]["ms"] for row in r["ev"]]
            fl = r["ev"][0][name]["flops"]
            rate = f"   {fl / (np.median(ms) * 1e-3) / 1e12:.1f} TFLOP/s" if name == "gemm" and np.median(ms) > 0 else ""
            say(f"    {name:9s} {np.median(ms):8.2f} {fmt(ms)}  ({r['ev'][0][name]['launches']} brackets){rate}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
