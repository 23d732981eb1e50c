"""
Timings of GeneralisedGpRegressor (Laplace's method on the device: csrc/api_generalised.hip, csrc/generalised.hip) beside
the Gaussian GpRegressor at the same N, in one process.

    python tools/generalised_bench.py [--reps 3] [--tiny] [--out profiles/r24_generalised.txt]

Model: Poisson likelihood (exposure 1), SquaredExponential, d = 8, x of workloads.synthetic_dataset, counts drawn from
exp(1 + y) of its smooth y; theta = [0, ln 0.5 x 8]; N = 2048, 4096 and 8192.  Per N, end to end with every transfer,
after one discarded call the median of `reps` calls of
  fit        set_hyperparameters(theta)              Newton's iteration on lane 0, the factor of B at the mode kept
  logq       marginal_likelihood(theta')             the same on lane 1
  logq+grad  marginal_likelihood_gradient(theta')    ... and the gradient's tail
with the Newton step count, and beside them GpRegressor's fit and gradient at that N (y_err = 0.1): a Newton step
factorises a matrix as the Gaussian fit does, so the honest yardstick of `fit` is steps x the Gaussian fit.
Per call the device time by profile class (HIP events; in-kernel stamps for the trailing updates), in a run of its own
with the classes switched on: the events' synchronisation is not in the end-to-end figures, and classes that run side by
side on two streams (the factorisation's panels and updates) add up to more than the wall time.
The K V kernel on its own (gpmi_ggp_kv, 20 products between two HIP events): achieved bytes per second, 8 n_pad^2 bytes a
product, against the streamed-HBM rate of profiles/r20_select.txt (6000 GB/s).
`--tiny` runs small shapes (a check of the tool itself).
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
from inference_amd.gp import GeneralisedGpRegressor, GpRegressor, Poisson, SquaredExponential  # noqa: E402

STREAMED_HBM_GBS = 6000.0
CLASSES = (("kbuild", _lib.PROF_KBUILD), ("panel", _lib.PROF_PANEL), ("flow", _lib.PROF_FLOW), ("syrk", _lib.PROF_SYRK),
           ("syrk_rest", _lib.PROF_SYRK_REST), ("syrk_slice", _lib.PROF_SYRK_SLICE), ("solve", _lib.PROF_SOLVE),
           ("trsm", _lib.PROF_TRSM), ("terms", _lib.PROF_GGP_TERMS), ("kv", _lib.PROF_GGP_KV), ("bform", _lib.PROF_GGP_BFORM),
           ("grad_tail", _lib.PROF_GGP_GRAD))


def median_ms(fn, reps):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, [x * 1e3 for x in t]


def by_class(eng, fn):
    mask = 0
    for _, k in CLASSES:
        mask |= 2 << k
    eng.profile_enable(mask)
    eng.profile_reset()
    fn()
    out = {name: eng.profile_read(k) for name, k in CLASSES}
    eng.profile_reset()
    eng.profile_enable(0)
    return out


def fmt(med, all_):
    return f"{med:9.2f} ({' '.join(f'{x:.2f}' for x in all_)})"


def run(n, d, reps, say):
    x, y, _ = wl.synthetic_dataset(2, n, d)
    counts = np.random.default_rng(n).poisson(np.exp(1.0 + y)).astype(float)
    theta = np.array([0.0] + [np.log(0.5)] * d)
    other = theta + 0.05
    gp = GeneralisedGpRegressor(x, counts, likelihood=Poisson(), kernel=SquaredExponential(), hyperpars=theta)
    eng = gp.engine
    steps = gp.newton_log["iterations"]
    steps_other = eng.ggp_logq(gp._kernel_id, other, gp.tol, gp.max_iter)[1][0]
    calls = {"fit": lambda: gp.set_hyperparameters(theta), "logq": lambda: gp.marginal_likelihood(other),
             "logq+grad": lambda: gp.marginal_likelihood_gradient(other)}
    say(f"N = {n}, d = {d}: Newton steps {steps} (fit), {steps_other} (theta'), halvings {gp.newton_log['halvings']}; "
        f"log q = {gp._logq:.6f}")
    times = {}
    for name, fn in calls.items():
        times[name] = median_ms(fn, reps)
        say(f"  {name:10s} {fmt(*times[name])} ms")
    for name, fn in calls.items():
        prof = by_class(eng, fn)
        say(f"  {name:10s} device ms by class: " + "  ".join(f"{k} {v['ms']:.2f}/{v['launches']}" for k, v in prof.items()
                                                              if v["launches"]))
    # the K V kernel alone
    n_pad = -(-n // 128) * 128
    V = np.random.default_rng(1).normal(size=(4, n))
    for nv in (1, 4):
        eng.ggp_kv(gp._kernel_id, theta, V[:nv], reps=2)
        ms = float(np.median([eng.ggp_kv(gp._kernel_id, theta, V[:nv], reps=20, timed=True)[1] for _ in range(reps)])) / 20.0
        gbs = 8.0 * n_pad * n_pad / (ms * 1e-3) / 1e9
        say(f"  K V, {nv} vector(s): {ms * 1e3:8.1f} us per product, {gbs:7.0f} GB/s = {100.0 * gbs / STREAMED_HBM_GBS:.0f} % of "
            f"streamed HBM ({8.0 * n_pad * n_pad / 1e9:.3f} GB per pass)")
    gp.engine.close()
    # the Gaussian model at the same N
    gth = wl.timing_theta(wl.SE, y, d)
    gg = GpRegressor(x, y, y_err=np.full(n, 0.1), hyperpars=gth, kernel=SquaredExponential)
    gfit = median_ms(lambda: gg.set_hyperparameters(gth), reps)
    ggrad = median_ms(lambda: gg.marginal_likelihood_gradient(gth + 0.05), reps)
    say(f"  GpRegressor fit {fmt(*gfit)} ms, gradient {fmt(*ggrad)} ms")
    say(f"  fit / (steps x Gaussian fit) = {times['fit'][0] / (steps * gfit[0]):.2f};  "
        f"logq+grad / (steps x Gaussian fit + Gaussian gradient) = "
        f"{times['logq+grad'][0] / (steps_other * gfit[0] + ggrad[0]):.2f}")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/generalised_bench.py --reps {args.reps}{' --tiny' if args.tiny else ''}: Poisson, SquaredExponential, d = 8; "
        "milliseconds: median (every repetition) after one discarded call; class ms/launches from a run of its own")
    for n in ((300, 640) if args.tiny else (2048, 4096, 8192)):
        run(n, 8, args.reps, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
