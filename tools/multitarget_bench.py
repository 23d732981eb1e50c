"""
Timings of MultiTargetGpRegressor (T targets on one device factorisation: csrc/api_multi.hip) beside the single-target
GpRegressor calls at the same N and the loop over T single-target models a user had before it, in one process.

    python tools/multitarget_bench.py [--reps 3] [--tiny] [--parent DIR] [--out profiles/r23_multitarget.txt]

Model: SquaredExponential, d = 8, fixed hyper-parameters (workloads.timing_theta), y_err = 0.1; N = 4096 and 8192,
T = 16, 256 and 2048 targets, M = 1024 query points.  Per (N, T), end to end with every transfer, after one discarded call
the median of `reps` calls of
  fit       set_hyperparameters(theta)              K, L, V^T, A^T, lml_t back
  lml       marginal_likelihood(theta')             K, L, V^T on lane 1
  grad      marginal_likelihood_gradient(theta')    ... A^T, L^-T, K^-1, K^-1 - A A^T / T, one contraction
  predict   gp(points)                              M x T means and M variances back
and per call the device time by profile class (HIP events, in-kernel stamps for the trailing updates), taken in one run
of its own with the classes switched on - the events' synchronisation is not in the end-to-end figures, the split
covariance build is one launch there, and classes that run side by side on two streams (the factorisation's panels and
updates) add up to more than the wall time.  `single`: the same four calls of a GpRegressor at that N.  `loop`: T single-target
models one after another - construction (the data set goes up again), fit, lml, gradient, predict, close - run in full for
T <= 16 and extrapolated from those 16 beyond.
`--parent DIR`: a checkout of the parent commit with its library built; `python bench.py --gpus 1` is then run as a child
process in DIR and in this tree, after everything else, and both result lines go to the end of the output.
`--tiny` runs small shapes (a check of the tool itself).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import workloads as wl  # noqa: E402
from inference_amd import _lib  # noqa: E402
from inference_amd.gp import GpRegressor, MultiTargetGpRegressor, SquaredExponential  # noqa: E402

CLASSES = (("kbuild", _lib.PROF_KBUILD), ("panel", _lib.PROF_PANEL), ("flow", _lib.PROF_FLOW), ("syrk", _lib.PROF_SYRK),
           ("syrk_rest", _lib.PROF_SYRK_REST), ("syrk_slice", _lib.PROF_SYRK_SLICE), ("solve", _lib.PROF_SOLVE),
           ("trsm", _lib.PROF_TRSM))
CALLS = ("fit", "lml", "grad", "predict")


def make_targets(x, y, T, seed=5):
    """Column t: y (1 + 0.3 t) + 0.2 sin((t + 1) x_0) + 0.05 N(0, 1) (the recipe of tests/multitarget_host.py)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    return (y[:, None] * (1.0 + 0.3 * t)[None, :] + 0.2 * np.sin((t + 1)[None, :] * x[:, :1])
            + 0.05 * rng.standard_normal((x.shape[0], T)))


def median_ms(fn, reps):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def by_class(eng, fn):
    mask = 0
    for _, k in CLASSES:
        mask |= 2 << k
    eng.profile_enable(mask)
    eng.profile_reset()
    fn()
    out = {name: eng.profile_read(k)["ms"] for name, k in CLASSES}
    eng.profile_reset()
    eng.profile_enable(0)
    return out


def calls_of(gp, theta, other, pts):
    return {"fit": lambda: gp.set_hyperparameters(theta), "lml": lambda: gp.marginal_likelihood(other),
            "grad": lambda: gp.marginal_likelihood_gradient(other), "predict": lambda: gp(pts)}


def fmt_classes(c):
    syrk = c["syrk"] + c["syrk_rest"] + c["syrk_slice"]
    return (f"kbuild {c['kbuild']:.2f} potrf {c['panel'] + c['flow'] + syrk:.2f} (updates {syrk:.2f}) "
            f"sweeps {c['solve']:.2f} row solves+products {c['trsm']:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = 8
    sizes, counts, M, full = ((300, 640), (3, 130), 257, 3) if a.tiny else ((4096, 8192), (16, 256, 2048), 1024, 16)
    lines = [f"# tools/multitarget_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}, one MI355X: SquaredExponential, d = {d}, "
             f"M = {M}; milliseconds end to end with transfers, median of {a.reps} after one discarded call; the classes: device "
             "milliseconds of ONE call from HIP events / in-kernel stamps, in a run of their own"]
    print(lines[0], flush=True)
    rows = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for n in sizes:
        x, y, e = wl.synthetic_dataset(23, n, d)
        pts = wl.query_points(23, M, d)
        theta = np.array(wl.timing_theta(wl.SE, y, d)[1:])
        other = theta + 0.05
        say(f"N = {n}")
        one = GpRegressor(x, y, y_err=e, hyperpars=np.concatenate([[y.mean()], theta]), kernel=SquaredExponential)
        th1, ot1 = np.concatenate([[y.mean()], theta]), np.concatenate([[y.mean()], other])
        single = {k: median_ms(f, a.reps) for k, f in calls_of(one, th1, ot1, pts).items()}
        single_cls = {k: by_class(one.engine, f) for k, f in calls_of(one, th1, ot1, pts).items()}
        say("  single-target GpRegressor:  " + "  ".join(f"{k} {single[k]:8.2f}" for k in CALLS))
        for k in CALLS:
            say(f"      {k:8s} {fmt_classes(single_cls[k])}")
        one.engine.close()
        Yfull = make_targets(x, y, max(counts))
        # the loop over single-target models, `full` of them in full
        t_loop = {k: 0.0 for k in ("build+fit",) + CALLS[1:]}
        for t in range(min(full, max(counts))):
            tht = np.concatenate([[Yfull[:, t].mean()], theta])
            t0 = time.perf_counter()
            g = GpRegressor(x, Yfull[:, t], y_err=e, hyperpars=tht, kernel=SquaredExponential)
            t1 = time.perf_counter()
            g.marginal_likelihood(tht + 0.05)
            t2 = time.perf_counter()
            g.marginal_likelihood_gradient(tht + 0.05)
            t3 = time.perf_counter()
            g(pts)
            t4 = time.perf_counter()
            g.engine.close()
            for k, dt in zip(t_loop, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                t_loop[k] += dt * 1e3
        n_loop = min(full, max(counts))
        for T in counts:
            Y = np.ascontiguousarray(Yfull[:, :T])
            t0 = time.perf_counter()
            gp = MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
            build = (time.perf_counter() - t0) * 1e3
            calls = calls_of(gp, theta, other, pts)
            ms = {k: median_ms(f, a.reps) for k, f in calls.items()}
            cls = {k: by_class(gp.engine, f) for k, f in calls.items()}
            scale = T / n_loop
            tag = "measured" if T <= n_loop else f"extrapolated from {n_loop} models"
            say(f"  T = {T:5d}: construction + first fit {build:9.2f}   " + "  ".join(f"{k} {ms[k]:8.2f}" for k in CALLS))
            say(f"      over the single-target call:        " + "  ".join(f"{k} {ms[k] / single[k]:7.2f}x" for k in CALLS))
            say(f"      loop over T models ({tag}): build+fit {t_loop['build+fit'] * scale:10.1f}  "
                + "  ".join(f"{k} {t_loop[k] * scale:10.1f}" for k in CALLS[1:]))
            tp = -(-T // 128) * 128
            say(f"      row solves, as triangular solves: 2 N^2 T_pad = {2.0 * n * n * tp / 1e9:.1f} GFLOP forward + backward (fit, grad), "
                f"half for lml; the gradient's product on the lower tiles: N^2 T_pad = {1.0 * n * n * tp / 1e9:.1f} GFLOP; the means: "
                f"2 M N T_pad = {2.0 * M * n * tp / 1e9:.1f} GFLOP and {8e-6 * M * T:.1f} MB back")
            for k in CALLS:
                say(f"      {k:8s} {fmt_classes(cls[k])}")
            rows.append({"n": n, "T": T, "ms": ms, "classes_ms": cls, "construction_ms": build, "single_ms": single,
                         "loop_ms": {k: v * scale for k, v in t_loop.items()}, "loop_models_run": n_loop})
            gp.engine.close()
    if a.parent:
        # behind everything else, each in a child process of its own: the headline belongs to code this model does not touch
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "60", "--warmup", "5"]
        for label, tree in (("parent", a.parent), ("this tree", ROOT), ("parent", a.parent), ("this tree", ROOT)):
            res = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
            last = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
            if res.returncode != 0 or not last:
                say(f"# bench.py ({label}) failed with status {res.returncode}: {res.stderr[-300:]}")
                break
            r = json.loads(last[-1])
            keep = {k: r[k] for k in r if isinstance(r[k], (int, float, str)) and len(str(r[k])) < 40}
            say(f"# bench.py --gpus 1 --steps 60 --warmup 5 ({label}): {json.dumps(keep)}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"tool": "multitarget_bench", "tiny": a.tiny, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
