"""
Timings of the fitted SparseGpRegressor's joint posterior, joint draws and derivatives by the query point
(gpmi_sgp_posterior, gpmi_sgp_posterior_draws, gpmi_sgp_spatial_derivatives: csrc/sparse.hip, sgp_qgrad_kernel).

    python tools/sparse_post_bench.py [--reps 3] [--limit 240] [--parent-tree DIR] [--out profiles/r19_sparse_post.txt]

Model: SquaredExponential + WhiteNoise, N = 1e5, d = 8, fixed hyper-parameters, inducing inputs a random subset of x, m in
{512, 1024, 2048}; each configuration in a child process of its own under a time limit of `--limit` seconds; the first
child that fails or runs out of time ends the run: nothing more is started on the device behind it.  After one discarded
call each, `reps` calls of every quantity are timed; every repetition is written down, the median first.
  fit, predict 1024             set_hyperparameters(theta), gp(points)
  d 1024 / d 4096               spatial_derivatives_batch at M points, with the variance part and (engine, want_var=False)
                                without
  post 1024 / post 4096         build_posterior at M points
  draws                         sample_posterior at (M, S) = (4096, 1024)
  products / fused              HIP events (GPMI_PROF_SGP_GRAM / _GRAD), in runs of their own, of one derivative call at
                                M = 4096: the cross build with its four products, and the fused kernel with its run sum;
                                `pairs/s` is m M / t of the fused kernel
  Sigma / factor / product      HIP events (GPMI_PROF_DRAWS_*) of the draws at (4096, 1024)
`--parent-tree DIR`: a built checkout of the parent commit; fit and predict 1024 are then measured on it by this script in
the same run, child by child next to this tree's, and the bits of F and of the predictions are compared.
At m = 512 the NumPy mirror (tests/sparse_post_host.py) is timed in the same process at M = 1024, for scale.  One more
child runs d = 64 (N = 20000, m = 1024: the large-LDS path of the fused kernel, one workgroup per CU).
`--tiny` runs small shapes (a check of the tool itself).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def use_tree(tree):
    for p in (os.path.join(ROOT, "tests"), tree, os.path.join(tree, "inference-tools_amd")):
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


def class_ms(eng, klass):
    """HIP-event milliseconds booked under one GPMI_PROF_* class since the last reset."""
    n = C.c_int64(0)
    ms, fl, by = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    eng.h.call("gpmi_profile_read", klass, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
    return ms.value


def events(eng, classes, fn, reps):
    """Medians (and every repetition) of the HIP-event time of each class over `reps` calls of fn."""
    mask = 0
    for k in classes:
        mask |= 2 << k
    eng.h.call("gpmi_profile_enable", mask)
    eng.h.call("gpmi_profile_reset")
    per = {k: [] for k in classes}
    for _ in range(reps):
        fn()
        for k in classes:
            per[k].append(class_ms(eng, k))
        eng.h.call("gpmi_profile_reset")
    eng.h.call("gpmi_profile_enable", 0)
    return {k: [float(np.median(v))] + [float(t) for t in v] for k, v in per.items()}


def one(n, d, m, reps, base_only, with_mirror, sizes):
    from inference_amd import _lib
    from inference_amd.gp import SparseGpRegressor, SquaredExponential, WhiteNoise

    x, y, theta = data(n, d)
    gp = SparseGpRegressor(x, y, inducing_points=m, kernel=SquaredExponential() + WhiteNoise(), hyperpars=theta, seed=17)
    rng = np.random.default_rng(18)
    pts = {M: rng.uniform(0.0, 1.0, size=(M, d)) for M in sorted(set(sizes) | {1024})}
    row = {"n": n, "d": d, "m": m, "fit_ms": times_ms(lambda: gp.set_hyperparameters(theta), reps),
           "predict_ms": times_ms(lambda: gp(pts[1024]), reps)}
    mean, std = gp(pts[1024])
    row["F"] = gp.bound
    row["digest"] = hashlib.sha256(np.float64(gp.bound).tobytes() + mean.tobytes() + std.tobytes()).hexdigest()[:16]
    if not base_only:
        eng = gp.engine
        big, S = max(sizes), sizes[0]
        for M in sizes:
            row[f"d{M}_ms"] = times_ms(lambda: gp.spatial_derivatives_batch(pts[M]), reps)
            row[f"d{M}_mean_only_ms"] = times_ms(lambda: eng.spatial_derivatives(pts[M], want_var=False), reps)
            row[f"post{M}_ms"] = times_ms(lambda: gp.build_posterior(pts[M]), reps)
        row["draws_ms"] = times_ms(lambda: gp.sample_posterior(pts[big], S, seed=1), reps)
        ev = events(eng, (_lib.PROF_SGP_GRAM, _lib.PROF_SGP_GRAD), lambda: eng.spatial_derivatives(pts[big]), reps)
        row["products_ev_ms"], row["fused_ev_ms"] = ev[_lib.PROF_SGP_GRAM], ev[_lib.PROF_SGP_GRAD]
        row["pairs_per_s"] = m * big / (row["fused_ev_ms"][0] * 1e-3)
        classes = (_lib.PROF_DRAWS_SIGMA, _lib.PROF_DRAWS_FACTOR, _lib.PROF_DRAWS_NORMALS, _lib.PROF_DRAWS_PRODUCT)
        ev = events(eng, classes, lambda: eng.posterior_draws(pts[big], n_draws=S, seed=1), reps)
        row["sigma_ev_ms"], row["factor_ev_ms"] = ev[_lib.PROF_DRAWS_SIGMA], ev[_lib.PROF_DRAWS_FACTOR]
        row["normals_ev_ms"], row["product_ev_ms"] = ev[_lib.PROF_DRAWS_NORMALS], ev[_lib.PROF_DRAWS_PRODUCT]
        if with_mirror:
            import sparse_host as sh
            import sparse_post_host as sph

            mir = sh.SparseMirror("se", x, gp.inducing_points)
            st = mir.state(theta[1:-1], float(np.exp(2.0 * theta[-1])), y - theta[0], None)
            t0 = time.perf_counter()
            dm, dv = sph.derivatives(mir, st, theta[1:-1], pts[1024])
            t1 = time.perf_counter()
            mu, sig = sph.posterior(mir, st, theta[1:-1], pts[1024])
            t2 = time.perf_counter()
            gm, gv = gp.spatial_derivatives_batch(pts[1024])
            row["mirror"] = {"derivatives_ms": (t1 - t0) * 1e3, "posterior_ms": (t2 - t1) * 1e3,
                             "dmean_diff": float(np.abs(gm - dm).max()), "dvar_diff": float(np.abs(gv - dv).max()),
                             "sigma_diff": float(np.abs(gp.build_posterior(pts[1024])[1] - sig).max())}
    print(json.dumps(row), flush=True)


def fmt(v):
    return f"{v[0]:9.2f} (" + " ".join(f"{t:.2f}" for t in v[1:]) + ")"


def child(args, limit, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args + (["--tree", tree] if tree else [])
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"no result within {limit:.0f} s"
    if res.returncode != 0:
        return None, f"exit status {res.returncode}: {res.stderr[-1500:]}"
    return json.loads(res.stdout.strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--one", nargs=3, type=int, default=None)  # n d m
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 4096])
    a = ap.parse_args()
    use_tree(a.tree or ROOT)
    if a.one:
        return one(a.one[0], a.one[1], a.one[2], a.reps, a.base_only, a.mirror, a.sizes)
    n = 4000 if a.tiny else 100000
    ms = [64, 200] if a.tiny else [512, 1024, 2048]
    sizes = ["--sizes"] + (["128", "300"] if a.tiny else ["1024", "4096"])
    big, S = (300, 128) if a.tiny else (4096, 1024)
    small = 128 if a.tiny else 1024
    lines = [f"# tools/sparse_post_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}"
             f"{' --parent-tree <a built checkout of the parent commit>' if a.parent_tree else ''}: SquaredExponential + WhiteNoise, N = {n}, d = 8; "
             "milliseconds: median (every repetition) after one discarded call; `ev`: HIP events, in runs of their own"]
    print(lines[0], flush=True)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for m in ms:
        r, err = child(["--reps", str(a.reps), "--one", str(n), "8", str(m)] + sizes + (["--mirror"] if m == ms[0] else []), a.limit)
        if err:
            say(f"# m = {m}: {err}; the run ends here")
            break
        say(f"m = {m}")
        say(f"  fit {fmt(r['fit_ms'])}   predict 1024 {fmt(r['predict_ms'])}   F = {r['F']:.9g}")
        for M in (small, big):
            say(f"  M = {M}: derivatives {fmt(r[f'd{M}_ms'])}   mean only {fmt(r[f'd{M}_mean_only_ms'])}   build_posterior {fmt(r[f'post{M}_ms'])}")
        say(f"  sample_posterior (M, S) = ({big}, {S}) {fmt(r['draws_ms'])}")
        say(f"  ev, derivatives at M = {big}: products {fmt(r['products_ev_ms'])}   fused kernel {fmt(r['fused_ev_ms'])}   "
            f"{r['pairs_per_s']:.3g} pairs/s")
        say(f"  ev, draws at ({big}, {S}): Sigma {fmt(r['sigma_ev_ms'])}   factor {fmt(r['factor_ev_ms'])}   normals {fmt(r['normals_ev_ms'])}   "
            f"product {fmt(r['product_ev_ms'])}")
        if "mirror" in r:
            mr = r["mirror"]
            say(f"  NumPy mirror, same process, M = {small}: derivatives {mr['derivatives_ms']:.0f} ms, posterior {mr['posterior_ms']:.0f} ms; "
                f"device - mirror: d mean {mr['dmean_diff']:.2e}, d var {mr['dvar_diff']:.2e}, Sigma {mr['sigma_diff']:.2e}")
        if a.parent_tree:
            # the parent's child first, this tree's only behind its success: a child that fails ends the run
            base = ["--reps", str(a.reps), "--base-only", "--one", str(n), "8", str(m)]
            p, err = child(base, a.limit, tree=os.path.abspath(a.parent_tree))
            t, err = child(base, a.limit) if not err else (None, err)
            if err:
                say(f"#   parent commit: {err}; the run ends here")
                break
            say(f"  parent commit, same script, same run:  fit {fmt(p['fit_ms'])}   predict 1024 {fmt(p['predict_ms'])}")
            say(f"  this tree, measured next to it:        fit {fmt(t['fit_ms'])}   predict 1024 {fmt(t['predict_ms'])}")
            say(f"  F and the 1024 predictions bit-identical to the parent's: {p['digest'] == t['digest']}")
        else:
            say("  parent commit: not measured")
    else:
        if not a.tiny:  # (only behind a run in which every child succeeded)
            r, err = child(["--reps", str(a.reps), "--one", "20000", "64", "1024"] + sizes, a.limit)
            if err:
                say(f"# d = 64: {err}")
            else:
                say("d = 64, N = 20000, m = 1024 (144 KiB of LDS per workgroup, one workgroup per CU)")
                say(f"  M = 4096: derivatives {fmt(r['d4096_ms'])}   mean only {fmt(r['d4096_mean_only_ms'])}")
                say(f"  ev: products {fmt(r['products_ev_ms'])}   fused kernel {fmt(r['fused_ev_ms'])}   {r['pairs_per_s']:.3g} pairs/s")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
