"""
Timings of GpRegressor.sample_posterior (joint posterior draws on the device: csrc/draws.hip around the solve, Gram update,
Cholesky and fp64-MFMA GEMM kernels) beside the host route a user had before it, in the same process.

    python tools/draws_bench.py [--reps 3] [--tiny] [--only K] [--out profiles/r16_draws.txt] [--json out.json]

Model: N = 4096 training points, d = 4, SquaredExponential, fixed hyper-parameters.  Shapes (M points, S draws):
(1024, 1024), (4096, 1024), (4096, 8192).  Per shape, after one discarded run of each route, the median of `reps` runs of
  device    sample_posterior(points, S, seed=...) end to end: points up, Sigma, the factorisation, the normals, the product
            and the S x M draws back to pageable memory
  Sigma / factor / normals / product
            of that, the four stages on the device from HIP events around them (profile classes GPMI_PROF_DRAWS_*), taken
            in runs of their own after the end-to-end runs: the events' synchronisation is not in `device`
  host      build_posterior (the device computes Sigma, the M x M matrix comes back), numpy.linalg.cholesky of
            Sigma + eps I, Generator.standard_normal((S, M)) and the matrix product, with each of the four pieces timed
`--only K` runs shape K alone; `--tiny` runs small shapes on a small model (a check of the tool itself).
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
from inference_amd import _lib  # noqa: E402
from inference_amd.gp import GpRegressor, SquaredExponential  # noqa: E402

SHAPES = [(1024, 1024), (4096, 1024), (4096, 8192)]
TINY = [(130, 64), (257, 300)]
JITTER = 1e-9
STAGES = (("Sigma", _lib.PROF_DRAWS_SIGMA), ("factor", _lib.PROF_DRAWS_FACTOR), ("normals", _lib.PROF_DRAWS_NORMALS),
          ("product", _lib.PROF_DRAWS_PRODUCT))


def median_ms(fn, reps):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def device_stages(gp, pts, S, reps):
    eng = gp.engine
    mask = 0
    for _, k in STAGES:
        mask |= 2 << k
    eng.profile_enable(mask)
    eng.profile_reset()
    per = {name: [] for name, _ in STAGES}
    for _ in range(reps):
        gp.sample_posterior(pts, S, seed=16, jitter=JITTER)
        for name, k in STAGES:
            per[name].append(eng.profile_read(k)["ms"])
        eng.profile_reset()
    eng.profile_enable(0)
    return {name: float(np.median(v)) for name, v in per.items()}


def host_route(gp, pts, S, reps, rng):
    parts = {"build_posterior": [], "cholesky": [], "normals": [], "matmul": []}
    total = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        mu, Sigma = gp.build_posterior(pts)
        t1 = time.perf_counter()
        L = np.linalg.cholesky(Sigma + (JITTER * np.diagonal(Sigma).max()) * np.eye(len(pts)))
        t2 = time.perf_counter()
        z = rng.standard_normal((S, len(pts)))
        t3 = time.perf_counter()
        draws = mu[None, :] + z @ L.T
        t4 = time.perf_counter()
        if rep == 0:
            continue  # discarded
        for key, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[key].append(dt)
        total.append(t4 - t0)
    assert np.isfinite(draws).all()
    return float(np.median(total)) * 1e3, {k: float(np.median(v)) * 1e3 for k, v in parts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, d = (300, 4) if a.tiny else (4096, 4)
    shapes = TINY if a.tiny else SHAPES
    if a.only is not None:
        shapes = [shapes[a.only]]
    x, y, e = wl.synthetic_dataset(16, n, d)
    gp = GpRegressor(x, y, y_err=e, hyperpars=wl.timing_theta(wl.SE, y, d), kernel=SquaredExponential)
    rng = np.random.default_rng(16)
    lines = [f"# tools/draws_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: N = {n}, d = {d}, SquaredExponential; milliseconds, "
             "medians after one discarded run; device = sample_posterior end to end, host = build_posterior + numpy",
             f"# {'(M, S)':>14s} {'device':>10s} | {'Sigma':>9s} {'factor':>9s} {'normals':>9s} {'product':>9s} | {'host':>10s} = "
             f"{'posterior':>10s} {'cholesky':>9s} {'normals':>9s} {'matmul':>9s} | {'host/device':>11s}"]
    print("\n".join(lines), flush=True)
    rows = []
    for M, S in shapes:
        pts = wl.query_points(16, M, d)
        dev = median_ms(lambda: gp.sample_posterior(pts, S, seed=16, jitter=JITTER), a.reps)
        st = device_stages(gp, pts, S, a.reps)
        host, hp = host_route(gp, pts, S, a.reps, rng)
        line = (f"{str((M, S)):>16s} {dev:10.2f} | {st['Sigma']:9.2f} {st['factor']:9.2f} {st['normals']:9.2f} {st['product']:9.2f} | "
                f"{host:10.2f} = {hp['build_posterior']:10.2f} {hp['cholesky']:9.2f} {hp['normals']:9.2f} {hp['matmul']:9.2f} | "
                f"{host / dev:11.2f}")
        print(line, flush=True)
        lines.append(line)
        rows.append({"M": M, "S": S, "device_ms": dev, "device_stages_ms": st, "host_ms": host, "host_parts_ms": hp})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out = {"tool": "draws_bench", "tiny": a.tiny, "reps": a.reps, "n": n, "d": d, "rows": rows}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
