"""
Timings of the sample covariance on the device (inference_amd.mcmc.sample_covariance over csrc/cov.hip) beside numpy.cov
in the same process, and of the direction updates of a PcaChain.

    python tools/cov_bench.py [--reps 3] [--tiny] [--only K] [--out profiles/r15_cov.txt] [--json out.json]

Rows, for the shapes (10^4, 8), (10^5, 64), (10^6, 64), (10^5, 512) in C order, standard normal columns:
  device    one sample_covariance call end to end: the copy of the sample to the device from pageable memory, the two
            passes, the reduction and the copy of the matrix back (the median of `reps` runs after one discarded run)
  kernels   of that, the kernels alone, from the column sums to the scaled covariance (HIP events around them, profile
            class GPMI_PROF_COV; the median of the same runs): the rest of `device` is the copy and the call
  numpy     numpy.cov(sample.T) on this machine's CPU, the median of `reps` runs after one discarded run
Then the first five direction updates of a PcaChain with ten parameters (99, 149, 224, 336 and 504 rows): the chain runs
on numpy.cov, and at every update both routes are timed on the rows of that update, in the same way.
`--only K` runs shape K alone (0 .. 3, no chain); `--tiny` runs every row at small sizes and two updates (the GPU test of
this tool); `--out` writes the table as text.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from inference_amd import _lib  # noqa: E402
from inference_amd.mcmc import PcaChain, sample_covariance  # noqa: E402
from inference_amd.pdf import _device  # noqa: E402

SHAPES = [(10_000, 8), (100_000, 64), (1_000_000, 64), (100_000, 512)]
TINY = [(600, 5), (5_000, 70)]
CHAIN_P = 10


def kernel_ms(h):
    n, ms = C.c_int64(0), C.c_double(0.0)
    h.call("gpmi_profile_read", _lib.PROF_COV, C.byref(n), C.byref(ms), None, None)
    h.call("gpmi_profile_reset")
    return ms.value


def time_both(s, reps, h):
    """(device ms, kernels ms, numpy ms, largest difference relative to the diagonal's scale)"""
    cov = sample_covariance(s)  # discarded
    kernel_ms(h)
    dev, ker = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        cov = sample_covariance(s)
        dev.append(time.perf_counter() - t0)
        ker.append(kernel_ms(h))
    np.cov(s.T)  # discarded
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref = np.cov(s.T)
        host.append(time.perf_counter() - t0)
    d = np.sqrt(np.diag(ref))
    diff = float((np.abs(cov - ref) / np.outer(d, d)).max())
    return float(np.median(dev)) * 1e3, float(np.median(ker)), float(np.median(host)) * 1e3, diff


def chain_posterior(t):
    """Ten parameters in five pairs with a correlation of 0.9."""
    q = 0.0
    for k in range(0, CHAIN_P, 2):
        a, b = float(t[k]), float(t[k + 1]) * 2.0
        q += (a * a - 1.8 * a * b + b * b) / 0.19
    return -0.5 * q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    shapes = TINY if a.tiny else SHAPES
    if a.only is not None:
        shapes = [shapes[a.only]]
    rng = np.random.default_rng(15)
    h = _device.handle()
    h.call("gpmi_profile_enable", 2 << _lib.PROF_COV)
    rows, updates = [], []
    head = f"# {'':>8s} {'shape':>16s} {'device ms':>11s} {'kernels ms':>11s} {'numpy ms':>11s} {'numpy / device':>15s} {'max diff':>10s}"
    lines = [f"# tools/cov_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: milliseconds, medians; device = end to end, "
             "transfers included", head]
    print("\n".join(lines), flush=True)

    def report(label, s):
        dev, ker, host, diff = time_both(s, a.reps, h)
        line = f"{label:>10s} {str(s.shape):>16s} {dev:11.3f} {ker:11.3f} {host:11.3f} {host / dev:15.2f} {diff:10.1e}"
        print(line, flush=True)
        lines.append(line)
        return {"shape": list(s.shape), "device_ms": dev, "kernels_ms": ker, "numpy_ms": host, "max_diff": diff}

    for shape in shapes:
        s = rng.normal(size=shape)
        rows.append(report("device/numpy", s))
        del s

    if a.only is None:
        def covariance(sample):
            updates.append(report("update", sample))  # as the chain hands them over: the transpose of a C array
            return np.cov(sample.T)

        chain = PcaChain(chain_posterior, np.full(CHAIN_P, 0.5), widths=[0.3] * CHAIN_P, display_progress=False,
                         covariance=covariance)
        chain.rng = np.random.default_rng(16)
        want = 2 if a.tiny else 5
        while len(updates) < want:
            chain.take_step()
    h.call("gpmi_profile_enable", 0)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out = {"tool": "cov_bench", "tiny": a.tiny, "reps": a.reps, "rows": rows, "updates": updates}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
