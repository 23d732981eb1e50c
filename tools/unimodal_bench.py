"""
Timings of the device sums behind UnimodalPdf (inference_amd.pdf.UnimodalPdf over csrc/unimodal.hip).

    python tools/unimodal_bench.py [--reps 3] [--tiny] [--json out.json]

Rows, for n = 2 000, 20 000, 100 000 and 1 000 000 samples of a Gamma(3) distribution (every figure is the median of
`reps` runs after one discarded run; the entry point synchronises its stream before it returns):
  sums_1    one gpmi_unimodal_logpdf_sums call with 1 theta over the whole sample (what one evaluation of the fit costs),
            as the median over a loop of 200 calls per run
  sums_36   one call with 36 theta
  sums_72   one call with 72 theta (the fit's guesses: one launch)
  numpy_1   the same sum for 1 theta with NumPy on this machine's CPU (log_pdf_model(sample, theta).sum())
  fit       the whole constructor UnimodalPdf(sample): upload, guesses, one or two Nelder-Mead passes; with the number of
            posterior evaluations it made
`--tiny` runs every row at small sizes (the GPU test of this tool).
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/unimodal_bench.py` in a command of its own.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "inference-tools_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from inference_amd.pdf import UnimodalPdf  # noqa: E402
from inference_amd.pdf import _device  # noqa: E402
from inference_amd.pdf import unimodal as uni  # noqa: E402

LOOP = 200


def timed(fn, reps):
    fn()  # discarded
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def row(rows, name, n, ms, extra=""):
    print(f"{name:9s} n = {n:8d} {ms:12.4f} ms   {extra}", flush=True)
    rows.append({"name": name, "n": n, "ms": ms, "note": extra})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sizes = (300, 3000) if a.tiny else (2_000, 20_000, 100_000, 1_000_000)
    loop = 20 if a.tiny else LOOP
    rows = []
    rng = np.random.default_rng(9)
    for n in sizes:
        s = rng.gamma(3.0, 1.0, n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            guesses, _ = uni.guesses_and_bounds(s, s)
        thetas = np.array(guesses)
        dev = _device.DeviceUnimodal(s)
        for name, T in (("sums_1", 1), ("sums_36", 36), ("sums_72", 72)):
            th = thetas[:T]

            def calls():
                t0 = time.perf_counter()
                for _ in range(loop):
                    dev.sums(th)
                return (time.perf_counter() - t0) / loop

            ms, per = timed(calls, a.reps)
            row(rows, name, n, ms / loop, f"{n * T / (ms / loop * 1e-3):.3e} (sample, theta) terms/s")
        ms, _ = timed(lambda: [uni.log_pdf_model(s, thetas[0]).sum() for _ in range(5)], a.reps)
        row(rows, "numpy_1", n, ms / 5, "NumPy on this machine's CPU")

        evals = [0]

        class Counting(UnimodalPdf):
            def posterior_batch(self, th):
                evals[0] += len(th)
                return super().posterior_batch(th)

        def build():
            evals[0] = 0
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return Counting(s)

        ms, pdf = timed(build, a.reps)
        row(rows, "fit", n, ms, f"{evals[0]} evaluations, skip = {pdf.skip}, success = {pdf.min_result.success}, "
                                f"mode = {pdf.mode:.6g}")
        del dev, pdf

    line = {"tool": "unimodal_bench", "tiny": a.tiny, "reps": a.reps, "rows": rows}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
