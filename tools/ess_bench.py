"""
Timings of the batched effective sample sizes (inference_amd.mcmc.effective_sample_size_batch over csrc/acf.hip) against
a loop of the host function.

    python tools/ess_bench.py [--reps 3] [--tiny] [--only K] [--no-host] [--out profiles/r11_ess.txt] [--json out.json]

Rows, for the shapes (10^4, 64), (10^5, 64), (10^5, 4096), (10^6, 64) in C order and three kinds of column - AR(1) with
phi = 0.5, AR(1) with phi = 0.99, and a ramp (an unconverged chain: its first negative lag is at 0.21 n):
  batch     one effective_sample_size_batch call end to end: the pitched copy of the sample to the device, the layout
            pass, the centring, the rounds of lag sums with their read-backs, and the integers finished on the host
            (the median of `reps` runs after one discarded run)
  host      effective_sample_size (one FFT pair per column) over every column on this machine's CPU, one run
The device sums n (cut rounded up to its block) products per column where the FFT costs O(n log n): short cuts win by the
batching, a ramp of 10^6 rows need not.  `--only K` runs shape K alone (0 .. 3); `--tiny` runs every row at small sizes
(the GPU test of this tool); `--out` writes the table as text.
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

from inference_amd.mcmc import effective_sample_size, effective_sample_size_batch  # noqa: E402

SHAPES = [(10_000, 64), (100_000, 64), (100_000, 4096), (1_000_000, 64)]
TINY = [(600, 5), (5_000, 3)]
KINDS = ("phi=0.5", "phi=0.99", "ramp")


def draw(kind, shape, rng):
    n, p = shape
    if kind == "ramp":
        return np.arange(n)[:, None] * (0.25 + 0.001 * np.arange(p))[None, :] - 7.0
    phi = float(kind.split("=")[1])
    x = rng.normal(size=shape)
    for i in range(1, n):
        x[i] += phi * x[i - 1]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    shapes = TINY if a.tiny else SHAPES
    if a.only is not None:
        shapes = [shapes[a.only]]
    rng = np.random.default_rng(11)
    rows = []
    lines = [f"# tools/ess_bench.py --reps {a.reps}{' --tiny' if a.tiny else ''}: milliseconds end to end, transfers included",
             f"# {'shape':>16s} {'kind':>9s} {'cut (min .. max)':>18s} {'batch ms':>11s} {'host ms':>11s} {'host / batch':>13s}"]
    print("\n".join(lines), flush=True)
    for shape in shapes:
        for kind in KINDS:
            s = draw(kind, shape, rng)
            effective_sample_size_batch(s)  # discarded
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ess, f0, total, cut = effective_sample_size_batch(s, details=True)
                ts.append(time.perf_counter() - t0)
            batch_ms = float(np.median(ts)) * 1e3
            host_ms = None
            if not a.no_host:
                t0 = time.perf_counter()
                ref = np.array([effective_sample_size(s[:, c]) for c in range(shape[1])])
                host_ms = (time.perf_counter() - t0) * 1e3
                if shape[0] % 2 == 0:  # (an odd length follows the reference's shorter inverse transform on the host)
                    assert (np.abs(ref - ess) <= 1).all(), "device and host disagree"
            ratio = f"{host_ms / batch_ms:13.2f}" if host_ms is not None else f"{'-':>13s}"
            host_txt = f"{host_ms:11.2f}" if host_ms is not None else f"{'-':>11s}"
            line = f"batch/host {str(shape):>7s} {kind:>9s} {f'{cut.min()} .. {cut.max()}':>18s} {batch_ms:11.2f} {host_txt} {ratio}"
            print(line, flush=True)
            lines.append(line)
            rows.append({"shape": list(shape), "kind": kind, "cut_min": int(cut.min()), "cut_max": int(cut.max()),
                         "batch_ms": batch_ms, "host_ms": host_ms})
            del s
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    out = {"tool": "ess_bench", "tiny": a.tiny, "reps": a.reps, "rows": rows}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
