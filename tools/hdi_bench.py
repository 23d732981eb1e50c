"""
Timings of the batched highest-density intervals (inference_amd.pdf.sample_hdi_batch over csrc/hdi.hip).

    python tools/hdi_bench.py [--reps 3] [--tiny] [--only K] [--no-host] [--json out.json]

Rows, for the 2D shapes (2000, 200), (10^4, 10^3), (10^5, 10^2), (10^5, 10^3) in C order and the 1D samples n = 10^6 and
10^7, fractions (0.65, 0.95), normal draws:
  batch     one sample_hdi_batch call end to end: validation, the pitched copy of the sample to the device, the layout
            pass, the sorts, the window scans and the copy back (the median of `reps` runs after one discarded run; the
            entry point synchronises its stream before it returns)
  batch_T   the same for the transposed view of the (m, n) C array (the layout hdi_plot gets when the user passes
            (len(x), n)): no layout pass
  host      the host sample_hdi once per fraction on this machine's CPU (a single run: it sorts a copy per call)
`--only K` runs shape K alone (0 .. 5); `--tiny` runs every row at small sizes (the GPU test of this tool).
Kernel times and the split between copy, layout pass, chunk sort, merge passes and window scan: run one shape under
`rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/hdi_bench.py --only K --reps 1 --no-host` in a
command of its own (two calls are traced: the discarded one and the timed one).
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

from inference_amd.pdf import sample_hdi, sample_hdi_batch  # noqa: E402

FRACTIONS = (0.65, 0.95)
SHAPES = [(2_000, 200), (10_000, 1_000), (100_000, 100), (100_000, 1_000), (1_000_000,), (10_000_000,)]
TINY = [(300, 20), (9_000, 3), (20_000,)]


def timed(fn, reps):
    fn()  # discarded
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def row(rows, name, shape, ms, extra=""):
    print(f"{name:8s} {str(shape):16s} {ms:12.3f} ms   {extra}", flush=True)
    rows.append({"name": name, "shape": list(shape), "ms": ms, "note": extra})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    shapes = TINY if a.tiny else SHAPES
    if a.only is not None:
        shapes = [shapes[a.only]]
    rows = []
    rng = np.random.default_rng(10)
    warnings.simplefilter("ignore")
    for shape in shapes:
        s = rng.normal(size=shape)
        mb = s.nbytes / 1e6
        ms, dev = timed(lambda: sample_hdi_batch(s, FRACTIONS), a.reps)
        row(rows, "batch", shape, ms, f"{mb:.1f} MB sample, {mb / ms:.2f} GB/s of sample end to end")
        if len(shape) == 2:
            t = np.ascontiguousarray(s.T)
            ms, dev_t = timed(lambda: sample_hdi_batch(t.T, FRACTIONS), a.reps)
            row(rows, "batch_T", shape, ms, "column-contiguous view: no layout pass")
            assert np.array_equal(dev, dev_t)
            del t
        if not a.no_host:
            t0 = time.perf_counter()
            ref = np.stack([sample_hdi(s, f) for f in FRACTIONS])
            row(rows, "host", shape, (time.perf_counter() - t0) * 1e3, "sample_hdi per fraction, this machine's CPU, one run")
            assert np.array_equal(dev, ref), "device and host disagree"
        del s

    line = {"tool": "hdi_bench", "tiny": a.tiny, "reps": a.reps, "fractions": list(FRACTIONS), "rows": rows}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
