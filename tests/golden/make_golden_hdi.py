"""
Golden vectors of the reference's sample_hdi (pdf/hdi.py), hdi_plot and trace_plot (plotting.py:306-454), written to
hdi.npz beside this file by IMPORTING the reference the way make_golden.py does (its module level sets that import up;
the file itself is not changed).  Data only (allow_pickle=False).

Run in the build container only:   python tests/golden/make_golden_hdi.py

The inputs are the seeded recipes of tests/hdi_host.py (`case`); of each, the archive holds the first and last 8 values
(`<case>_ends`), which the tests compare before they trust the recipe, and the small ones whole (`<case>_sample`).

Cases (prefix in the archive; `<case>_hdi` is the stack of sample_hdi(sample, f) over `<case>_fractions`)
  edge_<n>    n = 2^k - 1, 2^k, 2^k + 1 for k = 10 .. 15, 3 columns: power-of-two and chunk edges, the first merge
  tiny_<n>    n = 2, 3, 5, 63, 64, 65, 257, 4 columns, window lengths 0 and n - 1 included (stored whole)
  runs_<n>    n = 3 2^14 + 5, 5 2^13 + 1, 100 003 (2 columns) and 1 000 003 (1 column): odd and even numbers of runs
  layout      (257, 129): every column count and view of the layout tests is a slice of it; layout_half is a[::2]
  tie_small   rng.integers(0, 5) as floats (50, 4), a constant column and a column of two values (stored whole)
  tie_big     the same at (20 000, 3)
  nf_small    (40, 6) with a NaN in column 1, +inf in column 3, -inf and +inf in column 4 (stored whole)
  nf_big      the same at (20 000, 6)
  band_a/b    hdi_plot's bands for a (400, 60) and a (60, 400) sample at intervals (0.95, 0.35, 0.65), read off the
              polygons that the reference drew under the Agg backend (lower / upper, highest interval first)
  trace       trace_plot's y-limits and y-ticks of five parameters of 3000 samples, read off the figure it returns
  ragged      the same for five samples of different lengths
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.pdf import sample_hdi  # noqa: E402
from inference.plotting import hdi_plot, trace_plot  # noqa: E402

import hdi_host as hh  # noqa: E402

OUT = {}


def record(name, fractions, sample=None, store=False):
    s = hh.case(name) if sample is None else sample
    if sample is None:
        OUT[f"{name}_ends"] = hh.ends(s)
    if store:
        OUT[f"{name}_sample"] = s
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        OUT[f"{name}_hdi"] = np.stack([sample_hdi(s, f).reshape(2, -1) for f in fractions])
    OUT[f"{name}_fractions"] = np.array(fractions)
    return s


def bands(name):
    import matplotlib.pyplot as plt

    s = hh.case(name)
    OUT[f"{name}_ends"] = hh.ends(s)
    x = np.linspace(0.0, 1.0, 60)
    _, ax = plt.subplots()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hdi_plot(x, s, intervals=hh.BAND_INTERVALS, axis=ax)
    lower, upper = [], []
    for poly in ax.collections:  # fill_between: (x0, y2_0), (x, y1), (x_end, y2_end), (x, y2) reversed
        v = poly.get_paths()[0].vertices
        np.testing.assert_array_equal(v[1:61, 0], x)
        lower.append(v[1:61, 1])
        upper.append(v[62:122, 1][::-1])
    OUT[f"{name}_lower"], OUT[f"{name}_upper"] = np.array(lower), np.array(upper)
    OUT[f"{name}_labels"] = np.array([p.get_label() for p in ax.collections])
    # what was drawn is sample_hdi of the columns, highest interval first
    cols = s if s.shape[1] == 60 else s.T
    for k, f in enumerate(sorted(hh.BAND_INTERVALS, reverse=True)):
        ref = sample_hdi(cols, f)
        np.testing.assert_array_equal(ref, [lower[k], upper[k]])
    plt.close("all")


def trace(name):
    import matplotlib.pyplot as plt

    samples = hh.case(name)
    OUT[f"{name}_ends"] = hh.ends(samples)
    fig = trace_plot([s for s in samples], show=False)
    OUT[f"{name}_limits"] = np.array([ax.get_ylim() for ax in fig.axes])
    OUT[f"{name}_ticks"] = np.array([ax.get_yticks() for ax in fig.axes])
    OUT[f"{name}_labels"] = np.array([ax.get_ylabel() for ax in fig.axes])
    plt.close("all")


def main():
    for n in hh.EDGE_N:
        record(f"edge_{n}", hh.FRACTIONS)
    for n in hh.TINY_N:
        record(f"tiny_{n}", hh.TINY_FRACTIONS, store=True)
    for n, _ in hh.RUNS:
        record(f"runs_{n}", hh.FRACTIONS)
    a = record("layout", hh.FRACTIONS)
    record("layout_half", hh.FRACTIONS, sample=a[::2])
    t = record("tie_small", hh.TIE_FRACTIONS, store=True)
    print("tie_small at 0.5:", sample_hdi(t[:, :4], 0.5).tolist())
    record("tie_big", hh.TIE_FRACTIONS)
    record("nf_small", hh.FRACTIONS, store=True)
    record("nf_big", hh.FRACTIONS)
    bands("band_a")
    bands("band_b")
    trace("trace")
    trace("ragged")
    path = os.path.join(HERE, "hdi.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
