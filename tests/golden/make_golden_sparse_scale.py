"""
Maker of tests/golden/sparse_scale.npz: the NumPy mirrors' values for the sparse model and the greedy selection at the
shapes where the device's schedules change (tests/sparse_host.py: SCALE_CASES, `scale_case`, `select_case`), with the
allowance of every quantity.  CPU only; it imports the mirrors under tests/ and nothing of the device path.

    python tests/golden/make_golden_sparse_scale.py [case ...]

Per case `c` the file holds c/F, c/grad (the full gradient [mean, kernel parameters, (ln s)]), c/gz (dF/dZ), c/alpha at
the 512 indices c/alpha_idx, c/mean and c/var at the case's 17 query points, c/allow and c/spread in the order of
QUANTITIES, c/ripples, c/cond = cond(K_mm + eps I), the first and last rows of x and Z (c/x_ends, c/z_ends: the test
regenerates the inputs and compares them bit for bit) and the numbers of the conditions asserted below.

Allowances (the project's rule, measured against the mirror and never against the device): a quantity's allowance is
10 x its largest movement under ripples of 1e-13 relative on the mirror's K_mm, K_mn and K_mq, floored at 1e-10 of its
scale.  48 ripples per case, except run16 (8) and max_m (6), whose evaluations take a minute and half a minute on the two
BLAS threads of a worker.

Conditions asserted here, so that a passing device test means something:
  - cond(K_mm + eps I) <= 1e4 for every case but bench_like, whose condition number is only recorded;
  - run4, run8, run16: the part of dF/dZ that comes from the data rows in the third and later 64-row tiles of their run
    (the run length of the schedule in SCALE_SCHEDULE) exceeds 1e3 x the allowance of dF/dZ in every 64-point tile of Z -
    a kernel that dropped or double-counted those tiles cannot pass; max_m: the same for the K_mm term and its runs of 8;
  - long: the rows >= 262144 (the second trip of the weights pass) move F, sum w and the noise gradient by more than
    1e3 x their allowances;
  - the selection (n = 66000, weighted and unweighted): float64 and long-double pivots identical, every margin from step
    1 on >= 1e-9, every pivot variance >= 1e-2, and the bound on the device's deviation, (m + d + 40) 2^-53 / min pivot
    variance, at least 1e4 below the smallest margin.

The cases run in four worker processes with two BLAS threads each (set before NumPy is imported: the thread count is part
of what fixes the bits).  Measured on an 8-core host: 8.6 minutes for the whole file (run16 alone 515 s, max_m 251 s, bench_like
185 s, run8 156 s, run4 50 s); a second run reproduced tiles3, long, run4 and the selection bit for bit.
"""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "2"

import multiprocessing as mp
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "inference-tools_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import select_host as sel  # noqa: E402
import sparse_host as sh  # noqa: E402
import sparse_z_host as szh  # noqa: E402

OUT = os.path.join(HERE, "sparse_scale.npz")
QUANTITIES = ("F", "grad", "gz", "alpha", "mean", "var")
RIPPLES = {name: sh.N_RIPPLES for name in sh.SCALE_NAMES}
RIPPLES.update(run16=8, max_m=6)
RUN_TILES = {"run4": 4, "run8": 8, "run16": 16, "max_m": 8}  # (asserted against gpmi_sgp_schedule in test_sparse_scale_cpu.py)
LONG_HEAD = 262144  # rows of `long` the first trip of the weights pass covers: 1024 workgroups of 256


def tile_maxima(part):
    """max |part| over each tile of 64 inducing points"""
    m = len(part)
    return np.array([np.abs(part[i:i + 64]).max() for i in range(0, m, 64)])


def make_case(name):
    t0 = time.time()
    case = sh.scale_case(name)
    n, m = len(case["x"]), len(case["z"])
    mir = sh.SparseMirror(case["kind"], case["x"], case["z"])
    cond = mir.cond_kmm(case["theta"])
    data_rows = sh.later_tile_rows(n, RUN_TILES[name]) if name in ("run4", "run8", "run16") else None
    z_rows = sh.later_tile_rows(m, RUN_TILES[name]) if name == "max_m" else None
    base = szh.all_quantities(case, mir, data_rows=data_rows, z_rows=z_rows)
    moved = [szh.all_quantities(case, mir, sh.rippler(1000 * case["number"] + i)) for i in range(RIPPLES[name])]
    allow, spread = szh.allowances(base, moved, np.exp(2.0 * case["theta"][0]))
    out = {k: base[k] for k in ("F", "grad", "gz", "mean", "var")}
    idx = np.sort(np.random.default_rng(600 + case["number"]).choice(n, min(512, n), replace=False))
    out.update(alpha_idx=idx, alpha=base["alpha"][idx], allow=np.array([allow[k] for k in QUANTITIES]),
               spread=np.array([spread[k] for k in QUANTITIES]), ripples=np.array(RIPPLES[name]), cond=np.array(cond),
               x_ends=case["x"][[0, -1]], z_ends=case["z"][[0, -1]])
    if name != "bench_like":
        assert cond <= 1e4, (name, cond)
    if data_rows is not None or z_rows is not None:
        part = base["gz_data_part" if data_rows is not None else "gz_kmm_part"]
        out["later_tiles_part"] = tile_maxima(part)
        assert out["later_tiles_part"].min() > 1e3 * allow["gz"], (name, out["later_tiles_part"].min(), allow["gz"])
    if name == "long":
        head = dict(case, x=case["x"][:LONG_HEAD], y=case["y"][:LONG_HEAD], e=case["e"][:LONG_HEAD])
        cut = szh.all_quantities(head, sh.SparseMirror(case["kind"], head["x"], case["z"]))
        w = 1.0 / (case["e"] ** 2 + case["white"])
        moves = np.array([abs(base["F"][0] - cut["F"][0]), w[LONG_HEAD:].sum(), abs(base["grad"][-1] - cut["grad"][-1])])
        floors = np.array([allow["F"], 1e-10 * w.sum(), allow["grad"]])
        out.update(tail_moves=moves, tail_allow=floors)
        assert (moves > 1e3 * floors).all(), (moves, floors)
    print(f"{name}: cond {cond:.3g}, " + ", ".join(f"{k} {spread[k]:.2e} -> {allow[k]:.2e}" for k in QUANTITIES)
          + f" ({RIPPLES[name]} ripples, {time.time() - t0:.0f} s)", flush=True)
    return name, out


def make_selection():
    x, theta, w = sh.select_case()
    out = {}
    for label, weights in (("weighted", w), ("unweighted", None)):
        run = sel.select("m52", x, theta, sh.SELECT_M, weights)
        wide = sel.select("m52", x, theta, sh.SELECT_M, weights, dtype=np.longdouble)
        assert run["index"].tolist() == wide["index"].tolist() and len(run["index"]) == sh.SELECT_M, label
        margin, pv = float(run["margin"][1:].min()), float(run["pivot_var"].min())
        deviation = (sh.SELECT_M + x.shape[1] + 40) * 2.0**-53 / pv
        assert margin >= 1e-9 and pv >= 1e-2 and deviation * 1e4 <= margin, (label, margin, pv, deviation)
        print(f"selection {label}: smallest margin {margin:.2e}, smallest pivot variance {pv:.3f}, deviation bound "
              f"{deviation:.1e}", flush=True)
        out.update({f"{label}_index": run["index"], f"{label}_trace": run["trace"], f"{label}_pivot_var": run["pivot_var"],
                    f"{label}_margin": run["margin"]})
    out["x_ends"] = x[[0, -1]]
    return "select", out


def _make(name):
    return make_selection() if name == "select" else make_case(name)


def main(names):
    t0 = time.time()
    order = sorted(names, key=lambda nm: -{"max_m": 5, "run8": 4, "bench_like": 3, "run16": 2}.get(nm, 0))
    with mp.get_context("spawn").Pool(4) as pool:
        parts = dict(pool.map(_make, order, chunksize=1))
    flat = {f"{name}/{k}": np.asarray(v) for name in names for k, v in parts[name].items()}
    if set(names) != set(sh.SCALE_NAMES) | {"select"} and os.path.exists(OUT):  # some cases again: the others are kept
        old = dict(np.load(OUT))
        old.update(flat)
        flat = old
    np.savez_compressed(OUT, **{k: flat[k] for k in sorted(flat)})
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main(sys.argv[1:] or list(sh.SCALE_NAMES) + ["select"])
