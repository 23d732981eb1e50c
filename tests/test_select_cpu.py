"""CPU checks of the greedy inducing-point selection: the NumPy mirror (tests/select_host.py) against the dense
definition and the bound's trace term, the preconditions the device tests rest on, the duplicate set, the argument
errors of the Python layer that need no device, and the names of the C entry point.  No device call is made.

Measured here (printed by each test): trace identity at most 2.5e-14 relative; the smallest margin from step 1 on 7.2e-8
(case 1, unweighted); the smallest pivot variance 7.1e-3 (case 2, weighted).  The device differs from the mirror by about
(m + d + 40) 2^-53 / min pivot_var ~ 4e-12 relative in a score, more than three orders below that margin."""
import os
import re

import numpy as np
import pytest

import select_host as sel
import sparse_host as sh

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RUNS = [(number, weighted) for number in (1, 2, 3, 4) for weighted in (False, True)]


@pytest.mark.parametrize("number", [1, 2, 3, 4])
def test_pivots_equal_the_dense_definition(number):
    """argmax_i w_i [K - K_.S K_SS^-1 K_S.]_ii over the points not yet chosen, for the first 12 steps."""
    case, w, _ = sel.reference(number, True)
    x, steps = case["x"], 12
    run = sel.select(case["kind"], x, case["theta"], steps, w)
    C = sel.unit_cross(case["kind"], x, x, case["theta"])
    chosen = []
    for t in range(steps):
        S = np.array(chosen, dtype=int)
        cond = np.diag(C) - (np.einsum("is,si->i", C[:, S], np.linalg.solve(C[np.ix_(S, S)], C[S, :])) if t else 0.0)
        score = w * cond
        score[S] = -1.0
        chosen.append(int(np.argmax(score)))
    print(f"case {number}: dense {chosen}  mirror {run['index'][:steps].tolist()}")
    assert chosen == run["index"][:steps].tolist()


@pytest.mark.parametrize("number,weighted", RUNS)
def test_trace_is_the_trace_term_of_the_bound(number, weighted):
    """a^2 tr_m = a^2 sum w - tr H of SparseMirror(jitter = 0) at Z = x[pivots], within 1e-10 a^2 sum w."""
    case, w, run = sel.reference(number, weighted)
    ww = np.ones(len(case["x"])) if w is None else w
    mir = sh.SparseMirror(case["kind"], case["x"], case["x"][run["index"]], jitter=0.0)
    st = mir.state(case["theta"], 0.0, np.zeros(len(ww)), 1.0 / ww)
    want = st["a2"] * ww.sum() - np.trace(st["H"])
    got = st["a2"] * run["trace"][-1]
    rel = abs(got - want) / (st["a2"] * ww.sum())
    print(f"case {number} weighted {weighted}: a^2 tr_m {got:.6f}  bound's term {want:.6f}  relative difference {rel:.3g}")
    assert rel <= 1e-10


@pytest.mark.parametrize("number,weighted", RUNS)
def test_fixture_preconditions(number, weighted):
    """What the device tests rest on: float64 and long double pick the same pivots, the margins from step 1 on are at
    least 1e-8, the pivot variances at least 1e-3."""
    case, _, run = sel.reference(number, weighted)
    _, _, yard = sel.reference(number, weighted, np.longdouble)
    assert len(run["index"]) == len(case["z"])
    assert run["index"].tolist() == yard["index"].tolist()
    low = float(run["margin"][1:].min()) if len(run["margin"]) > 1 else np.inf  # (step 0 without weights is the tie of ones)
    print(f"case {number} weighted {weighted}: smallest margin from step 1 on {low:.3g}  smallest pivot variance "
          f"{run['pivot_var'].min():.3g}")
    assert low >= 1e-8
    assert run["pivot_var"].min() >= 1e-3
    assert np.all(np.diff(run["trace"]) < 0)


def test_duplicates_stop_at_the_distinct_rows():
    """40 distinct rows, each twice: 40 pivots, each the lower index of its pair."""
    x, theta = sel.duplicates()
    run = sel.select("se", x, theta, 60)
    assert len(run["index"]) == 40 and len(run["trace"]) == 41
    for p in run["index"]:
        twins = np.flatnonzero((x == x[p]).all(axis=1))
        assert len(twins) == 2 and p == twins.min()


def test_argument_errors_of_the_python_layer():
    from inference_amd.gp import SparseGpRegressor, select_inducing_points  # noqa: F401  (both names are public)
    from inference_amd.gp.sparse import select_inducing_points as from_module

    assert from_module is select_inducing_points
    x, y, e = sh.dataset(40, 2)
    with pytest.raises(ValueError, match="inducing_method"):
        SparseGpRegressor(x, y, y_err=e, inducing_points=8, inducing_method="kmeans", hyperpars=[0.0, 0.0, -1.0, -1.0])
    with pytest.raises(ValueError, match="greedy"):
        SparseGpRegressor(x, y, y_err=e, inducing_points=x[:8], inducing_method="greedy", hyperpars=[0.0, 0.0, -1.0, -1.0])


def test_entry_point_is_declared_everywhere():
    from inference_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"\bint gpmi_select_points\(gpmi_ctx\* ctx,", header)
    assert "#define GPMI_VERSION 100" in header and "#define GPMI_PROF_NCLASS 17" in header
    assert "gpmi_select_points" in _lib.SIGNATURES and len(_lib.SIGNATURES["gpmi_select_points"][1]) == 15
    version_map = open(os.path.join(ROOT, "inference-tools_amd", "csrc", "gpmi.map")).read()
    assert "gpmi_*" in version_map
    assert "select.hip" in open(os.path.join(ROOT, "inference-tools_amd", "csrc", "Makefile")).read()
