"""GPU tests of the greedy inducing-point selection (gpmi_select_points, `select_inducing_points`,
`SparseGpRegressor(inducing_method="greedy")`, `reselect_inducing_points`) against the NumPy mirror tests/select_host.py.

Cases (tests/sparse_host.py), each unweighted and weighted by 1 / (y_err^2 + s^2):
  1  SE        N = 300   d = 3   m = 33    two workgroups of 256 points, the last ragged
  2  Matern52  N = 2100  d = 2   m = 130   nine workgroups, the last ragged (52 points)
  3  RQ        N = 257   d = 17  m = 64    one point in the second workgroup; no y_err: the weights are constant
  4  Matern32  N = 200   d = 64  m = 1     the widest points, one step

Allowances: the pivots equal the mirror's exactly - tests/test_select_cpu.py asserts that every margin of these runs is
at least 1e-8 and every pivot variance at least 1e-3, while the device differs from the mirror by about
(m + d + 40) 2^-53 / min pivot_var ~ 4e-12; |trace - mirror| <= 1e-10 tr_0, |pivot_var - mirror| <= 1e-10, the project's
floor.  Each test prints the device's error next to the allowance (`pytest -m gpu -s tests/test_select_gpu.py`).

Measured on one MI355X: case 1 weighted trace 1.8e-12 / 1.0e-6, pivot variances 3.1e-16 / 1e-10; case 2 weighted (through
the model) trace 2.9e-11 / 2.8e-5, pivot variances 1.6e-15 / 1e-10; bound at the greedy Z 817.466 against -1012.524 ..
-360.789 at the five random subsets; the sixteen tests together take 1.2 s."""
import ctypes as C
import pickle

import numpy as np
import pytest

import select_host as sel
import sparse_host as sh
from sparse_host import check, full_theta

pytestmark = pytest.mark.gpu

GPMI_OK, GPMI_ERR_ARG = 0, -1
RUNS = [(number, weighted) for number in (1, 2, 3, 4) for weighted in (False, True)]
SENTINEL = -7.0


def kernel_id(kind):
    from inference_amd import _lib

    return {"se": _lib.KERNEL_SE, "rq": _lib.KERNEL_RQ, "m32": _lib.KERNEL_M32, "m52": _lib.KERNEL_M52}[kind]


@pytest.fixture(scope="module")
def handle():
    from inference_amd import _lib

    h = _lib.Handle()
    yield h
    h.close()


def raw_select(h, x, theta, kernel, m_max, w=None, floor_rel=1e-8, trace_tol=0.0, n_theta=None, null=()):
    """One call of the C entry point: (status, count, index, trace, pivot_var) with the full output buffers, filled with
    a sentinel before the call.  null: names of pointer arguments passed as NULL."""
    from inference_amd._lib import dptr

    x, theta = np.ascontiguousarray(x, dtype=float), np.ascontiguousarray(theta, dtype=float)
    w = None if w is None else np.ascontiguousarray(w, dtype=float)
    index = np.full(m_max, int(SENTINEL), dtype=np.int64)
    trace, pivot_var = np.full(m_max + 1, SENTINEL), np.full(m_max, SENTINEL)
    count = C.c_int64(int(SENTINEL))
    rc = h.lib.gpmi_select_points(
        h.ctx, x.shape[0], x.shape[1], None if "x" in null else dptr(x), dptr(w), int(kernel),
        None if "theta" in null else dptr(theta), theta.size if n_theta is None else n_theta, m_max, float(floor_rel),
        float(trace_tol), None if "index" in null else index.ctypes.data_as(C.POINTER(C.c_int64)),
        None if "trace" in null else dptr(trace), None if "pivot_var" in null else dptr(pivot_var),
        None if "count" in null else C.byref(count))
    return rc, count.value, index, trace, pivot_var


def device_run(h, case, w, m_max=None, **kw):
    m_max = len(case["z"]) if m_max is None else m_max
    rc, count, index, trace, pivot_var = raw_select(h, case["x"], case["theta"], kernel_id(case["kind"]), m_max, w, **kw)
    assert rc == GPMI_OK, h.lib.gpmi_last_error(h.ctx).decode()
    assert (index[count:] == int(SENTINEL)).all() and (trace[count + 1:] == SENTINEL).all() and (pivot_var[count:] == SENTINEL).all()
    return dict(index=index[:count], trace=trace[:count + 1], pivot_var=pivot_var[:count])


def compare(label, got, want):
    assert got["index"].tolist() == want["index"].tolist(), label
    check(f"{label} trace", got["trace"], want["trace"], 1e-10 * float(want["trace"][0]))
    check(f"{label} pivot_var", got["pivot_var"], want["pivot_var"], 1e-10)


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("index", "trace", "pivot_var"))


@pytest.mark.parametrize("number,weighted", RUNS)
def test_device_equals_the_mirror(handle, number, weighted):
    case, w, want = sel.reference(number, weighted)
    got = device_run(handle, case, w)
    assert len(got["index"]) == len(case["z"])
    compare(f"case {number} weighted {weighted}", got, want)


def test_repeated_call_is_bit_identical(handle):
    case, w, _ = sel.reference(2, True)
    assert same_bits(device_run(handle, case, w), device_run(handle, case, w))


def test_position_independence(handle):
    """700 rows of weight 0 behind case 1: the same pivots, bit-identical pivot variances, the trace within the allowance
    (its sum runs over other workgroups)."""
    case, w, want = sel.reference(1, True)
    extra = np.random.default_rng(11).uniform(0.0, 1.0, size=(700, case["x"].shape[1]))
    longer = dict(case, x=np.concatenate([case["x"], extra]))
    a = device_run(handle, case, w)
    b = device_run(handle, longer, np.concatenate([w, np.zeros(700)]))
    assert a["index"].tolist() == b["index"].tolist()
    assert a["pivot_var"].tobytes() == b["pivot_var"].tobytes()
    check("appended rows: trace", b["trace"], a["trace"], 1e-10 * float(a["trace"][0]))
    compare("case 1 with 700 appended rows", b, want)


def test_zero_weights_are_never_selected(handle):
    case, w, _ = sel.reference(1, True)
    w = w.copy()
    w[0::2] = 0.0
    want = sel.select(case["kind"], case["x"], case["theta"], len(case["z"]), w)
    assert want["margin"][1:].min() >= 1e-8 and want["pivot_var"].min() >= 1e-3  # (the exact comparison's preconditions)
    got = device_run(handle, case, w)
    assert (got["index"] % 2 == 1).all()
    compare("even rows of weight 0", got, want)


def test_stop_on_trace_tol(handle):
    """trace_tol = the mirror's tr_20 / tr_0, a rounding guard of 1e-9 above it (the device's tr_20 differs from the
    mirror's in the last bits; tr_19 lies percents higher): 20 rows, a prefix of the full run bit for bit."""
    case, w, want = sel.reference(2, True)
    tol = float(want["trace"][20] / want["trace"][0]) * (1.0 + 1e-9)
    assert want["trace"][19] > tol * want["trace"][0] * (1.0 + 1e-6)
    full = device_run(handle, case, w)
    short = device_run(handle, case, w, trace_tol=tol)
    assert len(short["index"]) == 20 and len(short["trace"]) == 21
    assert short["index"].tobytes() == full["index"][:20].tobytes()
    assert short["trace"].tobytes() == full["trace"][:21].tobytes()
    assert short["pivot_var"].tobytes() == full["pivot_var"][:20].tobytes()


def test_exhausted_candidates(handle):
    x, theta = sel.duplicates()
    want = sel.select("se", x, theta, 60)
    got = device_run(handle, dict(x=x, theta=theta, kind="se", z=x), None, m_max=60)
    assert len(got["index"]) == 40
    compare("duplicates", got, want)
    for p in got["index"]:
        assert p == np.flatnonzero((x == x[p]).all(axis=1)).min()


def test_one_step_and_one_point(handle):
    case, _, want = sel.reference(1, False)
    got = device_run(handle, case, None, m_max=1)
    assert got["index"].tolist() == [0] and got["pivot_var"].tolist() == [1.0]
    check("m_max = 1: trace", got["trace"], want["trace"][:2], 1e-10 * float(want["trace"][0]))
    one = device_run(handle, dict(x=np.array([[0.3, 0.4]]), theta=np.array([0.0, -1.0, -1.0]), kind="se", z=None), None, m_max=1)
    assert one["index"].tolist() == [0] and one["trace"].tolist() == [1.0, 0.0] and one["pivot_var"].tolist() == [1.0]


def test_argument_errors_leave_the_handle_usable(handle):
    from inference_amd import _lib

    case, w, want = sel.reference(1, True)
    x, theta, kern, m = case["x"], case["theta"], kernel_id(case["kind"]), len(case["z"])
    bad_x, bad_theta = x.copy(), theta.copy()
    bad_x[5, 1], bad_theta[2] = np.nan, np.inf
    negative, infinite = w.copy(), w.copy()
    negative[3], infinite[4] = -1.0, np.inf
    calls = {
        "x NULL": dict(null=("x",)), "theta NULL": dict(null=("theta",)), "index NULL": dict(null=("index",)),
        "trace NULL": dict(null=("trace",)), "count NULL": dict(null=("count",)),
        "sum kernel": dict(kernel=_lib.KERNEL_SUM), "unknown kernel": dict(kernel=17),
        "n_theta": dict(n_theta=theta.size + 1), "n_theta of RQ": dict(kernel=_lib.KERNEL_RQ),
        "x not finite": dict(x=bad_x), "theta not finite": dict(theta=bad_theta),
        "negative weight": dict(w=negative), "infinite weight": dict(w=infinite), "no positive weight": dict(w=np.zeros(len(w))),
        "floor_rel negative": dict(floor_rel=-1e-3), "floor_rel nan": dict(floor_rel=np.nan),
        "trace_tol negative": dict(trace_tol=-1.0), "trace_tol inf": dict(trace_tol=np.inf),
        "m_max above n": dict(m_max=len(x) + 1), "m_max zero": dict(m_max=0),
    }
    for label, change in calls.items():
        args = dict(x=x, theta=theta, kernel=kern, m_max=m, w=w)
        args.update(change)
        rc, count, index, trace, pivot_var = raw_select(handle, **args)
        assert rc == GPMI_ERR_ARG, (label, rc)
        assert handle.lib.gpmi_last_error(handle.ctx).decode().startswith("gpmi_select_points: "), label
        assert (index == int(SENTINEL)).all() and (trace == SENTINEL).all() and (pivot_var == SENTINEL).all(), label
        compare(f"after '{label}'", device_run(handle, case, w), want)
    without = device_run(handle, case, w, null=("pivot_var",))  # (pivot_var_host is optional)
    assert without["index"].tolist() == want["index"].tolist()


def test_end_to_end_case_2():
    from inference_amd.gp import Matern52, SparseGpRegressor, select_inducing_points

    case, w, want = sel.reference(2, True)
    x, m = case["x"], len(case["z"])

    def model(**kw):
        return SparseGpRegressor(x, case["y"], y_err=case["e"], kernel=Matern52(), hyperpars=full_theta(case),
                                 panel_rows=case["panel"], **kw)

    gp = model(inducing_points=m, inducing_method="greedy")
    assert np.array_equal(gp.inducing_points, x[want["index"]])
    assert gp.inducing_selection["indices"].tolist() == want["index"].tolist()
    check("inducing_selection trace", gp.inducing_selection["trace"], want["trace"], 1e-10 * float(want["trace"][0]))
    check("inducing_selection pivot_variances", gp.inducing_selection["pivot_variances"], want["pivot_var"], 1e-10)
    random_bounds = [model(inducing_points=m, seed=seed).bound for seed in range(5)]
    print(f"bound: greedy {gp.bound:.3f}, random subsets {min(random_bounds):.3f} .. {max(random_bounds):.3f}")
    assert gp.bound > max(random_bounds)

    back = pickle.loads(pickle.dumps(gp))
    assert np.array_equal(back.inducing_points, gp.inducing_points)
    assert all(np.array_equal(back.inducing_selection[k], gp.inducing_selection[k]) for k in gp.inducing_selection)
    assert back.bound == gp.bound

    F0 = gp.bound
    before, after = gp.reselect_inducing_points()
    assert before == F0 and after == F0 and np.array_equal(gp.inducing_points, x[want["index"]])
    before, after = gp.reselect_inducing_points(m=65)  # (another count: the engine is built anew)
    assert before == F0 and after == gp.bound and after < F0
    assert np.array_equal(gp.inducing_points, x[want["index"][:65]])
    assert gp.inducing_selection["indices"].tolist() == want["index"][:65].tolist()
    mean, sd = gp(case["q"])
    assert np.isfinite(mean).all() and np.isfinite(sd).all()

    rows = np.sort(np.random.default_rng(3).choice(len(x), 500, replace=False))
    sub = sel.select(case["kind"], x[rows], case["theta"], 40, w[rows])
    assert sub["margin"][1:].min() >= 1e-8 and sub["pivot_var"].min() >= 1e-3
    index, trace, pivot_var = select_inducing_points(x, 40, Matern52(), case["theta"], weights=w, candidates=500, seed=3)
    assert index.tolist() == rows[sub["index"]].tolist()
    check("candidates: trace", trace, sub["trace"], 1e-10 * float(sub["trace"][0]))
    check("candidates: pivot_variances", pivot_var, sub["pivot_var"], 1e-10)
