"""
Host side of the tests of the lockstep batches of the sparse model (gpmi_sgp_bound_batch,
`SparseGpRegressor.marginal_likelihood_batch` / `_gradient_batch`): the row sets, their mirror values and allowances, the
failing row.  Cases, mirror, ripples and `check` are those of tests/sparse_host.py.

A row set of a case: the case's theta in row 0 and six seeded perturbations, each of which moves every log-parameter
(ln a, ln kappa, ln l_k, ln s) by up to +-0.3 and draws the constant mean from {MU, MU +- 0.5}.  ROW_SEED is the first seed
from 700 on at which every row of the four cases meets the conditioning bounds tests/test_sparse_batch_cpu.py asserts
on the mirror (case 2 itself stands at cond 7.9e3 of the 1e4 allowed: longer length scales leave the bound).

Allowances (the convention of tests/test_sparse_gpu.py), per row and per quantity: 10 x the largest movement under
ripples of 1e-13 on the mirror's K_mm and K_mn, floored at 1e-10 of the quantity's scale.  48 ripples per row.  The mirror's small matrices run on one BLAS thread where
threadpoolctl is installed (many threads on 130 x 130 matrices cost a hundred times the arithmetic).
"""
import numpy as np

import sparse_host as sh
from sparse_host import MU

N_ROWS = 7
ROW_SEED = 755
BATCH_CASES = (1, 2, 3, 5)
FAIL_POSITION, FAIL_ROWS = 2, 5  # the failure test: the failing row's place among the rows of its batch


def row_set(case):
    """(N_ROWS, P) full hyper-parameter vectors [mean | kernel parameters | (ln s)] of the case."""
    base = sh.full_theta(case)
    rng = np.random.default_rng(ROW_SEED + case["number"])
    rows = [base]
    for _ in range(N_ROWS - 1):
        t = base.copy()
        t[1:] += rng.uniform(-0.3, 0.3, size=len(base) - 1)
        t[0] = MU + rng.choice([-0.5, 0.0, 0.5])
        rows.append(t)
    return np.array(rows)


def split_row(case, row):
    """A full vector -> (constant mean, the kernel's theta, the WhiteNoise variance)."""
    if case["white"] > 0.0:
        return float(row[0]), np.array(row[1:-1]), float(np.exp(2.0 * row[-1]))
    return float(row[0]), np.array(row[1:]), 0.0


def noise_var(case):
    return None if case["e"] is None else case["e"] ** 2


def mirror_row(case, mir, row, mean_vector=None, mean_features=None, ripple=None):
    """The mirror's F, full gradient and alpha of one row.  mean_vector / mean_features: mu(x) and the rows d mu / d theta_j
    of another mean function than the constant (then row[:len(mean_features)] are its parameters)."""
    mir.ripple = ripple or (lambda name, A: A)
    white = case["white"] > 0.0
    n_mean = 1 if mean_features is None else len(mean_features)
    theta = np.array(row[n_mean:-1] if white else row[n_mean:])
    wv = float(np.exp(2.0 * row[-1])) if white else 0.0
    mu = row[0] if mean_vector is None else mean_vector
    F, g, alpha = mir.bound_and_gradient(theta, wv, case["y"] - mu, noise_var(case))
    gmean = [alpha.sum()] if mean_features is None else [float(f @ alpha) for f in mean_features]
    return dict(F=np.array([F]), grad=np.concatenate([gmean, g if white else g[:-1]]), alpha=alpha)


def reference_row(case, row, n_ripples, seed, **mean):
    """(mirror quantities, allowances) of one row."""
    mir = sh.SparseMirror(case["kind"], case["x"], case["z"])
    base = mirror_row(case, mir, row, **mean)
    spread = {k: 0.0 for k in base}
    for i in range(n_ripples):
        moved = mirror_row(case, mir, row, ripple=sh.rippler(seed + i), **mean)
        for k in base:
            spread[k] = max(spread[k], float(np.abs(moved[k] - base[k]).max()))
    allow = {k: max(10.0 * spread[k], 1e-10 * float(np.abs(base[k]).max())) for k in base}
    return base, allow


def one_blas_thread():
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        from contextlib import nullcontext

        return nullcontext()
    return threadpool_limits(limits=1)


_REFERENCE = {}


def reference(number):
    """(case, rows (N_ROWS, P), [mirror quantities per row], [allowances per row]), computed once per case."""
    if number not in _REFERENCE:
        case = sh.case(number)
        rows = row_set(case)
        with one_blas_thread():
            both = [reference_row(case, row, sh.N_RIPPLES, 100000 * number + 1000 * t) for t, row in enumerate(rows)]
        _REFERENCE[number] = (case, rows, [b for b, _ in both], [a for _, a in both])
    return _REFERENCE[number]


def cond_rows(case, rows, jitter=1e-8):
    """cond(K_mm + jitter a^2 I) of the mirror for every row."""
    mir = sh.SparseMirror(case["kind"], case["x"], case["z"], jitter=jitter)
    return np.array([mir.cond_kmm(split_row(case, row)[1]) for row in rows])


def failing_row(case):
    """SE with ln a = 0 and ln l_k = 25: s <= 1e-20 for points of the unit cube, the kernel's exponential returns exactly 1
    and K_mm is the all-ones matrix - at jitter 0 its second pivot is exactly 0 in any elimination order."""
    assert case["kind"] == "se" and case["white"] > 0.0
    d = case["x"].shape[1]
    return np.array([MU, 0.0] + [25.0] * d + [0.5 * np.log(case["white"])])


def failure_rows(case):
    """The five rows of the failure test: rows 0..3 of the row set with the failing row put at FAIL_POSITION."""
    rows = list(row_set(case)[:FAIL_ROWS - 1])
    rows.insert(FAIL_POSITION, failing_row(case))
    return np.array(rows)


def make_gp(case, jitter=1e-8, mean=None, hyperpars="case", **kwargs):
    """`sparse_host.make_gp` with a mean function and hyper-parameters of the caller's (None: the constructor searches)."""
    from inference_amd.gp import ConstantMean, Matern32, Matern52, RationalQuadratic, SparseGpRegressor, SquaredExponential, WhiteNoise

    kern = {"se": SquaredExponential, "m52": Matern52, "m32": Matern32, "rq": RationalQuadratic}[case["kind"]]()
    if case["white"] > 0.0:
        kern = kern + WhiteNoise()
    return SparseGpRegressor(case["x"], case["y"], y_err=case["e"], inducing_points=case["z"], kernel=kern,
                             mean=ConstantMean if mean is None else mean,
                             hyperpars=sh.full_theta(case) if isinstance(hyperpars, str) else hyperpars, jitter=jitter,
                             panel_rows=case["panel"], **kwargs)


def bits(a):
    return np.ascontiguousarray(a, dtype=float).tobytes()
