"""
NumPy mirror of the greedy conditional-variance selection behind `select_inducing_points` and gpmi_select_points
(include/gpmi.h): the pivoted partial Cholesky factorisation of C = K / a^2.  The kernels come from tests/matern_host.py
(formulas, not the package's code); the cases from tests/sparse_host.py.

    d_i = 1, tr_0 = sum w_i;  step t: p = argmax over {d_i > floor_rel, w_i > 0} of w_i d_i (numpy.argmax: the lowest
    index among equals), c = C(x, x_p) - V[:t].T V[:t, p], V[t] = c / sqrt(d_p), d <- max(d - V[t]^2, 0), d_p <- 0,
    tr_{t+1} = sum w_i d_i;  stop when nothing is eligible, at t = m_max, or when tr_t <= trace_tol tr_0.

`dtype`: the arithmetic's type; numpy.longdouble gives the yardstick the float64 run is compared with.
"""
import numpy as np

import matern_host as mh
import sparse_host as sh


def unit_cross(kind, u, v, theta, dtype=np.float64):
    """C(u, v) = K / a^2 in `dtype` (matern_host.profiles on s = 1/2 sum_k ((u_k - v_k) / l_k)^2)."""
    _, kappa, scales = mh.split(kind, theta)
    u, v, scales = np.asarray(u, dtype), np.asarray(v, dtype), np.asarray(scales, dtype)
    s = np.zeros((len(u), len(v)), dtype)
    for k in range(u.shape[1]):
        s += dtype(0.5) * ((u[:, None, k] - v[None, :, k]) / scales[k]) ** 2
    return mh.profiles(kind, s, None if kappa is None else dtype(kappa))[0]


def select(kind, x, theta, m_max, weights=None, floor_rel=1e-8, trace_tol=0.0, dtype=np.float64):
    """dict(index (count,), trace (count + 1,), pivot_var (count,), margin (count,)): margin[t] is the top score of step t
    minus the runner-up's, relative to the top score (inf when one point alone was eligible)."""
    x = np.asarray(x, dtype)
    n = len(x)
    w = np.ones(n, dtype) if weights is None else np.asarray(weights, dtype)
    d = np.ones(n, dtype)
    V = np.zeros((m_max, n), dtype)
    index, pivot_var, margin, trace = [], [], [], [w.sum()]
    for t in range(m_max + 1):
        eligible = (d > floor_rel) & (w > 0)
        if not eligible.any() or t == m_max or trace[t] <= trace_tol * trace[0]:
            break
        score = np.where(eligible, w * d, -1.0)
        p = int(np.argmax(score))
        rest = np.delete(score, p)
        rest = rest[rest >= 0]
        margin.append(float((score[p] - rest.max()) / score[p]) if len(rest) else np.inf)
        c = unit_cross(kind, x, x[p:p + 1], theta, dtype)[:, 0] - V[:t].T @ V[:t, p]
        V[t] = c / np.sqrt(d[p])
        index.append(p)
        pivot_var.append(d[p])
        d = np.maximum(d - V[t] ** 2, 0)
        d[p] = 0
        trace.append((w * d).sum())
    return dict(index=np.array(index, dtype=np.int64), trace=np.array(trace, dtype), pivot_var=np.array(pivot_var, dtype),
                margin=np.array(margin))


def noise_weights(case):
    """1 / (y_err^2 + s^2) of a case of sparse_host.case, or None where it has no y_err."""
    return None if case["e"] is None else 1.0 / (case["e"] ** 2 + case["white"])


def duplicates(seed=7):
    """40 distinct rows of the unit square, each twice, shuffled: (x (80, 2), theta of SE with l = 0.05)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 1.0, size=(40, 2))
    x = np.concatenate([base, base])[rng.permutation(80)]
    return np.ascontiguousarray(x), np.array([0.0, np.log(0.05), np.log(0.05)])


_RUNS = {}


def reference(number, weighted, dtype=np.float64):
    """The mirror's run of sparse_host.case(number) at its own theta and m, computed once and shared: treat it as read-only."""
    key = (number, weighted, np.dtype(dtype).name)
    if key not in _RUNS:
        case = sh.case(number)
        w = noise_weights(case) if weighted else None
        if weighted and w is None:  # (case 3 has no y_err: its noise weights are constant, the selection is the unweighted one)
            w = np.full(len(case["x"]), 1.0 / case["white"])
        _RUNS[key] = (case, w, select(case["kind"], case["x"], case["theta"], len(case["z"]), w, dtype=dtype))
    return _RUNS[key]
