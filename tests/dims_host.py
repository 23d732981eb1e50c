"""
Inputs and a second yardstick for the tests of 17 .. 64 spatial dimensions (tests/test_dimensions_cpu.py,
tests/test_dimensions_gpu.py).  The oracle of every quantity is tests/matern_host.py (HostModel, OracleGp), which works at
any d; what this module adds:

  * `theta_dims`: hyper-parameters whose length scales grow like sqrt(d).  With `matern_host.theta_for` as it is
    (l in [0.7, 2], x in [0, 4]^d) s = 1/2 sum_k dx_k^2 / l_k^2 grows like d: at d = 64 every off-diagonal element of a
    SquaredExponential K is below 1e-12 of the diagonal (Matern: 1e-4, RationalQuadratic: 0.02), K is its own diagonal,
    and a kernel that dropped the axes 16 .. 63 altogether would still agree with the oracle in L, alpha, the likelihoods
    and the predictions.  1/2 ln d on every ln l_k keeps s, and with it the correlations, at what they are at d = 1
    (test_dimensions_cpu.py holds both statements).
  * `cross_ld`: the four covariance functions in np.longdouble, written from the formulas in matern_host's docstring - the
    float64 oracle's own rounding at these d, measured instead of assumed.
  * `model_theta`, `MODELS`: the models of the regressor tests and their parameter vectors.
"""
import numpy as np

import matern_host as mh

DIMS = (17, 32, 33, 63, 64)
KINDS = ("se", "rq", "m32", "m52")


# seeds of `theta_dims` for the single-kernel cases; 0 unless that draw violates a condition of test_dimensions_cpu.py
# (se, d = 32, seed 0: one length-scale component of the leave-one-out gradient at 8e-6 of the largest, below the 1e-5
# the element-wise comparison needs)
SEEDS = {("se", 32): 1}


def seed_for(kind, d):
    return SEEDS.get((kind, d), 0)


def theta_dims(kind, d, seed=0):
    """`matern_host.theta_for` with 1/2 ln d added to every ln l_k: a = e^0.2, l in sqrt(d) [0.7, 2]."""
    th = mh.theta_for(kind, d, seed)
    th[1 + mh.n_shape(kind):] += 0.5 * np.log(d)
    return th


def cross_ld(kind, u, v, theta):
    """a^2 C(s) between the rows of u and v in np.longdouble (every operation, exp / sqrt / power included)."""
    ld = np.longdouble
    theta = np.asarray(theta, dtype=ld)
    u, v = np.asarray(u, dtype=ld), np.asarray(v, dtype=ld)
    a2 = np.exp(2 * theta[0])
    scales = np.exp(theta[1 + mh.n_shape(kind):])
    s = np.zeros((len(u), len(v)), dtype=ld)
    for k in range(u.shape[1]):
        s += ((u[:, None, k] - v[None, :, k]) / scales[k]) ** 2
    s *= ld(1) / 2
    if kind == "se":
        C = np.exp(-s)
    elif kind == "rq":
        kappa = np.exp(theta[1])
        C = (1 + s / kappa) ** -kappa
    elif kind == "m32":
        t = np.sqrt(6 * s)
        C = (1 + t) * np.exp(-t)
    elif kind == "m52":
        t = np.sqrt(10 * s)
        C = (1 + t + t * t / 3) * np.exp(-t)
    else:
        raise ValueError(kind)
    assert C.dtype == ld
    return a2 * C


# the models of the regressor tests: `parts` of matern_host.HostModel, the ChangePoint's axis filled in with d - 1
MODELS = {
    "se": lambda d: [("se",)],
    "rq": lambda d: [("rq",)],
    "m52": lambda d: [("m52",)],
    "se+wn": lambda d: [("se",), ("wn",)],
    "se+rq": lambda d: [("se",), ("rq",)],
    "se+rq+m32+m52": lambda d: [("se",), ("rq",), ("m32",), ("m52",)],
    "cp[se,rq]": lambda d: [("cp", ("se", "rq"), d - 1)],
}


def model_theta(parts, d, seed=0):
    """[mean, the parts' parameters back to back], length scales from `theta_dims`; the components of a sum get different
    seeds and amplitudes (e^0.2, e^-0.1, ...), the ChangePoint sits at 2.0 on its axis with width 0.5."""
    out = [0.1]
    for i, p in enumerate(parts):
        if p[0] == "wn":
            out.append(np.log(0.15))
        elif p[0] == "cp":
            for j, k in enumerate(p[1]):
                out.extend(theta_dims(k, d, seed + 10 * j))
            out.extend([2.0, 0.5])
        else:
            th = theta_dims(p[0], d, seed + i)
            th[0] -= 0.3 * i
            out.extend(th)
    return np.array(out, dtype=float)


def scale_slices(parts, d):
    """Index arrays into a full theta (mean first) of the length-scale entries, one per stationary kernel of the model."""
    out, pos = [], 1
    for p in parts:
        if p[0] == "wn":
            pos += 1
        elif p[0] == "cp":
            for k in p[1]:
                out.append(np.arange(pos + 1 + mh.n_shape(k), pos + 1 + mh.n_shape(k) + d))
                pos += d + 1 + mh.n_shape(k)
            pos += 2
        else:
            out.append(np.arange(pos + 1 + mh.n_shape(p[0]), pos + 1 + mh.n_shape(p[0]) + d))
            pos += d + 1 + mh.n_shape(p[0])
    return out


def batch_thetas(parts, d, T):
    """T parameter vectors of one model with different length scales (seeds 0 .. T - 1 of `theta_dims`), amplitudes
    (ln a shifted by -0.2 .. 0.2) and means."""
    assert all(p[0] != "cp" for p in parts)
    rows = []
    for t in range(T):
        th = model_theta(parts, d, seed=t)
        for p, sl in zip([q for q in parts if q[0] != "wn"], scale_slices(parts, d)):
            th[sl[0] - 1 - mh.n_shape(p[0])] += 0.2 * (2.0 * t / max(T - 1, 1) - 1.0)
        th[0] += 0.02 * t
        rows.append(th)
    return np.array(rows)


def truncated(parts, x, theta, keep=16):
    """The same model on the first `keep` axes only - x[:, :keep] and the matching length scales - as (parts, x, theta,
    index of the kept entries in the full theta): what a kernel that ignored the axes >= keep would compute.  (A
    ChangePoint on a dropped axis is not expressible: single kernels, sums and WhiteNoise only.)"""
    d = x.shape[1]
    assert all(p[0] != "cp" for p in parts)
    drop = np.concatenate([sl[keep:] for sl in scale_slices(parts, d)])
    kept = np.setdiff1d(np.arange(theta.size), drop)
    return parts, x[:, :keep], theta[kept], kept
