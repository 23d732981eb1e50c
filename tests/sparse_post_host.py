"""
NumPy / SciPy mirror of the fitted sparse model's joint posterior and of its derivatives by the query point (gpmi_sgp_posterior,
gpmi_sgp_posterior_draws, gpmi_sgp_spatial_derivatives), on top of tests/sparse_host.py: everything comes from
`SparseMirror.state` by triangular solves, nothing from the package's code.

    V = [v(q_1) .. v(q_M)]^T, v = L^-1 k_m(q);   U likewise, u = L_B^-1 v
    mu = U c,   Sigma = K_qq - V V^T + U U^T
    gamma = L^-T L_B^-T c,   t(q) = L^-T (L_B^-T u(q) - v(q))
    d mean / d q_k = -(1 / l_k^2) sum_a gamma_a  a^2 g(s(q, z_a)) (q_k - z_ak)
    d var  / d q_k = -(2 / l_k^2) sum_a t_a(q)   a^2 g(s(q, z_a)) (q_k - z_ak)

The mirror's `ripple` hook is applied to K_mq ("mq"), as `SparseMirror.predict` does.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import matern_host as mh


def _vu(mir, st, theta, q):
    Kmq = mir.ripple("mq", mh.cross(mir.kind, mir.z, q, theta))
    v = solve_triangular(st["L"], Kmq, lower=True)
    u = solve_triangular(st["LB"], v, lower=True)
    return v, u


def posterior(mir, st, theta, q):
    """(mu (M,), Sigma (M, M)) of the latent function at the rows of q."""
    q = np.asarray(q, float)
    v, u = _vu(mir, st, theta, q)
    sigma = mh.cross(mir.kind, q, q, theta) - v.T @ v + u.T @ u
    return u.T @ st["c"], 0.5 * (sigma + sigma.T)


def derivatives(mir, st, theta, q):
    """(d mean / d q, d var / d q), (M, d) each."""
    q = np.asarray(q, float)
    a2, kappa, scales = mh.split(mir.kind, theta)
    v, u = _vu(mir, st, theta, q)
    gamma = solve_triangular(st["L"], solve_triangular(st["LB"], st["c"], lower=True, trans="T"), lower=True, trans="T")
    t = solve_triangular(st["L"], solve_triangular(st["LB"], u, lower=True, trans="T") - v, lower=True, trans="T")  # (m, M)
    s = 0.5 * mh._u2(mir.z, q, scales).sum(axis=0)
    pg = a2 * mh.profiles(mir.kind, s, kappa)[1]  # (m, M)
    dmean, dvar = np.zeros(q.shape), np.zeros(q.shape)
    for k in range(q.shape[1]):
        diff = q[None, :, k] - mir.z[:, None, k]  # (m, M)
        dmean[:, k] = -((gamma[:, None] * pg * diff).sum(axis=0)) / scales[k] ** 2
        dvar[:, k] = -2.0 * ((t * pg * diff).sum(axis=0)) / scales[k] ** 2
    return dmean, dvar


def draws(mu, sigma, z, jitter):
    """(mu + z chol(Sigma + eps I)^T, eps) with eps = jitter max diag Sigma."""
    eps = jitter * float(np.diag(sigma).max())
    L = cholesky(sigma + eps * np.eye(len(sigma)), lower=True)
    return mu + np.asarray(z, float) @ L.T, eps


def fd4_rows(f, q, h):
    """Fourth-order central differences of f: (M, d) points -> (M,) values, coordinate by coordinate: (M, d)."""
    q = np.asarray(q, float)
    out = np.zeros(q.shape)
    for k in range(q.shape[1]):
        e = np.zeros(q.shape[1])
        e[k] = h
        out[:, k] = (-f(q + 2 * e) + 8.0 * f(q + e) - 8.0 * f(q - e) + f(q - 2 * e)) / (12.0 * h)
    return out
