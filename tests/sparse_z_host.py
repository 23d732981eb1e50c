"""
NumPy mirror of the gradient of the variational bound by the inducing inputs (gpmi_sgp_bound_zgrad), on top of
`sparse_host.SparseMirror.state` and the profiles of tests/matern_host.py (formulas, not the package's code).

    gamma = (K_mm + eps I + G)^-1 K_mn W r,  alpha = W (r - K_nm gamma),  T = L^-T (I - B^-1) L^-1
    M1 = gamma alpha^T + T K_mn W,  M2 = gamma gamma^T + L^-T (B - 2 I + B^-1) L^-1   (symmetric)
    s_ij = 1/2 sum_k D_k^2 / l_k^2,  g the profile of dK / d ln l_k = a^2 g(s) D_k^2 / l_k^2,  so dK / dD_k = -a^2 g D_k / l_k^2
    dF/dz_ik = -1 / l_k^2 [sum_j M1_ij a^2 g(s(z_i, x_j)) (z_ik - x_jk) - sum_j M2_ij a^2 g(s(z_i, z_j)) (z_ik - z_jk)]

z_i enters row i and column i of K_mm and M2 is symmetric: the second term has no 1/2.  eps = jitter a^2 does not depend
on Z.  Nothing is divided by a distance: coincident points contribute exact zeros.
"""
import numpy as np
from scipy.linalg import solve_triangular

import matern_host as mh
import sparse_host as sh


def weights(st):
    """(M1, M2) from a `SparseMirror.state`, as `SparseMirror.bound_and_gradient` forms them."""
    w, L, LB, Kmn, B = (st[k] for k in ("w", "L", "LB", "Kmn", "B"))
    m = len(L)
    Linv = solve_triangular(L, np.eye(m), lower=True)
    Binv = solve_triangular(LB, solve_triangular(LB, np.eye(m), lower=True), lower=True, trans="T")
    Binv = 0.5 * (Binv + Binv.T)
    gamma = Linv.T @ (Binv @ (Linv @ st["b"]))
    alpha = w * (st["r"] - Kmn.T @ gamma)
    beta = Linv.T @ (Linv @ (Kmn @ alpha))
    T = Linv.T @ (np.eye(m) - Binv) @ Linv
    M1 = np.outer(beta, alpha) + (T @ Kmn) * w
    M2 = np.outer(beta, beta) + Linv.T @ (B - 2.0 * np.eye(m) + Binv) @ Linv
    return M1, 0.5 * (M2 + M2.T)


def inducing_gradient(mirror, theta, white_var, r, noise_var, st=None, data_rows=None, z_rows=None):
    """dF/dZ, (m, d), of the mirror's bound at its Z (the mirror's ripple acts on K_mm and K_mn, as in its state).  st: the
    `state` of the same arguments, if the caller has it already.  data_rows / z_rows (boolean masks over x / Z): the result
    becomes (dF/dZ, the part of its K_mn term summed over those rows of x, the part of its K_mm term summed over those
    rows of Z) - what a device schedule that dropped those rows would lose."""
    st = st or mirror.state(theta, white_var, r, noise_var)
    M1, M2 = weights(st)
    a2, kappa, scales = mh.split(mirror.kind, theta)
    z, x = mirror.z, mirror.x
    g_mn = a2 * mh.profiles(mirror.kind, 0.5 * mh._u2(z, x, scales).sum(axis=0), kappa)[1]
    g_mm = a2 * mh.profiles(mirror.kind, 0.5 * mh._u2(z, z, scales).sum(axis=0), kappa)[1]
    W1, W2 = M1 * g_mn, M2 * g_mm
    out, part_mn, part_mm = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
    for k in range(z.shape[1]):
        d_mn = z[:, None, k] - x[None, :, k]
        d_mm = z[:, None, k] - z[None, :, k]
        out[:, k] = -((W1 * d_mn).sum(axis=1) - (W2 * d_mm).sum(axis=1)) / scales[k] ** 2
        if data_rows is not None:
            part_mn[:, k] = -(W1[:, data_rows] * d_mn[:, data_rows]).sum(axis=1) / scales[k] ** 2
        if z_rows is not None:
            part_mm[:, k] = (W2[:, z_rows] * d_mm[:, z_rows]).sum(axis=1) / scales[k] ** 2
    if data_rows is None and z_rows is None:
        return out
    return out, part_mn, part_mm


def all_quantities(case, mirror, ripple=None, data_rows=None, z_rows=None):
    """Every quantity the scale tests compare, from one `state` of the mirror (one ripple of K_mm and K_mn, one of K_mq):
    F (1,), the full gradient [mean, kernel parameters, (ln s)], dF/dZ, alpha, mean and variance at the case's query
    points and, with the masks of `inducing_gradient`, the two parts of dF/dZ."""
    mirror.ripple = ripple or (lambda name, A: A)
    nv = None if case["e"] is None else case["e"] ** 2
    r = case["y"] - sh.MU
    st = mirror.state(case["theta"], case["white"], r, nv)
    F, g, alpha = mirror.bound_and_gradient(case["theta"], case["white"], r, nv, st=st)
    gz = inducing_gradient(mirror, case["theta"], case["white"], r, nv, st=st, data_rows=data_rows, z_rows=z_rows)
    mean, var = mirror.predict(case["theta"], case["white"], r, nv, case["q"], st=st)
    out = dict(F=np.array([F]), grad=np.concatenate([[alpha.sum()], g if case["white"] > 0.0 else g[:-1]]), alpha=alpha,
               mean=mean + sh.MU, var=var)
    if data_rows is None and z_rows is None:
        out["gz"] = gz
    else:
        out["gz"], out["gz_data_part"], out["gz_kmm_part"] = gz
    return out


def allowances(base, moved_list, a2):
    """The project's rule: 10 x the largest movement of a quantity under the ripples, floored at 1e-10 of its scale (the
    largest magnitude; a^2 for the variance).  Returns (allowances, spreads)."""
    keys = ("F", "grad", "gz", "alpha", "mean", "var")
    spread = {k: max(float(np.abs(mv[k] - base[k]).max()) for mv in moved_list) for k in keys}
    scale = {k: float(np.abs(base[k]).max()) for k in keys}
    scale["var"] = float(a2)
    return {k: max(10.0 * spread[k], 1e-10 * scale[k]) for k in keys}, spread


def bound_of_z(kind, x, theta, white_var, r, noise_var, jitter=1e-8):
    """vec(Z) -> F, for finite differences by the inducing inputs."""
    d = np.asarray(x).shape[1]
    return lambda v: sh.SparseMirror(kind, x, np.asarray(v).reshape(-1, d), jitter=jitter).bound(theta, white_var, r, noise_var)
