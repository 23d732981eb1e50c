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


def inducing_gradient(mirror, theta, white_var, r, noise_var):
    """dF/dZ, (m, d), of the mirror's bound at its Z (the mirror's ripple acts on K_mm and K_mn, as in its state)."""
    st = mirror.state(theta, white_var, r, noise_var)
    M1, M2 = weights(st)
    a2, kappa, scales = mh.split(mirror.kind, theta)
    z, x = mirror.z, mirror.x
    g_mn = a2 * mh.profiles(mirror.kind, 0.5 * mh._u2(z, x, scales).sum(axis=0), kappa)[1]
    g_mm = a2 * mh.profiles(mirror.kind, 0.5 * mh._u2(z, z, scales).sum(axis=0), kappa)[1]
    W1, W2 = M1 * g_mn, M2 * g_mm
    out = np.zeros_like(z)
    for k in range(z.shape[1]):
        d_mn = z[:, None, k] - x[None, :, k]
        d_mm = z[:, None, k] - z[None, :, k]
        out[:, k] = -((W1 * d_mn).sum(axis=1) - (W2 * d_mm).sum(axis=1)) / scales[k] ** 2
    return out


def bound_of_z(kind, x, theta, white_var, r, noise_var, jitter=1e-8):
    """vec(Z) -> F, for finite differences by the inducing inputs."""
    d = np.asarray(x).shape[1]
    return lambda v: sh.SparseMirror(kind, x, np.asarray(v).reshape(-1, d), jitter=jitter).bound(theta, white_var, r, noise_var)
