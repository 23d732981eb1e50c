"""
NumPy mirror of the Periodic device kernel (the reference has none, so there are no golden values to compare with).
Everything here is written from the formulas, not from the package's code:

    K(u, v) = a^2 exp(-s),   s = sum_k w_k / l_k^2,   D = u - v
    w_k = 1/2 D_k^2                    k not periodic
    w_k = 2 sin^2(pi D_k / p_k)        k periodic
    theta = [ln a, ln l_1 .. ln l_d, ln p_j for j in periodic_dims, ascending]
    dK/d ln a = 2 K,   dK/d ln l_k = 2 K w_k / l_k^2,   dK/d ln p_k = K 2 pi u_k sin(2 pi u_k) / l_k^2,  u_k = D_k / p_k
    dK(q, x)/dq_k = K delta_k / l_k^2,  delta_k = (x - q)_k  or  (2 pi / p_k) sin(2 pi (x - q)_k / p_k)
    prior variance of the derivative along axis k: a^2 / l_k^2  or  a^2 (2 pi / p_k)^2 / l_k^2
    diagonal of a build: a^2 (1 + 1e-12)

`cross(..., dtype=np.longdouble)` evaluates K from the float64 inputs in extended precision (80-bit on x86): the
yardstick of the element-wise error bound.  `HostKernel` is a plugin `CovarianceFunction` on these formulas:
`GpRegressor(kernel=HostKernel(dims))` takes the package's generic route (host-built matrices, the device's dense entry
points) - an independent way to every quantity the device path computes.
"""
import numpy as np

from inference_amd.gp.covariance import CovarianceFunction

JITTER = 1e-12


def split(theta, d, dims, dtype=float):
    """(a^2, l (d,), p (d,), 1 where not periodic)"""
    theta = np.asarray(theta, dtype=float).astype(dtype)
    assert theta.size == 1 + d + len(dims), (theta.size, d, dims)
    p = np.ones(d, dtype=dtype)
    p[list(dims)] = np.exp(theta[1 + d:])
    return np.exp(2 * theta[0]), np.exp(theta[1:1 + d]), p


def warped(u, v, theta, dims, dtype=float):
    """(w (d, n_u, n_v), D / p (d, n_u, n_v), l, p, a^2)"""
    u, v = np.asarray(u, dtype=float).astype(dtype), np.asarray(v, dtype=float).astype(dtype)
    d = u.shape[1]
    a2, l, p = split(theta, d, dims, dtype)
    pi = np.arccos(dtype(-1))
    w, uk = [], []
    for k in range(d):
        D = u[:, None, k] - v[None, :, k]
        uk.append(D / p[k])
        w.append(2 * np.sin(pi * uk[-1]) ** 2 if k in dims else D * D / 2)
    return np.array(w), np.array(uk), l, p, a2


def cross(u, v, theta, dims, dtype=float):
    w, _, l, _, a2 = warped(u, v, theta, dims, dtype)
    return a2 * np.exp(-(w / (l * l)[:, None, None]).sum(axis=0))


def build(x, theta, dims):
    K = cross(x, x, theta, dims)
    K[np.diag_indices_from(K)] += split(theta, x.shape[1], dims)[0] * JITTER
    return K


def build_and_grads(x, theta, dims):
    w, uk, l, p, a2 = warped(x, x, theta, dims)
    K0 = a2 * np.exp(-(w / (l * l)[:, None, None]).sum(axis=0))
    K = K0 + a2 * JITTER * np.eye(len(x))
    grads = [2.0 * K]
    grads.extend(2.0 * K0 * w[k] / l[k] ** 2 for k in range(x.shape[1]))
    grads.extend(K0 * 2.0 * np.pi * uk[k] * np.sin(2.0 * np.pi * uk[k]) / l[k] ** 2 for k in dims)
    return K, grads


def element_bound(u, v, theta, dims):
    """The bound on |K_device - K_true| per element, from the roundings of the device algorithm:
    a^2 e^-s [(d + 4) s + 4 + sum_periodic (2 / l_k^2)(3 pi |u_k| + 8) + sum_plain 4 w_k / l_k^2] 2^-53"""
    w, uk, l, _, a2 = warped(u, v, theta, dims, np.longdouble)
    d = len(l)
    s = (w / (l * l)[:, None, None]).sum(axis=0)
    extra = np.zeros_like(s)
    for k in range(d):
        if k in dims:
            extra += (2 / l[k] ** 2) * (3 * np.pi * np.abs(uk[k]) + 8)
        else:
            extra += 4 * w[k] / l[k] ** 2
    return a2 * np.exp(-s) * ((d + 4) * s + 4 + extra) * np.longdouble(2.0) ** -53


def delta(q, x, theta, dims):
    """(delta (N, d), l, p, a^2) for one query point q"""
    d = x.shape[1]
    a2, l, p = split(theta, d, dims)
    D = np.array(x - q[None, :], dtype=float)
    for k in dims:
        D[:, k] = (2.0 * np.pi / p[k]) * np.sin(2.0 * np.pi * D[:, k] / p[k])
    return D, l, p, a2


def gradient_terms(q, x, theta, dims):
    """(A (d, N), R (d,)): A_kn K(q, x_n) = dK(q, x_n)/dq_k, R_k the prior variance of the derivative along axis k."""
    D, l, p, a2 = delta(q, x, theta, dims)
    R = a2 / l**2
    for k in dims:
        R[k] *= (2.0 * np.pi / p[k]) ** 2
    return (D / l**2).T, R


class HostKernel(CovarianceFunction):
    """The Periodic kernel as a plugin: every matrix in NumPy on the host."""

    def __init__(self, dims=None):
        self.dims = dims
        self.bounds = None

    def pass_spatial_data(self, x):
        self.x = np.asarray(x, dtype=float)
        if self.dims is None:
            self.dims = list(range(self.x.shape[1]))
        self.n_params = 1 + self.x.shape[1] + len(self.dims)
        self.hyperpar_labels = [f"host periodic {i}" for i in range(self.n_params)]

    def estimate_hyperpar_bounds(self, y):
        self.bounds = [(-5.0, 5.0)] * self.n_params

    def __call__(self, u, v, theta):
        return cross(np.asarray(u, float), np.asarray(v, float), theta, self.dims)

    def build_covariance(self, theta):
        return build(self.x, theta, self.dims)

    def covariance_and_gradients(self, theta):
        return build_and_grads(self.x, theta, self.dims)

    def gradient_terms(self, v, x, theta):
        return gradient_terms(np.asarray(v, float), x, theta, self.dims)


SPAN = 5.0  # the coordinates: at most 8 periods of the shortest period of `theta_for` (0.7)


def dataset(n, d, seed=0):
    """x uniform in [0, 5]^d with row 1 a copy of row 0; y periodic in every coordinate plus noise; y_err = 0.1."""
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    x = rng.uniform(0.0, SPAN, size=(n, d))
    x[1] = x[0]
    y = np.sin(2.0 * np.pi * x[:, 0] / 1.7) + 0.3 * np.cos(1.3 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y, np.full(n, 0.1)


def theta_for(d, dims, seed=0):
    """[ln a, ln l_k, ln p_j]: a = e^0.2, l in [0.5, 2], p in [0.7, 3]."""
    rng = np.random.default_rng(31 + seed + d + 7 * len(dims))
    return np.array([0.2] + list(np.log(rng.uniform(0.5, 2.0, size=d))) + list(np.log(rng.uniform(0.7, 3.0, size=len(dims)))))
