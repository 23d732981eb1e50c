"""
NumPy / SciPy mirror of `inference_amd.gp.MultiTargetGpRegressor` for the kernels the CPU oracle has (SE, RQ, optionally
+ WhiteNoise): T targets at the same inputs with shared covariance hyper-parameters and fixed offsets.  Test
infrastructure only; the covariance matrices and their derivatives are the oracle's own (oracle/gp_oracle.py), so the
mirror differs from T single-target `OracleGp`s in nothing but the order of the algebra.

    K = L L^T,  R = Y - 1 m^T,  V = L^-1 R,  A = K^-1 R
    lml_t = -1/2 |V[:, t]|^2 - sum ln L_ii,   LML = sum_t lml_t
    dLML/dtheta_j = 1/2 sum (A A^T - T K^-1) o dK_j
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gp_oracle as orc


def make_targets(x, y, T, seed=5):
    """The target recipe of the tests: column t is y (1 + 0.3 t) + 0.2 sin((t + 1) x_0) + 0.05 N(0, 1)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    return (y[:, None] * (1.0 + 0.3 * t)[None, :] + 0.2 * np.sin((t + 1)[None, :] * x[:, :1])
            + 0.05 * rng.standard_normal((x.shape[0], T)))


def cov_theta(kernel, y, d, white_noise=False, ln_sigma=np.log(0.1)):
    """workloads.timing_theta without the mean, + ln sigma_n with WhiteNoise."""
    import workloads as wl

    th = list(wl.timing_theta(kernel, y, d)[1:])
    return np.array(th + ([ln_sigma] if white_noise else []))


class MultiTargetMirror:
    def __init__(self, x, Y, y_err=None, kernel=orc.SE, white_noise=False, target_means=None, hyperpars=None):
        self.x = np.asarray(x, float).reshape(len(x), -1)
        self.Y = np.asarray(Y, float).reshape(len(x), -1)
        self.n, self.T = self.Y.shape
        self.m = self.Y.mean(axis=0) if target_means is None else np.broadcast_to(np.asarray(target_means, float), (self.T,))
        self.R = self.Y - self.m[None, :]
        # the oracle builds K(theta) + white noise + diag(y_err^2): a one-target model on zeros lends its builders
        with np.errstate(divide="ignore"):  # (its hyper-parameter bounds take the logarithm of the zeros' spread)
            self._k = orc.OracleGp(self.x, np.zeros(self.n), y_err, kernel=kernel, white_noise=white_noise)
        self.kernel = kernel
        if hyperpars is not None:
            self.set_hyperparameters(hyperpars)

    def set_hyperparameters(self, theta):
        self.hyperpars = np.asarray(theta, float)
        self.L = cholesky(self._k._K(self.hyperpars), lower=True)
        self.alpha = solve_triangular(self.L.T, solve_triangular(self.L, self.R, lower=True), lower=False)

    def marginal_likelihood(self, theta, per_target=False):
        L = cholesky(self._k._K(np.asarray(theta, float)), lower=True)
        V = solve_triangular(L, self.R, lower=True)
        lml_t = -0.5 * (V * V).sum(axis=0) - np.log(np.diagonal(L)).sum()
        return lml_t if per_target else float(lml_t.sum())

    def marginal_likelihood_gradient(self, theta):
        K, grads = self._k._K_and_grads(np.asarray(theta, float))
        L = cholesky(K, lower=True)
        Li = solve_triangular(L, np.eye(self.n), lower=True)
        iK = Li.T @ Li
        A = iK @ self.R
        V = solve_triangular(L, self.R, lower=True)
        lml = -0.5 * (V * V).sum() - self.T * np.log(np.diagonal(L)).sum()
        Q = A @ A.T - self.T * iK
        return float(lml), np.array([0.5 * (Q * dK.T).sum() for dK in grads])

    def __call__(self, points):
        p = self._k._points(points)
        th = self._k._split(self.hyperpars)[0]
        Kq = orc.kernel_cross(self.kernel, p, self.x, th)
        v = solve_triangular(self.L, Kq.T, lower=True)
        var = np.exp(self.hyperpars[0]) ** 2 - (v * v).sum(axis=0)
        return Kq @ self.alpha + self.m[None, :], np.sqrt(np.abs(var))

    def _ikdiag(self, L):
        Li = solve_triangular(L, np.eye(self.n), lower=True)
        return (Li * Li).sum(axis=0)

    def loo_predictions(self):
        var = 1.0 / self._ikdiag(self.L)
        return self.Y - self.alpha * var[:, None], np.sqrt(var)

    def loo_likelihood(self, theta):
        L = cholesky(self._k._K(np.asarray(theta, float)), lower=True)
        A = solve_triangular(L.T, solve_triangular(L, self.R, lower=True), lower=False)
        var = 1.0 / self._ikdiag(L)
        return float(-0.5 * (var * (A * A).sum(axis=1) + self.T * np.log(var)).sum())


def _one_blas_thread():
    """N of a few hundred: a BLAS thread team per call only gets in the way of the threads over the columns."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib

        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


class OracleColumns:
    """The yardstick: one `OracleGp` per target column at theta_t = [m_t, theta_cov]; sums and stacks of their answers.
    Every column repeats the O(N^3) work the targets share - that is what is being checked against - so the columns are
    spread over a few threads (NumPy's linear algebra releases the interpreter lock); results keep the column order."""

    def __init__(self, x, Y, y_err, kernel, white_noise, means, theta_cov):
        self.means = np.asarray(means, float)
        self.theta_cov = np.asarray(theta_cov, float)
        self.T = Y.shape[1]
        self.gps = self._columns(lambda t: orc.OracleGp(x, Y[:, t], y_err, kernel=kernel, white_noise=white_noise,
                                                        hyperpars=self.theta(t, self.theta_cov)))

    def _columns(self, f):
        if self.T == 1:
            return [f(0)]
        with _one_blas_thread(), ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            return list(pool.map(f, range(self.T)))

    def theta(self, t, theta_cov):
        return np.concatenate([[self.means[t]], np.asarray(theta_cov, float)])

    def lml_t(self, theta_cov):
        return np.array(self._columns(lambda t: self.gps[t].marginal_likelihood(self.theta(t, theta_cov))))

    def lml_gradient(self, theta_cov):
        res = self._columns(lambda t: self.gps[t].marginal_likelihood_gradient(self.theta(t, theta_cov)))
        return sum(r[0] for r in res), np.sum([r[1][1:] for r in res], axis=0)

    def alpha(self):
        return np.stack([g.alpha for g in self.gps], axis=1)

    def predict(self, pts):
        res = self._columns(lambda t: self.gps[t](pts))
        return np.stack([r[0] for r in res], axis=1), res[0][1]

    def loo_predictions(self):
        res = self._columns(lambda t: self.gps[t].loo_predictions())
        return np.stack([r[0] for r in res], axis=1), res[0][1]

    def loo_likelihood(self, theta_cov):
        return sum(self._columns(lambda t: self.gps[t].loo_likelihood(self.theta(t, theta_cov))))
