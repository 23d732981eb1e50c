"""
`MultiTargetGpRegressor` (extension: the reference has no counterpart) - Gaussian-process regression of T targets
observed at the same inputs with the same data errors and SHARED covariance hyper-parameters.

With Y (N, T), fixed offsets m (T,), R = Y - 1 m^T and the covariance K(theta) of a `GpRegressor` with the same kernel
and `y_err`, K = L L^T, V = L^-1 R, A = K^-1 R:

    lml_t      = -1/2 |V[:, t]|^2 - sum_i ln L_ii          (no 2 pi term, as GpRegressor.marginal_likelihood)
    LML        = sum_t lml_t
    dLML/dth_j = 1/2 sum_ab (A A^T - T K^-1)_ab (dK/dth_j)_ab
    mean(q)[t] = k(q)^T A[:, t] + m_t,   var(q) = a^2 - |L^-1 k(q)|^2      (one variance for all targets)
    leave-one-out: var_i = 1 / (K^-1)_ii,  mu_loo[i, t] = Y[i, t] - A[i, t] var_i

The covariance matrix, its factor, K^-1 and the predictive variance do not depend on the targets: they are computed
once per call on the device (gpmi_mt_*, csrc/api_multi.hip); per target there are only the two O(N^2) solves.  Column t
of `alpha` is the `alpha` of the single-target `GpRegressor` of column t with `ConstantMean` fixed at m_t.
"""
from copy import copy
from inspect import isclass
from warnings import warn

import numpy as np
from numpy import array, ndarray, sqrt, zeros
from numpy.linalg import LinAlgError
from numpy.random import random
from scipy.optimize import fmin_l_bfgs_b

from inference_amd import _lib
from inference_amd._engine import GpEngine
from inference_amd.gp import _messages as msg
from inference_amd.gp.covariance import (CovarianceFunction, SquaredExponential, device_plan, heteroscedastic_slice,
                                         periodic_dims_of, sum_kernels)


class MultiTargetGpRegressor:
    """
    :param x: (N, d) array of point coordinates; 1-D input means d = 1 (coerced as `GpRegressor` does).
    :param Y: (N, T) array of values, one column per target; a 1-D array is one target.
    :param y_err: (N,) standard deviations shared by all targets, or None.  An (N, T) array is refused: errors of \
        their own give every target its own covariance matrix, which is what this class exists to avoid.
    :param hyperpars: the covariance hyper-parameters (layout, labels and bounds are the kernel's own); when omitted \
        they are found by a multi-start L-BFGS-B maximisation of the summed marginal likelihood.
    :param kernel: one stationary device kernel (`SquaredExponential`, `RationalQuadratic`, `Matern32`, `Matern52`) \
        or a sum of 2 to 4 of them, optionally `+ WhiteNoise()`.
    :param target_means: the fixed offsets m: None (the column means of Y), a scalar, or a (T,) array.  They are \
        numbers, not hyper-parameters.
    :param int n_starts: number of L-BFGS-B starting positions.
    :param device: HIP device index; default ``LOCAL_RANK`` / 0.
    """

    def __init__(self, x: ndarray, Y: ndarray, y_err: ndarray = None, hyperpars: ndarray = None,
                 kernel: CovarianceFunction = SquaredExponential, target_means=None, n_starts: int = None,
                 device: int = None):
        self.x, self.Y = self._coerce_training_data(x, Y)
        self.n_points, self.n_targets = self.Y.shape
        self.n_dimensions = self.x.shape[1]
        if self.n_dimensions > msg.MAX_DIMENSIONS:
            raise ValueError(msg.too_many_dimensions("MultiTargetGpRegressor", self.n_dimensions))
        if self.n_targets > _lib.MT_MAX_T:
            raise ValueError(f"[ MultiTargetGpRegressor error ] Y has {self.n_targets} targets, but the device entry "
                             f"points take at most {_lib.MT_MAX_T} (GPMI_MT_MAX_T).")
        self._noise_var = self._check_error_data(y_err)
        self.target_means = self._check_target_means(target_means)
        self._R = np.ascontiguousarray(self.Y - self.target_means[None, :])

        self.cov = kernel() if isclass(kernel) else kernel
        self.cov.pass_spatial_data(self.x)
        if periodic_dims_of(self.cov) is not None:
            raise NotImplementedError("[ MultiTargetGpRegressor error ] The Periodic covariance function is not served "
                                      "by the many-target entry points of the device: fit one GpRegressor per target.")
        plan = device_plan(self.cov)
        if plan is None or plan[0] == -1 or heteroscedastic_slice(self.cov) is not None:
            raise NotImplementedError(
                f"[ MultiTargetGpRegressor error ] The covariance function {type(self.cov).__name__} is not served: "
                "one stationary device kernel or a sum of 2 to 4 of them, optionally + WhiteNoise (no ChangePoint, "
                "no HeteroscedasticNoise, no plugin kernels).")
        self._kernel_id, self._stat, self._stat_slice, self._wn_index = plan
        self._sum_kernels = sum_kernels(self._stat) if self._kernel_id == _lib.KERNEL_SUM else None
        if self.cov.bounds is None:
            self.cov.estimate_hyperpar_bounds(self._R.ravel())
        self.hp_bounds = copy(self.cov.bounds)
        self.n_hyperpars = len(self.hp_bounds)
        self.hyperpar_labels = [*self.cov.hyperpar_labels]
        self._device = device
        self._engine = None
        self._alpha = None

        if hyperpars is None:
            hyperpars = self.multistart_bfgs(starts=n_starts)
        self.set_hyperparameters(hyperpars)

    # ---------------------------------------------------------------------------------
    # argument checks (no device call)
    # ---------------------------------------------------------------------------------
    @staticmethod
    def _coerce_training_data(x, Y):
        xa = np.asarray(x)
        Ya = np.asarray(Y, dtype=float)
        if Ya.ndim == 1:
            Ya = Ya.reshape([Ya.size, 1])
        if Ya.ndim != 2 or Ya.shape[1] < 1:
            raise ValueError(f"[ MultiTargetGpRegressor error ] 'Y' must be an (N, T) array with T >= 1 (or 1-D for one "
                             f"target), but has shape {Ya.shape}.")
        if xa.ndim > 2:
            raise ValueError(msg.x_not_2d(xa.ndim, xa.shape))
        if xa.ndim < 2:
            xa = xa.reshape([xa.size, 1])
        if xa.shape[0] != Ya.shape[0]:
            raise ValueError(f"[ MultiTargetGpRegressor error ] The first dimensions of 'x' and 'Y' must agree: 'x' has "
                             f"shape {xa.shape}, 'Y' has shape {Ya.shape}.")
        return np.ascontiguousarray(xa, dtype=float), np.ascontiguousarray(Ya)

    def _check_error_data(self, y_err):
        if y_err is None:
            return None
        e = np.asarray(y_err, dtype=float)
        if e.ndim == 2 and e.shape == (self.n_points, self.n_targets) and self.n_targets > 1:
            raise NotImplementedError(
                "[ MultiTargetGpRegressor error ] An (N, T) 'y_err' is not served: per-target errors give every target "
                "its own covariance matrix, and with it its own factorisation - build one GpRegressor per target.")
        e = e.squeeze() if e.ndim > 1 else e
        if e.shape != (self.n_points,):
            raise ValueError(msg.Y_ERR_SHAPE)
        return e**2

    def _check_target_means(self, target_means):
        if target_means is None:
            return self.Y.mean(axis=0)
        m = np.asarray(target_means, dtype=float)
        if m.ndim == 0:
            return np.full(self.n_targets, float(m))
        if m.shape != (self.n_targets,):
            raise ValueError(f"[ MultiTargetGpRegressor error ] 'target_means' must be None, a scalar or an array of "
                             f"shape ({self.n_targets},), but has shape {m.shape}.")
        return m.copy()

    # ---------------------------------------------------------------------------------
    # device plumbing
    # ---------------------------------------------------------------------------------
    @property
    def engine(self) -> GpEngine:
        if self._engine is None:
            eng = GpEngine(self.x, zeros(self.n_points), noise_var=self._noise_var, device=self._device)
            if self._sum_kernels is not None:
                eng.set_sum(self._sum_kernels)
            eng.mt_set_targets(self._R)
            self._engine = eng
        return self._engine

    def __getstate__(self):
        state = self.__dict__.copy()  # device handles do not pickle: re-attached lazily (the fit is not: set_hyperparameters)
        state["_engine"] = None
        return state

    def _split(self, theta):
        theta = np.asarray(theta, dtype=float)
        if theta.shape != (self.n_hyperpars,):
            raise ValueError(msg.wrong_hyperpar_count(self.n_hyperpars, theta.size))
        extra = float(np.exp(2 * theta[self._wn_index])) if self._wn_index is not None else 0.0
        return np.ascontiguousarray(theta[self._stat_slice]), extra

    # ---------------------------------------------------------------------------------
    # public API
    # ---------------------------------------------------------------------------------
    def set_hyperparameters(self, hyperpars: ndarray):
        """Update the hyper-parameters and re-fit: one factorisation, T pairs of solves."""
        theta_stat, extra = self._split(hyperpars)
        self.hyperpars = np.asarray(hyperpars, dtype=float).copy()
        self._alpha = None
        lml, lml_t, info = self.engine.mt_fit(self._kernel_id, theta_stat, extra)
        if info != 0:
            raise LinAlgError("Matrix is not positive definite")
        self._lml, self._lml_t = lml, lml_t

    @property
    def alpha(self) -> ndarray:
        """A = K^-1 R, (N, T); downloaded on first use."""
        if self._alpha is None:
            self._alpha = self.engine.mt_alpha()
        return self._alpha

    def process_points(self, points: ndarray) -> ndarray:
        q = np.asarray(points, dtype=float)
        d = self.n_dimensions
        if q.ndim > 2:
            raise ValueError(msg.points_not_2d(q.ndim, q.shape))
        if q.ndim <= 1:
            if d == 1:
                q = q.reshape([q.size, 1])
            elif q.ndim == 1 and q.size == d:
                q = q.reshape([1, d])
        if q.ndim != 2 or q.shape[1] != d:
            raise ValueError(msg.points_wrong_width(d, q.shape))
        return q

    def __call__(self, points: ndarray):
        """Means (M, T) and the standard deviation (M,) all targets share, sqrt(abs(var)) as `GpRegressor`."""
        p = self.process_points(points)
        mean, var = self.engine.mt_predict(p)
        return mean + self.target_means[None, :], sqrt(abs(var))

    def marginal_likelihood(self, theta: ndarray, per_target: bool = False):
        """Sum over the targets of the log-marginal likelihood (no 2 pi term); `per_target`: the (T,) terms.  -1e50
        where K does not factorise."""
        theta_stat, extra = self._split(theta)
        lml, lml_t, info = self.engine.mt_lml(self._kernel_id, theta_stat, extra, per_target=per_target)
        if info != 0:
            warn("Cholesky decomposition failure in marginal_likelihood")
            return np.full(self.n_targets, -1e50) if per_target else -1e50
        return lml_t if per_target else float(lml)

    def marginal_likelihood_batch(self, thetas: ndarray) -> ndarray:
        """`marginal_likelihood` for B hyper-parameter vectors, one after another (what the samplers and lockstep
        drivers of `inference_amd.mcmc` call); -1e50 rows for failures."""
        thetas = np.asarray(thetas, dtype=float)
        if thetas.size == 0:
            return np.empty(0)
        out = np.empty(len(np.atleast_2d(thetas)))
        failed = False
        for b, t in enumerate(np.atleast_2d(thetas)):
            theta_stat, extra = self._split(t)
            lml, _, info = self.engine.mt_lml(self._kernel_id, theta_stat, extra)
            failed |= info != 0
            out[b] = lml if info == 0 else -1e50
        if failed:
            warn("Cholesky decomposition failure in marginal_likelihood")
        return out

    def marginal_likelihood_gradient(self, theta: ndarray):
        """(LML, gradient): K^-1 is formed once and contracted once, whatever T."""
        theta_stat, extra = self._split(theta)
        lml, g_stat, trace_q, info = self.engine.mt_lml_grad(self._kernel_id, theta_stat, extra)
        if info != 0:
            raise LinAlgError("Matrix is not positive definite")
        grad = zeros(self.n_hyperpars)
        grad[self._stat_slice] = g_stat
        if self._wn_index is not None:
            grad[self._wn_index] = extra * trace_q  # 1/2 sum Q o (2 sigma^2 I) with Q = A A^T - T K^-1
        return float(lml), grad

    def loo_predictions(self):
        """Leave-one-out predictions (N, T) and their standard deviation (N,), R&W eq. 5.12 for every target."""
        resid, ikdiag = self.engine.mt_loo()
        return self.Y - resid, sqrt(1.0 / ikdiag)

    def loo_likelihood(self, theta: ndarray) -> float:
        """Leave-one-out log-likelihood summed over the targets: -1/2 sum_i (var_i sum_t A_it^2 + T ln var_i)."""
        theta_stat, extra = self._split(theta)
        a2, ikdiag, info = self.engine.mt_loo_terms(self._kernel_id, theta_stat, extra)
        if info != 0:
            warn("Cholesky decomposition failure in loo_likelihood")
            return -1e50
        var = 1.0 / ikdiag
        return float(-0.5 * (var * a2 + self.n_targets * np.log(var)).sum())

    # ---------------------------------------------------------------------------------
    # hyper-parameter search
    # ---------------------------------------------------------------------------------
    def bfgs_cost_func(self, theta: ndarray):
        y, grad_y = self.marginal_likelihood_gradient(theta)
        return -y, -grad_y

    def multistart_bfgs(self, starts: int = None):
        """Multi-start L-BFGS-B on the device gradient, the starts drawn as `GpRegressor.multistart_bfgs` draws them
        and run one after another.  `search_log`: dict(starts, start_values, values)."""
        if starts is None:
            starts = int(2 * sqrt(len(self.hp_bounds))) + 1
        lwr, upr = [array([k[i] for k in self.hp_bounds]) for i in [0, 1]]
        starting_positions = [lwr + (upr - lwr) * random(size=len(self.hp_bounds)) for _ in range(starts - 1)]
        starting_positions.append(0.5 * (lwr + upr))
        start_values = self.marginal_likelihood_batch(array(starting_positions))
        results = [fmin_l_bfgs_b(func=self.bfgs_cost_func, x0=x0, approx_grad=False, bounds=self.hp_bounds)
                   for x0 in starting_positions]
        self.search_log = dict(starts=array(starting_positions), start_values=start_values,
                               values=array([-float(r[1]) for r in results]))
        return sorted(results, key=lambda r: r[1])[0][0]

    def __str__(self):
        pad = max(len(label) for label in self.hyperpar_labels) + 2
        lines = [f"\n[ MultiTargetGpRegressor hyperparameters: {self.n_targets} targets ]\n"]
        for label, val in zip(self.hyperpar_labels, self.hyperpars):
            lines.append(f"{label:>{pad}} = {val:.4}\n")
        return "".join(lines)
