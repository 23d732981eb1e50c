"""
`SparseGpRegressor` - Gaussian-process regression for data sets too large for the exact `GpRegressor`: the variational
inducing-point approximation of Titsias (2009).  m << N inducing inputs Z summarise the N data points; an evaluation
costs O(N m^2) time and O(N d + m^2) memory, and the objective of the hyper-parameter search is a lower bound F of the
log marginal likelihood (with its 2 pi constant), equal to it for Z = x.  All of it runs on the device (include/gpmi.h:
gpmi_sgp_*): x never comes back, K_mn is never held whole.  The class follows `GpRegressor`: theta = [mean parameters |
covariance parameters], `marginal_likelihood`, `marginal_likelihood_gradient`, `set_hyperparameters`, `__call__`.

The inducing inputs are variational parameters: `marginal_likelihood_gradient(theta, inducing_points=True)` adds dF/dZ
(gpmi_sgp_bound_zgrad: a contraction behind the theta-gradient's, on the same panels), `set_inducing_points` moves Z
without rebuilding the object, and `optimise_inducing_points` (or the constructor's `optimise_inducing=True`) runs one
L-BFGS-B over vec(Z), or over [theta | vec(Z)] jointly, every coordinate of Z inside the bounding box of x.
Where Z starts: a random subset of x, or (`inducing_method="greedy"`, `select_inducing_points`,
`reselect_inducing_points`) the rows greedy conditional-variance selection picks on the device (gpmi_select_points).

Supported: one of SquaredExponential, RationalQuadratic, Matern32, Matern52 (class or instance), optionally
`+ WhiteNoise()`; the mean functions of `inference_amd.gp.mean` (evaluated on the host); data errors `y_err`.
The fitted model answers what `GpRegressor` answers, at O(M m^2) per call whatever N is: `build_posterior` (mean and
joint covariance), `sample_posterior` (joint draws; the covariance and the normals stay on the device),
`spatial_derivatives` / `spatial_derivatives_batch` (gradients of the predictive mean and variance, all four kernels) -
and through them the acquisition functions of `inference_amd.gp.acquisition` (`update_gp(sparse_model)`).
Batches of hyper-parameter vectors (`marginal_likelihood_batch`, `marginal_likelihood_gradient_batch`: one device call,
gpmi_sgp_bound_batch, every launch carrying all of them) make the lockstep drivers of `inference_amd.mcmc` and the lockstep
multi-start search (`multistart_bfgs(lockstep=True)`) run on a sparse model as they run on `GpRegressor`.
Not supported: FITC, `gradient` (the covariance of the gradient), `GpOptimiser`, several GPUs, dF/dZ in batches.
"""
import ctypes as C
from copy import copy, deepcopy
from inspect import isclass
from warnings import warn

import numpy as np
from numpy.linalg import LinAlgError
from numpy.random import random
from scipy.optimize import differential_evolution, fmin_l_bfgs_b

from inference_amd import _lib
from inference_amd._engine import SparseEngine
from inference_amd.gp import _messages as msg
from inference_amd.gp._draws import draw_arguments, raise_if_not_positive_definite
from inference_amd.gp.covariance import (CompositeCovariance, Periodic, SquaredExponential, WhiteNoise,
                                         _StationaryDeviceKernel, device_plan)
from inference_amd.gp.mean import ConstantMean
from inference_amd.gp.regression import GpRegressor

SUPPORTED = ("one of SquaredExponential, RationalQuadratic, Matern32, Matern52 (class or instance), optionally "
             "+ WhiteNoise(), with y_err data errors")
INDUCING_METHODS = ("random", "greedy")


def _has_periodic(cov):
    return any(isinstance(c, Periodic) for c in (cov.components if isinstance(cov, CompositeCovariance) else [cov]))


def _select_on_device(x, m, kernel_id, theta_stat, weights, tol, min_variance, device):
    """gpmi_select_points on a handle of its own: (indices (count,), trace (count + 1,), pivot variances (count,))."""
    x = _lib.as_f64(x)
    theta_stat = _lib.as_f64(theta_stat)
    weights = None if weights is None else _lib.as_f64(weights)
    if weights is not None and weights.shape != (x.shape[0],):
        raise ValueError(f"weights must have shape ({x.shape[0]},), got {weights.shape}")
    index, trace, pivot_var = np.zeros(m, dtype=np.int64), np.zeros(m + 1), np.zeros(m)
    count = C.c_int64(0)
    h = _lib.Handle(device)
    try:
        h.call("gpmi_select_points", x.shape[0], x.shape[1], _lib.dptr(x), _lib.dptr(weights), int(kernel_id),
               _lib.dptr(theta_stat), theta_stat.size, int(m), float(min_variance), float(tol),
               index.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(trace), _lib.dptr(pivot_var), C.byref(count))
    finally:
        h.close()
    k = count.value
    return index[:k].copy(), trace[:k + 1].copy(), pivot_var[:k].copy()


def select_inducing_points(x, m, kernel, theta_cov, *, weights=None, tol=0.0, min_variance=1e-8, candidates=None, seed=None,
                           device=None):
    """
    Greedy conditional-variance selection of m rows of x as inducing inputs, on the device (include/gpmi.h:
    gpmi_select_points): the pivoted partial Cholesky factorisation of K_nn.  Each step takes the point whose prior
    variance is least explained by the points already chosen (times its weight), so the first k indices are the selection
    of size k, and the quantity driven down, sum_i w_i (a^2 - Q_ii), is the trace term of the bound.

    :param x: (N, d) points (1-D input means d = 1).
    :param m: the most points to select, 1 <= m <= min(N, 4096).
    :param kernel: a stationary device kernel (class or instance), optionally ``+ WhiteNoise()``, whose part is ignored.
    :param theta_cov: the kernel's parameters in its own layout.
    :param weights: (N,) weights w_i >= 0, e.g. 1 / sigma_i^2; None: all 1.  Rows of weight 0 are never selected.
    :param tol: stop once the trace has fallen to `tol` times its start.
    :param min_variance: points whose conditional variance (in units of a^2) is not above it are not selected.
    :param candidates: k: select among k rows drawn by ``default_rng(seed).choice(N, k, replace=False)``, sorted, which
        bounds the device memory at k m 8 bytes.  The indices returned refer to x.
    :return: (indices (count,), trace (count + 1,), pivot_variances (count,)) with count <= m: the rows in the order
        chosen, tr_0 .. tr_count in units of a^2, and the conditional variance of each row when it was chosen.
    """
    x = np.asarray(x, dtype=float)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.ndim != 2 or x.shape[1] > msg.MAX_DIMENSIONS:
        raise ValueError(f"x must be an (N, d) array with d <= {msg.MAX_DIMENSIONS}, got shape {x.shape}")
    cov = deepcopy(kernel() if isclass(kernel) else kernel)
    if _has_periodic(cov):
        raise NotImplementedError("select_inducing_points: the Periodic covariance function is not served by the "
                                  f"selection kernels of the device; supported: {SUPPORTED}")
    cov.pass_spatial_data(x)
    plan = device_plan(cov)
    if plan is None or not isinstance(plan[1], _StationaryDeviceKernel):
        raise NotImplementedError(f"select_inducing_points: unsupported covariance {type(cov).__name__}; supported: {SUPPORTED}")
    kernel_id, _, stat_slice, _ = plan
    theta_cov = np.asarray(theta_cov, dtype=float)
    if theta_cov.shape != (cov.n_params,):
        raise ValueError(f"theta_cov must have {cov.n_params} entries, got shape {theta_cov.shape}")
    rows = None
    if candidates is not None:
        k = int(candidates)
        if not 1 <= k <= x.shape[0]:
            raise ValueError(f"candidates = {k}: must lie in 1 .. N = {x.shape[0]}")
        rows = np.sort(np.random.default_rng(seed).choice(x.shape[0], k, replace=False))
    n = x.shape[0] if rows is None else len(rows)
    m = int(m)
    if not 1 <= m <= min(n, _lib.SGP_MAX_M):
        raise ValueError(f"m = {m}: must lie in 1 .. min(number of candidate rows, {_lib.SGP_MAX_M})")
    if weights is not None:
        weights = np.asarray(weights, dtype=float)
        if weights.shape != (x.shape[0],):
            raise ValueError(f"weights must have shape ({x.shape[0]},), got {weights.shape}")
    index, trace, pivot_var = _select_on_device(x if rows is None else x[rows], m, kernel_id, theta_cov[stat_slice],
                                                weights if weights is None or rows is None else weights[rows], tol,
                                                min_variance, device)
    return (index if rows is None else rows[index]), trace, pivot_var


class SparseGpRegressor:
    """
    :param x: (N, d) coordinates (1-D input means d = 1), d <= 64.
    :param y: (N,) values.
    :param y_err: (N,) standard deviations of the values, or None (then the kernel needs `+ WhiteNoise()`).
    :param inducing_points: (m, d) array of inducing inputs, or an int m: m rows of x drawn by
        ``numpy.random.default_rng(seed).choice(N, m, replace=False)``, sorted.  1 <= m <= 4096.
    :param kernel: a stationary device kernel, optionally ``+ WhiteNoise()``.
    :param mean: mean-function class or instance.
    :param hyperpars: ``[mean params | covariance params]``; omitted: found by maximising the bound.
    :param optimizer: ``"bfgs"`` (multi-start L-BFGS-B on the device gradient) or ``"diffev"``.
    :param n_starts: number of L-BFGS-B starts (default as `GpRegressor`).
    :param seed: seed of the inducing-point choice.
    :param inducing_method: what an int `inducing_points` means: ``"random"`` - the draw above - or ``"greedy"``: the rows
        `select_inducing_points` picks on the device at `hyperpars` (or, if they are to be searched, at the midpoint of
        `hp_bounds`, the search's own last start), weighted by 1 / (y_err^2 + s^2) when `y_err` was given.  Z keeps the
        order in which the rows were chosen; the selection is kept in `inducing_selection`.  A selection that stops
        short of m warns and the model is built with the rows it found.
    :param jitter: eps = jitter a^2 is added to the diagonal of K_mm.
    :param panel_rows: (extension) rows of x per panel of the device sweep; 0: the library's default.
    :param optimise_inducing: True: once the hyper-parameters are set, `optimise_inducing_points` moves Z - at the given
        `hyperpars`, or, if they were searched for, jointly with them from the result of that search.
    :param lockstep_search: (extension) True: the multi-start search advances all its starts in lockstep on
        `marginal_likelihood_gradient_batch` (`multistart_bfgs(lockstep=True)`).
    """

    def __init__(self, x, y, y_err=None, inducing_points=256, kernel=SquaredExponential, mean=ConstantMean, hyperpars=None,
                 optimizer="bfgs", n_starts=None, seed=None, jitter=1e-8, device=None, y_cov=None, panel_rows=0, optimise_inducing=False,
                 inducing_method="random", lockstep_search=False):
        if inducing_method not in INDUCING_METHODS:
            raise ValueError(f"inducing_method = {inducing_method!r}: must be one of {INDUCING_METHODS}")
        if inducing_method == "greedy" and not isinstance(inducing_points, (int, np.integer)):
            raise ValueError('inducing_method = "greedy" selects the inducing points itself: inducing_points must be an int')
        self.x, self.y = GpRegressor._coerce_training_data(x, y)
        self.x = np.ascontiguousarray(self.x, dtype=float)
        self.y = np.asarray(self.y, dtype=float)
        self.n_points, self.n_dimensions = self.x.shape
        if self.n_dimensions > msg.MAX_DIMENSIONS:
            raise ValueError(msg.too_many_dimensions("SparseGpRegressor", self.n_dimensions))
        if self.n_points < 2:
            raise ValueError("SparseGpRegressor needs at least two data points")
        if y_cov is not None:
            raise NotImplementedError(f"SparseGpRegressor does not take a dense y_cov; supported: {SUPPORTED}")
        self.n_points = self.y.size
        self._noise_var, _ = GpRegressor.check_error_data(self, y_err, None)

        self.cov = kernel() if isclass(kernel) else kernel
        self.mean = mean() if isclass(mean) else mean
        main = self.cov
        if _has_periodic(self.cov):
            raise NotImplementedError("SparseGpRegressor: the Periodic covariance function is not served by the "
                                      f"sparse-model kernels of the device; supported: {SUPPORTED}")
        if isinstance(self.cov, CompositeCovariance):
            parts = self.cov.components
            wn = [c for c in parts if isinstance(c, WhiteNoise)]
            stat = [c for c in parts if isinstance(c, _StationaryDeviceKernel)]
            if len(parts) != 2 or len(wn) != 1 or len(stat) != 1:
                raise NotImplementedError(f"SparseGpRegressor: unsupported covariance {type(self.cov).__name__}; supported: {SUPPORTED}")
            main = stat[0]
        if not isinstance(main, _StationaryDeviceKernel):
            raise NotImplementedError(f"SparseGpRegressor: unsupported covariance {type(main).__name__}; supported: {SUPPORTED}")
        self.cov.pass_spatial_data(self.x)
        self.mean.pass_spatial_data(self.x)
        self._kernel_id, _, self._stat_slice, self._wn_index = device_plan(self.cov)
        if self._noise_var is None and self._wn_index is None:
            raise ValueError("SparseGpRegressor needs noise: pass y_err or add WhiteNoise() to the kernel")
        if not (np.isfinite(jitter) and jitter >= 0.0):
            raise ValueError("jitter must be finite and not negative")
        self.jitter = float(jitter)
        self.panel_rows = int(panel_rows)

        if isinstance(inducing_points, (int, np.integer)):
            m = int(inducing_points)
            if not 1 <= m <= min(self.n_points, _lib.SGP_MAX_M):
                raise ValueError(f"inducing_points = {m}: an int must lie in 1 .. min(N, {_lib.SGP_MAX_M})")
            if inducing_method == "greedy":
                self.inducing_points = None  # (selected below, once the hyper-parameters' bounds are known)
            else:
                rows = np.sort(np.random.default_rng(seed).choice(self.n_points, m, replace=False))
                self.inducing_points = self.x[rows].copy()
        else:
            z = np.asarray(inducing_points, dtype=float)
            if z.ndim == 1 and self.n_dimensions == 1:
                z = z.reshape(-1, 1)
            if z.ndim != 2 or z.shape[1] != self.n_dimensions or not 1 <= z.shape[0] <= _lib.SGP_MAX_M:
                raise ValueError(f"inducing_points must be an (m, {self.n_dimensions}) array with 1 <= m <= {_lib.SGP_MAX_M}, "
                                 f"got shape {z.shape}")
            if not np.isfinite(z).all():
                raise ValueError("inducing_points must be finite")
            self.inducing_points = np.ascontiguousarray(z)

        if self.cov.bounds is None:
            self.cov.estimate_hyperpar_bounds(self.y)
        if self.mean.bounds is None:
            self.mean.estimate_hyperpar_bounds(self.y)
        self.hp_bounds = copy(self.mean.bounds)
        self.hp_bounds.extend(copy(self.cov.bounds))
        self.n_hyperpars = len(self.hp_bounds)
        self.mean_slice = slice(0, self.mean.n_params)
        self.cov_slice = slice(self.mean.n_params, self.n_hyperpars)
        self.hyperpar_labels = [*self.mean.hyperpar_labels, *self.cov.hyperpar_labels]
        self._device = device
        self._engine = None
        self._targets_mean = None
        self._observations_up = False
        self._batch_independent = False

        if self.inducing_points is None:
            at = hyperpars if hyperpars is not None else [0.5 * (lo + hi) for lo, hi in self.hp_bounds]
            self.inducing_points, self.inducing_selection = self._greedy_selection(int(inducing_points), at, 0.0)

        searched = hyperpars is None
        if hyperpars is None:
            if optimizer not in ["bfgs", "diffev"]:
                optimizer = "bfgs"
                warn(msg.BAD_OPTIMIZER)
            hyperpars = (self.differential_evo() if optimizer == "diffev"
                         else self.multistart_bfgs(starts=n_starts, lockstep=bool(lockstep_search)))
        self.set_hyperparameters(hyperpars)
        if optimise_inducing:
            self.optimise_inducing_points(hyperpars=searched)

    # ---- device plumbing -----------------------------------------------------------------------------------------
    @property
    def engine(self) -> SparseEngine:
        if self._engine is None:
            self._engine = SparseEngine(self.x, self.inducing_points, device=self._device)
            if "hyperpars" in self.__dict__:  # (a model back from pickle: the fit goes with the new engine)
                self.set_hyperparameters(self.hyperpars)
        return self._engine

    def _split(self, theta):
        """theta -> (stationary-kernel parameters, WhiteNoise variance); the residual of theta's mean goes to the device
        when it differs from the one already there."""
        theta = np.asarray(theta, dtype=float)
        if theta.size != self.n_hyperpars:
            raise ValueError(msg.wrong_hyperpar_count(self.n_hyperpars, theta.size))
        theta_mean, theta_cov = theta[self.mean_slice], theta[self.cov_slice]
        if self._targets_mean is None or not np.array_equal(self._targets_mean, theta_mean):
            self.engine.set_targets(self.y - self.mean.build_mean(theta_mean), self._noise_var)
            self._targets_mean = np.array(theta_mean)
        white = float(np.exp(2.0 * theta_cov[self._wn_index])) if self._wn_index is not None else 0.0
        return np.ascontiguousarray(theta_cov[self._stat_slice]), white

    # ---- the bound -----------------------------------------------------------------------------------------------
    def marginal_likelihood(self, theta) -> float:
        """The variational lower bound F of the log marginal likelihood; -1e50 where a factorisation fails."""
        if self._batch_independent:
            return float(self.marginal_likelihood_batch(np.asarray(theta, dtype=float)[None, :])[0])
        theta_stat, white = self._split(theta)
        F, _, _, info = self.engine.bound(self._kernel_id, theta_stat, white, self.jitter, self.panel_rows)
        if info != 0:
            warn("Cholesky decomposition failure in marginal_likelihood")
            return -1e50
        return float(F)

    def marginal_likelihood_gradient(self, theta, inducing_points=False):
        """(F, dF/dtheta) with the gradient from the device; the mean parameters' part is (d mu / d theta)^T alpha.
        inducing_points=True: (F, dF/dtheta, dF/dZ) with the (m, d) gradient by the inducing inputs."""
        theta = np.asarray(theta, dtype=float)
        if self._batch_independent and not inducing_points:
            F, grad = self.marginal_likelihood_gradient_batch(theta[None, :])
            return float(F[0]), grad[0]
        theta_stat, white = self._split(theta)
        F, g, alpha, info, *zgrad = self.engine.bound(self._kernel_id, theta_stat, white, self.jitter, self.panel_rows, True, True,
                                                      want_zgrad=bool(inducing_points))
        if info != 0:
            raise LinAlgError("Matrix is not positive definite")
        grad = np.zeros(self.n_hyperpars)
        _, mean_grads = self.mean.mean_and_gradients(theta[self.mean_slice])
        grad[self.mean_slice] = [float(np.dot(dmu, alpha)) for dmu in mean_grads]
        cov_grad = np.zeros(self.cov.n_params)
        cov_grad[self._stat_slice] = g[:-1]
        if self._wn_index is not None:
            cov_grad[self._wn_index] = g[-1]
        grad[self.cov_slice] = cov_grad
        if inducing_points:
            return float(F), grad, zgrad[0]
        return float(F), grad

    # ---- lockstep batches of the bound (as GpRegressor's: what the lockstep drivers of inference_amd.mcmc call) -------
    def batch_independent_values(self, on: bool = True):
        """(extension) on: `marginal_likelihood` and `marginal_likelihood_gradient(theta)` go through a batch of one, whose
        values are, bit for bit, those of the same theta anywhere inside `marginal_likelihood_batch` /
        `marginal_likelihood_gradient_batch` - a chain advanced alone then walks the trajectory it walks in lockstep.  The
        gradient by the inducing inputs (`inducing_points=True`) keeps the single evaluation.  Off (the default): both are
        the single evaluations."""
        self._batch_independent = bool(on)

    def _batch_call(self, thetas, want_grad):
        """(thetas (T, P), means or None, the engine's bound_batch results) for T full hyper-parameter vectors."""
        thetas = np.atleast_2d(np.asarray(thetas, dtype=float))
        if thetas.ndim != 2 or thetas.shape[1] != self.n_hyperpars:
            raise ValueError(msg.wrong_hyperpar_count(self.n_hyperpars, thetas.shape[-1]))
        if not np.isfinite(thetas).all():
            raise ValueError("the hyper-parameters of a batch must be finite")
        if not self._observations_up:
            self.engine.set_observations(self.y, self._noise_var)
            self._observations_up = True
        cov = thetas[:, self.cov_slice]
        white = np.exp(2.0 * cov[:, self._wn_index]) if self._wn_index is not None else np.zeros(len(thetas))
        constant = isinstance(self.mean, ConstantMean)
        means = None if constant else [self.mean.mean_and_gradients(t[self.mean_slice]) for t in thetas]
        mean_kw = dict(mu_const=thetas[:, 0]) if constant else dict(mus=np.array([mu for mu, _ in means]))
        out = self.engine.bound_batch(self._kernel_id, np.ascontiguousarray(cov[:, self._stat_slice]), white, self.jitter,
                                      self.panel_rows, want_grad=want_grad, want_alpha=want_grad and not constant, **mean_kw)
        return thetas, means, out

    def marginal_likelihood_batch(self, thetas) -> np.ndarray:
        """(extension) The bound F for T hyper-parameter vectors in one device call (gpmi_sgp_bound_batch: every launch
        carries all of them); -1e50 where a factorisation fails, with one warning per call.  A row's value does not depend
        on the rows it shares the call with."""
        thetas = np.asarray(thetas, dtype=float)
        if thetas.size == 0:
            return np.empty(0)
        _, _, (F, _, _, _, info) = self._batch_call(thetas, False)
        if (info != 0).any():
            warn("Cholesky decomposition failure in marginal_likelihood")
            F[info != 0] = -1e50
        return F

    def marginal_likelihood_gradient_batch(self, thetas, failed: str = "raise"):
        """(extension) (F (T,), dF/dtheta (T, P)) for T hyper-parameter vectors in one device call.  A vector whose
        matrices are not positive definite raises LinAlgError for the whole batch; with `failed="sentinel"` such a row
        gets -1e50 and a zero gradient instead (one warning per call) and the other rows keep their values."""
        if failed not in ("raise", "sentinel"):
            raise ValueError("'failed' must be \"raise\" or \"sentinel\"")
        thetas = np.asarray(thetas, dtype=float)
        if thetas.size == 0:
            return np.empty(0), np.empty((0, self.n_hyperpars))
        thetas, means, (F, g, sum_alpha, alpha, info) = self._batch_call(thetas, True)
        grads = np.zeros((len(thetas), self.n_hyperpars))
        if means is None:
            grads[:, 0] = sum_alpha  # ConstantMean: d mu / d theta_0 = 1
        else:
            for t, (_, mean_grads) in enumerate(means):
                grads[t, self.mean_slice] = [float(np.dot(dmu, alpha[t])) for dmu in mean_grads]
        cov_grads = np.zeros((len(thetas), self.cov.n_params))
        cov_grads[:, self._stat_slice] = g[:, :-1]
        if self._wn_index is not None:
            cov_grads[:, self._wn_index] = g[:, -1]
        grads[:, self.cov_slice] = cov_grads
        return GpRegressor._failed_rows(F, grads, info, failed)

    def set_hyperparameters(self, hyperpars):
        hyperpars = np.asarray(hyperpars, dtype=float)
        theta_stat, white = self._split(hyperpars)
        F, info = self.engine.fit(self._kernel_id, theta_stat, white, self.jitter, self.panel_rows)
        if info != 0:
            raise LinAlgError("Matrix is not positive definite")
        self.hyperpars = hyperpars
        self.mean_hyperpars = hyperpars[self.mean_slice]
        self.cov_hyperpars = hyperpars[self.cov_slice]
        self.bound = float(F)

    # ---- the inducing inputs ---------------------------------------------------------------------------------------
    def _check_inducing(self, z):
        z = np.asarray(z, dtype=float)
        if z.ndim == 1 and self.n_dimensions == 1:
            z = z.reshape(-1, 1)
        if z.shape != self.inducing_points.shape:
            raise ValueError(f"inducing points must keep their shape {self.inducing_points.shape}, got {z.shape}")
        if not np.isfinite(z).all():
            raise ValueError("inducing points must be finite")
        return np.array(z, dtype=float, order="C")

    def _move(self, z, hyperpars):
        """Z and the hyper-parameters together, with one fit; a fit that fails puts the previous Z and fit back."""
        old_z, old_hp = self.inducing_points, self.hyperpars
        self.engine.set_inducing(z)
        self.inducing_points = z
        try:
            self.set_hyperparameters(hyperpars)
        except LinAlgError:
            self.engine.set_inducing(old_z)
            self.inducing_points = old_z
            self.set_hyperparameters(old_hp)
            raise

    def set_inducing_points(self, z):
        """Move the inducing inputs to the (m, d) finite array z (same m) and fit again at the current hyper-parameters.
        ValueError for anything else, LinAlgError if the fit fails; both leave the previous Z and fit in place."""
        self._move(self._check_inducing(z), self.hyperpars)

    def _greedy_selection(self, m, theta, tol):
        """(Z in pivot order, dict(indices, trace, pivot_variances)) of the greedy selection at theta; warns if it stopped
        short of m."""
        theta = np.asarray(theta, dtype=float)
        if theta.size != self.n_hyperpars:
            raise ValueError(msg.wrong_hyperpar_count(self.n_hyperpars, theta.size))
        theta_cov = theta[self.cov_slice]
        white = float(np.exp(2.0 * theta_cov[self._wn_index])) if self._wn_index is not None else 0.0
        weights = None if self._noise_var is None else 1.0 / (self._noise_var + white)
        index, trace, pivot_var = _select_on_device(self.x, m, self._kernel_id, theta_cov[self._stat_slice], weights, tol, 1e-8,
                                                    self._device)
        if len(index) < m:
            warn(f"the greedy selection stopped at {len(index)} of {m} inducing points: the model is built with those")
        return self.x[index].copy(), dict(indices=index, trace=trace, pivot_variances=pivot_var)

    def reselect_inducing_points(self, m=None, tol=0.0):
        """Select the inducing points again, greedily at the current hyper-parameters (`select_inducing_points`; m: the
        current number), and fit there.  Returns (F_before, F_after).  Another number of points rebuilds the device
        object.  LinAlgError if the fit fails: the previous Z and fit are put back."""
        m = self.inducing_points.shape[0] if m is None else int(m)
        if not 1 <= m <= min(self.n_points, _lib.SGP_MAX_M):
            raise ValueError(f"m = {m}: must lie in 1 .. min(N, {_lib.SGP_MAX_M})")
        F_before = self.bound
        z, selection = self._greedy_selection(m, self.hyperpars, tol)
        if z.shape == self.inducing_points.shape:
            self._move(z, self.hyperpars)
        else:
            old_z = self.inducing_points
            try:
                self._rebuild(z)
            except LinAlgError:
                self._rebuild(old_z)
                raise
        self.inducing_selection = selection
        return F_before, self.bound

    def _rebuild(self, z):
        """Z of another shape: the engine is dropped and built anew with the fit, as for a model back from pickle."""
        self.inducing_points = z
        self._engine = None
        self._targets_mean = None
        self._observations_up = False
        self.set_hyperparameters(self.hyperpars)

    def optimise_inducing_points(self, hyperpars=True, maxiter=200):
        """One L-BFGS-B on the device gradients from the current state, over vec(Z) or (hyperpars=True) [theta | vec(Z)]:
        theta inside `hp_bounds`, every coordinate of Z inside the bounding box of that column of x.  Leaves the model
        fitted at the best point found - the start, if nothing better was - and returns (F_before, F_after), also kept
        with the number of evaluations and L-BFGS-B's warnflag in `inducing_log`."""
        theta0, z0, F_before = np.array(self.hyperpars), self.inducing_points.copy(), self.bound
        nh = self.n_hyperpars if hyperpars else 0
        lo, hi = self.x.min(axis=0), self.x.max(axis=0)
        bounds = list(self.hp_bounds[:nh]) + [(lo[k], hi[k]) for _ in range(z0.shape[0]) for k in range(z0.shape[1])]

        def cost(v):
            self.engine.set_inducing(v[nh:].reshape(z0.shape))
            try:
                F, g, gz = self.marginal_likelihood_gradient(v[:nh] if hyperpars else theta0, inducing_points=True)
            except LinAlgError:
                return 1e50, np.zeros(v.size)
            return -F, -np.concatenate([g[:nh], gz.ravel()])

        try:
            best, _, info = fmin_l_bfgs_b(func=cost, x0=np.concatenate([theta0[:nh], z0.ravel()]), approx_grad=False,
                                          bounds=bounds, maxiter=maxiter)
        finally:
            self.engine.set_inducing(z0)  # (the search moved the device's Z, not the model's)
        try:
            self._move(np.array(best[nh:].reshape(z0.shape), order="C"), best[:nh] if hyperpars else theta0)
        except LinAlgError:
            pass  # (_move has put the start back)
        if self.bound < F_before:
            self._move(z0, theta0)
        self.inducing_log = dict(F_before=F_before, F_after=self.bound, evaluations=int(info["funcalls"]),
                                 warnflag=int(info["warnflag"]))
        return F_before, self.bound

    def __call__(self, points):
        """(mean, standard deviation) of the latent function at the points, as `GpRegressor.__call__`."""
        q = np.ascontiguousarray(GpRegressor.process_points(self, points), dtype=float)
        mean, var = self.engine.predict(q)
        return mean + GpRegressor._mean_at(self, q), np.sqrt(np.abs(var))

    # ---- the fitted model beyond mean and standard deviation (as GpRegressor) ---------------------------------------
    def process_points(self, points):
        """Bring query points to shape (M, d), as `GpRegressor.process_points`."""
        return GpRegressor.process_points(self, points)

    def _query(self, points):
        return np.ascontiguousarray(self.process_points(points), dtype=float)

    def build_posterior(self, points, mean_only=False):
        """Posterior mean vector (with the mean function) and covariance matrix of the latent function at the M points,
        as `GpRegressor.build_posterior`: mu = U c, Sigma = K_qq - V V^T + U U^T (include/gpmi.h: gpmi_sgp_posterior)."""
        q = self._query(points)
        mu, sigma = self.engine.posterior(q, mean_only=mean_only)
        mu = mu + GpRegressor._mean_at(self, q)
        if mean_only:
            return mu
        return mu, sigma

    def sample_posterior(self, points, n_draws=1, *, seed=None, z=None, jitter=1e-9, first_draw=0):
        """`n_draws` joint draws of the latent function at the M `points`, shape (n_draws, M): mu + z_s L^T with
        L L^T = Sigma + eps I for the mean and covariance of `build_posterior` and eps = jitter * max diag(Sigma), on the
        device.  Arguments, the generator's stream and `last_sample_seed` as `GpRegressor.sample_posterior`.  Sigma is
        numerically singular from about a hundred points on: keep a positive `jitter`.
        Raises numpy.linalg.LinAlgError if Sigma + eps I is not positive definite."""
        q = self._query(points)
        n_draws, seed, z, jitter, first_draw = draw_arguments("SparseGpRegressor", len(q), n_draws, seed, z, jitter, first_draw)
        draws, _, eps, info = self.engine.posterior_draws(q, n_draws=n_draws, seed=0 if seed is None else seed, z=z,
                                                          jitter=jitter, first_draw=first_draw)
        if info == 0:
            draws += GpRegressor._mean_at(self, q)
        self.last_sample_seed = seed
        raise_if_not_positive_definite("SparseGpRegressor", info, jitter, eps)
        return draws

    def spatial_derivatives(self, points):
        """Gradients of the predictive mean and variance at the points, squeezed as `GpRegressor.spatial_derivatives`
        (all four kernels, RationalQuadratic included).  As there, the derivative of the mean function is not added: the
        results are those of the zero-mean latent part, exact for `ConstantMean`.  The accuracy of the mean's gradient
        scales with cond(K_mm + eps I) (include/gpmi.h): about 1e-6 relative at cond 1e6."""
        dmu, dvar = self.engine.spatial_derivatives(self._query(points))
        return dmu.squeeze(), dvar.squeeze()

    def spatial_derivatives_batch(self, points):
        """`spatial_derivatives` for M points with un-squeezed (M, d) results: the form the batched acquisition functions
        consume.  Row j depends on (fit, point j) alone, bit for bit."""
        return self.engine.spatial_derivatives(self._query(points))

    # ---- hyper-parameter search (as GpRegressor: SciPy on the host, every evaluation on the device) ----------------
    def bfgs_cost_func(self, theta):
        try:
            F, g = self.marginal_likelihood_gradient(theta)
        except LinAlgError:
            return 1e50, np.zeros(self.n_hyperpars)
        return -F, -g

    def multistart_bfgs(self, starts=None, lockstep=False):
        """Multi-start L-BFGS-B on the device gradient, one start after another; lockstep=True: all starts advance together
        (gp/_lockstep.py), one `marginal_likelihood_gradient_batch` per round, a failed row counted as 1e50 with a zero
        gradient as `bfgs_cost_func` counts it."""
        if starts is None:
            starts = int(2 * np.sqrt(len(self.hp_bounds))) + 1
        lwr, upr = [np.array([k[i] for k in self.hp_bounds]) for i in [0, 1]]
        starting_positions = [lwr + (upr - lwr) * random(size=len(self.hp_bounds)) for _ in range(starts - 1)]
        starting_positions.append(0.5 * (lwr + upr))
        if lockstep:
            from inference_amd.gp._lockstep import lockstep_lbfgsb
            from warnings import catch_warnings, simplefilter

            def neg_batch(X):
                with catch_warnings():
                    simplefilter("ignore")
                    F, g = self.marginal_likelihood_gradient_batch(X, failed="sentinel")
                return -F, -g

            results = lockstep_lbfgsb(neg_batch, np.array(starting_positions), self.hp_bounds)
        else:
            results = [fmin_l_bfgs_b(func=self.bfgs_cost_func, x0=x0, approx_grad=False, bounds=self.hp_bounds)
                       for x0 in starting_positions]
        self.search_log = [(np.array(x0), np.array(r[0]), float(r[1])) for x0, r in zip(starting_positions, results)]
        return sorted(results, key=lambda r: r[1])[0][0]

    def differential_evo(self):
        from warnings import catch_warnings, simplefilter

        def neg(t):
            with catch_warnings():
                simplefilter("ignore")
                return -self.marginal_likelihood(t)

        return differential_evolution(func=neg, bounds=self.hp_bounds).x

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engine"] = None
        state["_targets_mean"] = None
        state["_observations_up"] = False
        return state

    def __str__(self):
        pad = max(len(label) for label in self.hyperpar_labels) + 2
        lines = ["\n[ SparseGpRegressor hyperparameters ]\n"]
        for label, val in zip(self.hyperpar_labels, self.hyperpars):
            lines.append(f"{label:>{pad}} = {val:.4}\n")
        return "".join(lines)
