"""
`GeneralisedGpRegressor` (extension: the reference has no counterpart) - Gaussian-process regression through a
non-Gaussian, log-concave likelihood by Laplace's method (Rasmussen & Williams, GPML, Alg. 3.1, 3.2 and 5.1).

With the constant offset m, the latent f = m + K a and psi(a) = -1/2 a^T (f - m) + sum_i log p(y_i | f_i), a Newton step
takes g = d log p / df, W = -d^2 log p / df^2, sw = sqrt W, factorises B = I + sw sw^T o K = L L^T and sets

    b = W (f - m) + g,     a+ = b - sw o L^-T L^-1 (sw o K b),     f+ = m + K a+,

halving the step along a+ - a (at most ten times) while psi(a+) < psi(a) - 1e-12 |psi(a)|, until
max |f+ - f| <= tol (1 + max |f+|).  Every evaluation starts from a = 0: a value depends on theta alone.  At the mode

    log q(y | theta) = psi - sum_i ln L_ii
    mean(q) = m + k(q)^T g,      var(q) = k(q, q) - |L^-1 (sw o k(q))|^2
    d log q / d theta_j = 1/2 sum_ab [1/2 (u g^T + g u^T) - R]_ab (dK / d theta_j)_ab
        R = sw sw^T o B^-1,  s2 = 1/2 (diag K - diag(K R K)) o d3,  w = s2 - R K s2,  u = g + 2 w

(the sign of s2 is that of d3 = d^3 log p / df^3: GPML's printed eq. 5.23 has it the other way).  The iteration, the
factorisations and the gradient run on the device (gpmi_ggp_*, csrc/api_generalised.hip); `predict_response` is O(M) on
the host.
"""
from copy import copy
from inspect import isclass
from warnings import warn

import numpy as np
from numpy import array, ndarray, sqrt
from numpy.random import random
from scipy.optimize import fmin_l_bfgs_b

from inference_amd._engine import GpEngine
from inference_amd.gp import _messages as msg
from inference_amd.gp.covariance import CovarianceFunction, Periodic, SquaredExponential, _StationaryDeviceKernel
from inference_amd.gp.likelihood import Binomial, Likelihood, Logistic, Poisson, logistic_parts

MAX_COLUMNS = 64  # of x: the covariance kernels' limit


class GeneralisedGpRegressor:
    """
    :param x: (N, d) array of point coordinates; 1-D input means d = 1.
    :param y: (N,) observations in the domain of the likelihood.
    :param likelihood: a `Logistic`, `Poisson` or `Binomial` instance (or class: its defaults).
    :param kernel: one of `SquaredExponential`, `RationalQuadratic`, `Matern32`, `Matern52`.  The latent covariance \
        carries no noise term: `+ WhiteNoise()`, sums, `ChangePoint`, `HeteroscedasticNoise` and plugin kernels raise \
        `NotImplementedError`.
    :param hyperpars: the covariance hyper-parameters (layout, labels and bounds are the kernel's own); when omitted \
        they are found by a multi-start L-BFGS-B maximisation of the Laplace log-evidence.
    :param offset: the constant prior mean m of f - a number, not a hyper-parameter.  None: mean(y) for `Logistic`, \
        ln max(mean(y / e), 1e-3) for `Poisson`, 0 for `Binomial`.
    :param int n_starts: number of L-BFGS-B starting positions.
    :param device: HIP device index; default ``LOCAL_RANK`` / 0.
    :param tol, max_iter: the stopping rule of Newton's iteration.
    """

    def __init__(self, x: ndarray, y: ndarray, likelihood: Likelihood = Logistic, kernel: CovarianceFunction = SquaredExponential,
                 hyperpars: ndarray = None, offset: float = None, n_starts: int = None, device: int = None,
                 tol: float = 1e-9, max_iter: int = 50):
        # every argument check runs before the first device call
        self.x, self.y = self._coerce_training_data(x, y)
        self.n_points, self.n_dimensions = self.x.shape
        if self.n_dimensions > MAX_COLUMNS or self.n_dimensions > msg.MAX_DIMENSIONS:
            raise ValueError(msg.too_many_dimensions("GeneralisedGpRegressor", self.n_dimensions))
        self.likelihood = likelihood() if isclass(likelihood) else likelihood
        if not isinstance(self.likelihood, (Logistic, Poisson, Binomial)):
            raise NotImplementedError(
                f"[ GeneralisedGpRegressor error ] The likelihood {type(self.likelihood).__name__} is not served: one of "
                "Logistic, Poisson, Binomial (log-concave likelihoods; Cauchy and Student-t need another algorithm).")
        self.aux = self.likelihood.bind(self.n_points)
        self.likelihood.check(self.y)
        if not (0.0 < float(tol) < 1.0) or int(max_iter) < 1:
            raise ValueError("[ GeneralisedGpRegressor error ] 'tol' must lie in (0, 1) and 'max_iter' be at least 1.")
        self.tol, self.max_iter = float(tol), int(max_iter)
        if offset is None:
            offset = self.likelihood.default_offset(self.y, self.aux)
        if np.ndim(offset) != 0 or not np.isfinite(float(offset)):
            raise ValueError("[ GeneralisedGpRegressor error ] 'offset' must be None or a finite number.")
        self.offset = float(offset)

        self.cov = kernel() if isclass(kernel) else kernel
        if isinstance(self.cov, Periodic):
            raise NotImplementedError("[ GeneralisedGpRegressor error ] The Periodic covariance function is not served by "
                                      "the generalised-GP entry points of the device.")
        if not isinstance(self.cov, _StationaryDeviceKernel):
            raise NotImplementedError(
                f"[ GeneralisedGpRegressor error ] The covariance function {type(self.cov).__name__} is not served: one "
                "of SquaredExponential, RationalQuadratic, Matern32, Matern52 (no WhiteNoise, no sums, no ChangePoint, "
                "no HeteroscedasticNoise, no plugin kernels).")
        self.cov.pass_spatial_data(self.x)
        self._kernel_id = self.cov._gpmi_kernel
        if self.cov.bounds is None:
            self.cov.estimate_hyperpar_bounds(self.likelihood.latent_proxy(self.y, self.aux) - self.offset)
        self.hp_bounds = copy(self.cov.bounds)
        self.n_hyperpars = len(self.hp_bounds)
        self.hyperpar_labels = [*self.cov.hyperpar_labels]
        if hyperpars is not None:
            self._theta(hyperpars)
        self._device = device
        self._engine = None
        self._mode = None

        if hyperpars is None:
            hyperpars = self.multistart_bfgs(starts=n_starts)
        self.set_hyperparameters(hyperpars)

    # ---------------------------------------------------------------------------------
    # argument checks (no device call)
    # ---------------------------------------------------------------------------------
    @staticmethod
    def _coerce_training_data(x, y):
        xa = np.asarray(x)
        ya = np.asarray(y, dtype=float)
        ya = ya.squeeze() if ya.ndim > 1 else ya
        if ya.ndim != 1 or ya.size < 1:
            raise ValueError(f"[ GeneralisedGpRegressor error ] 'y' must be an (N,) array, but has shape {np.shape(y)}.")
        if xa.ndim > 2:
            raise ValueError(msg.x_not_2d(xa.ndim, xa.shape))
        if xa.ndim < 2:
            xa = xa.reshape([xa.size, 1])
        if xa.shape[0] != ya.shape[0]:
            raise ValueError(f"[ GeneralisedGpRegressor error ] The first dimensions of 'x' and 'y' must agree: 'x' has "
                             f"shape {xa.shape}, 'y' has shape {ya.shape}.")
        return np.ascontiguousarray(xa, dtype=float), np.ascontiguousarray(ya)

    def _theta(self, theta):
        theta = np.asarray(theta, dtype=float)
        if theta.shape != (self.n_hyperpars,):
            raise ValueError(msg.wrong_hyperpar_count(self.n_hyperpars, theta.size))
        return np.ascontiguousarray(theta)

    # ---------------------------------------------------------------------------------
    # device plumbing
    # ---------------------------------------------------------------------------------
    @property
    def engine(self) -> GpEngine:
        if self._engine is None:
            eng = GpEngine(self.x, np.zeros(self.n_points), device=self._device)
            eng.ggp_set_observations(self.likelihood.code, self.y, self.aux, self.offset)
            self._engine = eng
        return self._engine

    def __getstate__(self):
        state = self.__dict__.copy()  # device handles do not pickle: re-attached lazily (the fit is not: set_hyperparameters)
        state["_engine"] = None
        return state

    # ---------------------------------------------------------------------------------
    # public API
    # ---------------------------------------------------------------------------------
    def set_hyperparameters(self, hyperpars: ndarray):
        """Update the hyper-parameters and find the mode again; `RuntimeError` if Newton's iteration fails."""
        theta = self._theta(hyperpars)
        self._mode = None
        logq, (iters, halvings), info = self.engine.ggp_fit(self._kernel_id, theta, self.tol, self.max_iter)
        self._newton = dict(iterations=iters, halvings=halvings, converged=info == 0, psi=None)
        if info != 0:
            raise RuntimeError(self._failure(info))
        self.hyperpars = theta.copy()
        self._logq = logq

    def _failure(self, info):
        if info > 0:
            return (f"[ GeneralisedGpRegressor error ] B = I + W^1/2 K W^1/2 did not factorise at leading minor {info}: "
                    "the covariance is not finite at these hyper-parameters.")
        return (f"[ GeneralisedGpRegressor error ] Newton's iteration did not converge within max_iter = {self.max_iter} "
                "steps.")

    def _fetch_mode(self):
        if self._mode is None:
            f, g = self.engine.ggp_mode()
            self._mode = (f, g)
            lp = self.likelihood.log_prob(self.y, f, self.aux).sum()
            self._newton["psi"] = float(-0.5 * g @ (f - self.offset) + lp)
        return self._mode

    @property
    def newton_log(self) -> dict:
        """dict(iterations, halvings, converged, psi) of the last `set_hyperparameters`; psi is evaluated on the host
        from the downloaded mode."""
        if self._newton["converged"] and self._newton["psi"] is None:
            self._fetch_mode()
        return dict(self._newton)

    @property
    def mode(self) -> ndarray:
        """f-hat (N,): the maximiser of p(y | f) p(f | theta)."""
        return self._fetch_mode()[0]

    @property
    def alpha(self) -> ndarray:
        """a = grad log p(y | f-hat) (N,): K a = f-hat - m at the mode."""
        return self._fetch_mode()[1]

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
        """Mean and standard deviation, sqrt(abs(var)) as `GpRegressor`, of the latent f at the points."""
        mean, var = self.engine.ggp_predict(self.process_points(points))
        return mean, sqrt(abs(var))

    def predict_response(self, points: ndarray, aux=None):
        """Mean and standard deviation of a new observation y* at the points, O(M) on the host from the latent
        N(mu, sigma^2).  `aux`: the exposure (`Poisson`), trials (`Binomial`) or noise sigma (`Logistic`) of the new
        observations, scalar or (M,); default 1 (`Logistic`: the mean of the training sigmas).
        `Poisson`: lognormal-Poisson moments; `Binomial`: 32-point Gauss-Hermite; `Logistic`: mu, sqrt(sigma^2 + noise^2)."""
        mu, sig = self(points)
        return response_moments(self.likelihood, mu, sig, aux)

    def marginal_likelihood(self, theta: ndarray) -> float:
        """The Laplace log-evidence log q(y | theta); -1e50 (with one `RuntimeWarning`) where the iteration fails."""
        logq, _, info = self.engine.ggp_logq(self._kernel_id, self._theta(theta), self.tol, self.max_iter)
        if info != 0:
            warn(self._failure(info), RuntimeWarning)
            return -1e50
        return float(logq)

    def marginal_likelihood_batch(self, thetas: ndarray) -> ndarray:
        """`marginal_likelihood` for B hyper-parameter vectors, one after another; -1e50 rows for failures."""
        thetas = np.asarray(thetas, dtype=float)
        if thetas.size == 0:
            return np.empty(0)
        rows = np.atleast_2d(thetas)
        out = np.empty(len(rows))
        failed = 0
        for b, t in enumerate(rows):
            logq, _, info = self.engine.ggp_logq(self._kernel_id, self._theta(t), self.tol, self.max_iter)
            failed += info != 0
            out[b] = logq if info == 0 else -1e50
        if failed:
            warn(f"[ GeneralisedGpRegressor ] Newton's iteration failed at {failed} of {len(rows)} hyper-parameter vectors",
                 RuntimeWarning)
        return out

    def marginal_likelihood_gradient(self, theta: ndarray):
        """(log q, gradient by theta), explicit and implicit parts; `RuntimeError` where the iteration fails."""
        logq, grad, _, info = self.engine.ggp_logq_grad(self._kernel_id, self._theta(theta), self.tol, self.max_iter)
        if info != 0:
            raise RuntimeError(self._failure(info))
        return float(logq), grad

    # ---------------------------------------------------------------------------------
    # hyper-parameter search
    # ---------------------------------------------------------------------------------
    def bfgs_cost_func(self, theta: ndarray):
        try:
            y, grad_y = self.marginal_likelihood_gradient(theta)
        except RuntimeError:
            return 1e50, np.zeros(self.n_hyperpars)
        return -y, -grad_y

    def multistart_bfgs(self, starts: int = None):
        """Multi-start L-BFGS-B on the device gradient, the starts drawn as `MultiTargetGpRegressor.multistart_bfgs` draws
        them and run one after another.  `search_log`: dict(starts, start_values, values)."""
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
        lines = [f"\n[ GeneralisedGpRegressor hyperparameters: {self.likelihood.name} likelihood ]\n"]
        for label, val in zip(self.hyperpar_labels, self.hyperpars):
            lines.append(f"{label:>{pad}} = {val:.4}\n")
        return "".join(lines)


_GH_X, _GH_W = np.polynomial.hermite_e.hermegauss(32)
_GH_W = _GH_W / _GH_W.sum()


def response_moments(likelihood, mu, sig, aux=None):
    """Mean and standard deviation of y* given the latent N(mu, sig^2) per point (see `predict_response`)."""
    mu, sig = np.asarray(mu, dtype=float), np.asarray(sig, dtype=float)
    if aux is None:
        aux = float(np.mean(likelihood.noise_sigma)) if isinstance(likelihood, Logistic) else 1.0
    aux = np.broadcast_to(np.asarray(aux, dtype=float), mu.shape)
    if isinstance(likelihood, Logistic):
        return mu.copy(), sqrt(sig**2 + aux**2)
    if isinstance(likelihood, Poisson):
        # y* | f ~ Poisson(e exp f), f ~ N(mu, sig^2): E = e exp(mu + sig^2 / 2), Var = E + E^2 (exp(sig^2) - 1)
        mean = aux * np.exp(mu + 0.5 * sig**2)
        return mean, sqrt(mean + mean**2 * np.expm1(sig**2))
    # Binomial: p = sigma(f); E = n E[p], Var = n E[p (1 - p)] + n^2 Var[p]
    f = mu[:, None] + sig[:, None] * _GH_X[None, :]
    p, p1m, _ = logistic_parts(f)
    ep = p @ _GH_W
    ep2 = (p * p) @ _GH_W
    var = aux * (p1m @ _GH_W) + aux**2 * np.maximum(ep2 - ep**2, 0.0)
    return aux * ep, sqrt(var)
