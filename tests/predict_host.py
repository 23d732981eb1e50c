"""Host reference of the hyper-parameter-marginalised prediction (`GpRegressor.predict_samples` /
`predict_marginalised`, gpmi_predict_batch), shared by tests/test_predict_batch_cpu.py and tests/test_predict_batch_gpu.py.

Per hyper-parameter vector the reference is the CPU oracle: `OracleGp.set_hyperparameters(theta_t)` followed by
`oracle(points)` for the models the oracle restates (one SE / RQ kernel, optionally + WhiteNoise, ConstantMean).  A sum of
kernels and a LinearMean are not in `OracleGp`; for them `HostSum` composes the same steps (regression.py:218-244, 188-216)
from the oracle's covariance builders.  The mixture over the vectors is the two-pass law of total variance in NumPy, with
failed rows left out and the remaining weights renormalised.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import workloads as wl
from oracle import gp_oracle as orc

# (tag, kinds, WhiteNoise, mean, seed, N, d): the models of the GPU tests.  Data: workloads.synthetic_dataset (y_err = 0.1)
MODELS = {
    "a": ((orc.SE,), False, "const", 5, 48, 1),      # one padded tile
    "b": ((orc.SE,), True, "const", 7, 200, 2),      # two tiles
    "c": ((orc.RQ,), False, "const", 11, 300, 3),    # three tiles
    "d": ((orc.SE, orc.RQ), False, "const", 13, 130, 2),  # a sum, two points past a tile edge
    "e": ((orc.SE,), False, "linear", 5, 48, 1),     # model (a) with a LinearMean
}


def dataset(tag):
    _, _, _, seed, n, d = MODELS[tag]
    return wl.synthetic_dataset(seed, n, d)


def middle_half(bounds, T, seed):
    """T vectors drawn from the middle half of every interval of `bounds` (seeded)."""
    b = np.asarray(bounds, dtype=float)
    u = np.random.default_rng(seed).uniform(0.25, 0.75, (T, len(b)))
    return b[:, 0] + u * (b[:, 1] - b[:, 0])


class HostSum:
    """The steps of OracleGp.set_hyperparameters / __call__ for a sum of SE / RQ kernels (+ WhiteNoise) with a Constant or
    Linear mean: theta = [mean | component 1 | component 2 ... | ln sigma_n]."""

    def __init__(self, x, y, y_err, kinds, white_noise=False, mean="const"):
        self.x = np.asarray(x, float).reshape(len(y), -1)
        self.y = np.asarray(y, float)
        self.n, self.d = self.x.shape
        self.sig = np.asarray(y_err, float) ** 2
        self.kinds, self.white_noise, self.mean = tuple(kinds), white_noise, mean
        self.n_mean = 1 if mean == "const" else 1 + self.d
        self.x_mean = self.x.mean(axis=0)

    def _mean(self, pts, th):
        if self.mean == "const":
            return np.full(len(pts), th[0])
        return th[0] + (pts - self.x_mean[None, :]) @ th[1:]

    def _parts(self, theta_cov):
        off, parts = 0, []
        for k in self.kinds:
            nk = orc.kernel_n_params(k, self.d)
            parts.append((k, theta_cov[off:off + nk]))
            off += nk
        wn = float(np.exp(2 * theta_cov[off])) if self.white_noise else 0.0
        return parts, wn

    def set_hyperparameters(self, theta):
        theta = np.asarray(theta, float)
        self.theta_mean, self.theta_cov = theta[: self.n_mean], theta[self.n_mean:]
        parts, wn = self._parts(self.theta_cov)
        K = sum(orc.kernel_build(k, self.x, th) for k, th in parts)
        K[np.diag_indices(self.n)] += wn
        K[np.diag_indices(self.n)] += self.sig
        self.L = cholesky(K, lower=True)
        r = self.y - self._mean(self.x, self.theta_mean)
        self.alpha = solve_triangular(self.L.T, solve_triangular(self.L, r, lower=True))

    def __call__(self, points):
        p = np.asarray(points, float).reshape(-1, self.d)
        parts, _ = self._parts(self.theta_cov)
        K_qx = sum(orc.kernel_cross(k, p, self.x, th) for k, th in parts)
        a2 = sum(np.exp(th[0]) ** 2 for _, th in parts)  # K_qq[0, 0]: neither noise nor jitter
        mu = K_qx @ self.alpha + self._mean(p, self.theta_mean)
        v = solve_triangular(self.L, K_qx.T, lower=True)
        return mu, np.sqrt(np.abs(a2 - (v**2).sum(axis=0)))


def host_model(tag):
    kinds, wn, mean, _, _, _ = MODELS[tag]
    x, y, e = dataset(tag)
    if len(kinds) == 1 and mean == "const":
        return orc.OracleGp(x, y, e, kernel=kinds[0], white_noise=wn)
    return HostSum(x, y, e, kinds, white_noise=wn, mean=mean)


def samples(model, points, thetas):
    """(means (T, m), variances (T, m), failed (T,)): per row `model.set_hyperparameters` + `model(points)`; a row whose
    matrix is not positive definite is NaN and flagged."""
    thetas = np.atleast_2d(np.asarray(thetas, float))
    mus, vs, bad = [], [], np.zeros(len(thetas), dtype=bool)
    m = None
    for t, th in enumerate(thetas):
        try:
            model.set_hyperparameters(th)
            mu, sd = model(points)
        except np.linalg.LinAlgError:
            bad[t] = True
            mus.append(None)
            vs.append(None)
            continue
        m = len(mu)
        mus.append(np.asarray(mu, float))
        vs.append(np.asarray(sd, float) ** 2)
    nan = np.full(m if m is not None else 1, np.nan)
    return (np.array([nan if v is None else v for v in mus]), np.array([nan if v is None else v for v in vs]), bad)


def normalise(weights, T, bad=None):
    """Weights of the rows that did not fail, divided by their sum (None: equal); zero for the failed rows."""
    w = np.full(T, 1.0 / T) if weights is None else np.asarray(weights, float)
    w = w / w.sum()  # (on the host, as the class does - also for the default)
    if bad is not None:
        w = np.where(bad, 0.0, w)
    return w / w.sum()


def mixture(means, variances, weights=None, bad=None):
    """Two passes (law of total variance): mean = sum w mu, var = sum w (sigma^2 + (mu - mean)^2) over the good rows."""
    T = len(means)
    bad = np.zeros(T, dtype=bool) if bad is None else bad
    w = normalise(weights, T, bad)
    good = ~bad
    mean = (w[good, None] * means[good]).sum(axis=0)
    var = (w[good, None] * (variances[good] + (means[good] - mean[None, :]) ** 2)).sum(axis=0)
    return mean, var


def brute_force_mixture(means, variances, weights=None, bad=None):
    """The moments of the mixture of Gaussians in closed form, E[x^2] - E[x]^2, in longdouble: what T-fold sampling from the
    components would converge to."""
    T = len(means)
    bad = np.zeros(T, dtype=bool) if bad is None else bad
    w = np.asarray(normalise(weights, T, bad), dtype=np.longdouble)
    good = ~bad
    mu = np.asarray(means[good], dtype=np.longdouble)
    s2 = np.asarray(variances[good], dtype=np.longdouble)
    wg = w[good, None]
    e1 = (wg * mu).sum(axis=0)
    e2 = (wg * (s2 + mu * mu)).sum(axis=0)
    return e1, e2 - e1 * e1
