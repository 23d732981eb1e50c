"""
Likelihoods of `GeneralisedGpRegressor`: log-concave p(y_i | f_i) of one latent value per observation.

Each class carries its per-point data `aux`, checks the domain of `y`, and evaluates on the host - in the overflow-safe
forms the device kernel uses (csrc/generalised.hip) - the log-likelihood and its first three derivatives by f:

    g = d log p / df,    W = -d^2 log p / df^2 >= 0,    d3 = d^3 log p / df^3

`Logistic` is the reference's `LogisticLikelihood` (inference/likelihoods.py) with the model prediction equal to f; the
reference's `CauchyLikelihood` (and Student-t) are not log-concave - W changes sign - and are not served.
"""
import numpy as np
from scipy.special import gammaln

from inference_amd import _lib


def _exp_neg_abs(t):
    return np.exp(-np.abs(t))


def softplus(t):
    """ln(1 + e^t) = max(t, 0) + log1p(exp(-|t|)): finite for every finite t."""
    t = np.asarray(t, dtype=float)
    return np.maximum(t, 0.0) + np.log1p(_exp_neg_abs(t))


def logistic_parts(t):
    """(sigma(t), sigma (1 - sigma), 1 - 2 sigma) from e = exp(-|t|), without cancellation in either tail."""
    t = np.asarray(t, dtype=float)
    e = _exp_neg_abs(t)
    r = 1.0 / (1.0 + e)
    sig = np.where(t >= 0, r, e * r)
    h = (1.0 - e) * r
    return sig, e * r * r, np.where(t >= 0, -h, h)


class Likelihood:
    """Base class: `aux` (N,), `code` (the device's id), `check(y)`, `log_prob`, `derivatives`, `default_offset`,
    `latent_proxy` (rough latent values: the scale the kernel's amplitude bounds are estimated from)."""

    code = None
    name = "Likelihood"

    def bind(self, n: int):
        """The per-point data as an (n,) array (scalars are broadcast); checks its domain."""
        raise NotImplementedError

    def check(self, y: np.ndarray):
        raise NotImplementedError

    def log_prob(self, y, f, aux):
        raise NotImplementedError

    def derivatives(self, y, f, aux):
        """(g, W, d3)"""
        raise NotImplementedError

    def _broadcast(self, value, n, label):
        a = np.asarray(value, dtype=float)
        if a.ndim == 0:
            a = np.full(n, float(a))
        a = a.squeeze() if a.ndim > 1 else a
        if a.shape != (n,):
            raise ValueError(f"[ {self.name} error ] '{label}' must be a scalar or an array of shape ({n},), "
                             f"but has shape {np.shape(value)}.")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"[ {self.name} error ] '{label}' holds values that are not finite.")
        return np.ascontiguousarray(a)


class Logistic(Likelihood):
    """Robust regression: y_i = f_i + logistic noise of standard deviation sigma_i (heavier tails than a Gaussian).
    log p = z - 2 softplus(z) - ln s with z = (y - f) / s and s = sigma sqrt(3) / pi."""

    code = _lib.GGP_LOGISTIC
    name = "Logistic"

    def __init__(self, sigma=1.0):
        self.sigma = sigma

    def bind(self, n):
        sig = self._broadcast(self.sigma, n, "sigma")
        if np.any(sig <= 0):
            raise ValueError("[ Logistic error ] 'sigma' must be positive.")
        self.noise_sigma = sig
        return sig * (np.sqrt(3.0) / np.pi)

    def check(self, y):
        if not np.all(np.isfinite(y)):
            raise ValueError("[ Logistic error ] 'y' holds values that are not finite.")

    def log_prob(self, y, f, aux):
        z = (y - f) / aux
        return z - 2.0 * softplus(z) - np.log(aux)

    def derivatives(self, y, f, aux):
        _, s1, m2 = logistic_parts((y - f) / aux)
        return -m2 / aux, 2.0 * s1 / aux**2, 2.0 * s1 * m2 / aux**3

    def default_offset(self, y, aux):
        return float(np.mean(y))

    def latent_proxy(self, y, aux):
        return y


class Poisson(Likelihood):
    """Counts with a log link: y_i ~ Poisson(e_i exp(f_i)), e_i the exposure (integration time, area, ...)."""

    code = _lib.GGP_POISSON
    name = "Poisson"

    def __init__(self, exposure=1.0):
        self.exposure = exposure

    def bind(self, n):
        e = self._broadcast(self.exposure, n, "exposure")
        if np.any(e <= 0):
            raise ValueError("[ Poisson error ] 'exposure' must be positive.")
        return e

    def check(self, y):
        if not np.all(np.isfinite(y)) or np.any(y < 0) or np.any(y != np.floor(y)):
            raise ValueError("[ Poisson error ] 'y' must hold counts: integers >= 0.")

    def log_prob(self, y, f, aux):
        return y * (f + np.log(aux)) - aux * np.exp(f) - gammaln(y + 1.0)

    def derivatives(self, y, f, aux):
        mu = aux * np.exp(f)
        return y - mu, mu, -mu

    def default_offset(self, y, aux):
        return float(np.log(max(np.mean(y / aux), 1e-3)))

    def latent_proxy(self, y, aux):
        return np.log((y + 0.5) / aux)


class Binomial(Likelihood):
    """k successes of n trials with a logit link: y_i ~ Binomial(n_i, sigma(f_i)); trials=1 is hit-or-miss data."""

    code = _lib.GGP_BINOMIAL
    name = "Binomial"

    def __init__(self, trials=1):
        self.trials = trials

    def bind(self, n):
        t = self._broadcast(self.trials, n, "trials")
        if np.any(t < 1) or np.any(t != np.floor(t)):
            raise ValueError("[ Binomial error ] 'trials' must hold integers >= 1.")
        self._trials = t
        return t

    def check(self, y):
        if not np.all(np.isfinite(y)) or np.any(y < 0) or np.any(y != np.floor(y)) or np.any(y > self._trials):
            raise ValueError("[ Binomial error ] 'y' must hold integers in 0 .. trials.")

    def log_prob(self, y, f, aux):
        # y f - n softplus(f) = -(y softplus(-f) + (n - y) softplus(f)): every term of one sign, nothing cancels
        return (gammaln(aux + 1.0) - gammaln(y + 1.0) - gammaln(aux - y + 1.0)) - (y * softplus(-f) + (aux - y) * softplus(f))

    def derivatives(self, y, f, aux):
        sig, s1, m2 = logistic_parts(f)
        return y - aux * sig, aux * s1, -aux * s1 * m2

    def default_offset(self, y, aux):
        return 0.0

    def latent_proxy(self, y, aux):
        p = (y + 0.5) / (aux + 1.0)
        return np.log(p / (1.0 - p))
