"""
Parametric estimate of a univariate, unimodal PDF from a sample (reference: pdf/unimodal.py:10-171): a heavily modified
Student-t curve with six parameters theta = (x0, s0, ln v, f, k, q), fitted by maximising the sample's log-probability
with Nelder-Mead.

Every sum over the sample runs on the device (csrc/unimodal.hip): `posterior(theta)` is the device sum minus
n_fit log(norm(theta)), and `posterior_batch` scores the 72 starting guesses in one call.  What does not touch the sample
stays on the host, where the CPU tests drive it through the plain functions below: the model curve (a closed form in six
numbers), its normalisation on 128 Chebyshev nodes, the guesses and bounds, the SciPy Nelder-Mead driving with its two
passes, the cdf (a chain of `scipy.integrate.quad` calls) and the moments (Simpson on 1000 points).
"""
from itertools import product

import numpy as np
from numpy import array, atleast_1d, cos, exp, linspace, log, mean, pi, sqrt, tanh, zeros
from scipy.integrate import quad, simpson
from scipy.optimize import minimize

from inference_amd.pdf import _device
from inference_amd.pdf.base import DensityEstimator
from inference_amd.pdf.hdi import sample_hdi


# ---- host logic (plain functions) -----------------------------------------------------------------------------------
def chebyshev_nodes(n_nodes=128, sd=0.2):
    """Axis u and weights w of the quadrature behind `model_norm` (unimodal.py:27-33): Chebyshev nodes t mapped to the
    whole real line by u = t / (1 - t^2), for a curve of scale `sd`."""
    k = linspace(1, n_nodes, n_nodes)
    t = cos(0.5 * pi * ((2 * k - 1) / n_nodes))
    u = t / (1.0 - t**2)
    w = (pi / n_nodes) * (1 + t**2) / (sd * (1 - t**2) ** 1.5)
    return u, w


def log_pdf_model(x, theta):
    """Logarithm of the un-normalised model curve at x (unimodal.py:144-151)."""
    x0, s0, ln_v, f, k, q = theta
    v = exp(ln_v)
    z0 = (x - x0) / s0
    z = z0 * exp(-f * tanh(z0 / k))
    return -(0.5 * (1 + v)) * log(1 + (abs(z) ** q) / v)


def pdf_model(x, theta):
    return exp(log_pdf_model(x, theta))


def model_norm(theta, u, w, sd):
    """Integral of the model curve over the real line (unimodal.py:136-139): the shape at scale `sd` on the nodes,
    rescaled by s0."""
    v = pdf_model(u, [0.0, sd, *theta[2:]])
    return (w * v).sum() * theta[1]


def sample_moments(samples):
    """Mean, standard deviation and skewness of a sample from its raw moments (unimodal.py:95-102)."""
    mu = mean(samples)
    x2 = samples**2
    x3 = x2 * samples
    sig = sqrt(mean(x2) - mu**2)
    skew = (mean(x3) - 3 * mu * sig**2 - mu**3) / sig**3
    return mu, sig, skew


def guesses_and_bounds(sample, fitted_samples):
    """The 72 starting points of the fit and its bounds (unimodal.py:74-93): the moments of the fitted samples, and the
    50 % highest-density interval of the whole sample for x0.  A guess for f (half the skewness, and the skewness) may
    lie outside its bounds (-3, 3); SciPy clips it, with its warning."""
    mu, sigma, skew = sample_moments(fitted_samples)
    lwr, upr = sample_hdi(sample=sample, fraction=0.5)
    bounds = [(lwr, upr), (sigma * 0.1, sigma * 10), (0.0, 5.0), (-3.0, 3.0), (1e-2, 20.0), (1.0, 6.0)]
    x0 = [lwr * (1 - f) + upr * f for f in [0.3, 0.5, 0.7]]
    s0 = [sigma, sigma * 2]
    ln_v = [0.25, 2.0]
    f = [0.5 * skew, skew]
    k = [1.0, 4.0, 8.0]
    q = [2.0]
    return [array(i) for i in product(x0, s0, ln_v, f, k, q)], bounds


def fit(guesses, bounds, skip, objective, use_full_sample=lambda: None):
    """The reference's fit (unimodal.py:40-64) with its requests batched.  `objective(thetas)` returns the log-
    probabilities of a list of parameter vectors: it is called once with all the guesses, then with one vector per
    evaluation of `scipy.optimize.minimize(method="Nelder-Mead", bounds=bounds)` started at the best guess (ties keep
    the order of the guesses).  When skip > 1 the objective so far summed over a reduced sample: `use_full_sample()` is
    called and a second minimisation starts from the first one's result.  A result with success=False is used as it is.
    Returns the last OptimizeResult."""
    cost = [-p for p in objective(guesses)]
    best = sorted(range(len(guesses)), key=cost.__getitem__)[0]

    def cost_func(theta):
        return -objective([theta])[0]

    result = minimize(fun=cost_func, x0=guesses[best], bounds=bounds, method="Nelder-Mead")
    if skip > 1:
        use_full_sample()
        result = minimize(fun=cost_func, x0=result.x, bounds=bounds, method="Nelder-Mead")
    return result


def map_limits(MAP):
    """(lwr_limit, upr_limit) of the fitted curve (unimodal.py:69-72): where the cdf starts, and its counterpart."""
    x0, s0, _, f, _, _ = MAP
    return x0 - s0 * (4 * exp(-f) + 1), x0 + s0 * (4 * exp(f) + 1)


def model_cdf(pdf, lwr_limit, x):
    """The reference's cdf (unimodal.py:113-127) of the curve `pdf`: the points in increasing order, one `quad` per gap.
    The first integral starts at `lwr_limit` and is 0 for a point at or below it, while the later ones integrate the
    true curve - so the cdf of a batch that starts below `lwr_limit` is short of the mass below its smallest point.
    A single point gives a scalar."""
    x = atleast_1d(x)
    order = x.argsort()
    back = order.argsort()
    v = x[order]
    pieces = zeros(x.size)
    if v[0] > lwr_limit:
        pieces[0] = quad(pdf, lwr_limit, v[0])[0]
    for i in range(1, x.size):
        pieces[i] = quad(pdf, v[i - 1], v[i])[0]
    total = pieces.cumsum()[back]
    return total if x.size > 1 else total[0]


def model_moments(pdf, mode, s, f):
    """Mean, variance, skewness and excess kurtosis of the curve `pdf` (unimodal.py:153-171): Simpson's rule on 1000
    points over mode -/+ 5 s max(exp(-/+f), 1)."""
    x = linspace(mode - 5 * max(exp(-f), 1.0) * s, mode + 5 * max(exp(f), 1.0) * s, 1000)
    p = pdf(x)
    mu = simpson(p * x, x=x)
    var = simpson(p * (x - mu) ** 2, x=x)
    skw = simpson(p * (x - mu) ** 3, x=x) / var**1.5
    kur = (simpson(p * (x - mu) ** 4, x=x) / var**2) - 3.0
    return mu, var, skw, kur


# ---- the estimator --------------------------------------------------------------------------------------------------
class UnimodalPdf(DensityEstimator):
    """
    Estimate of a univariate, unimodal PDF from a sample; call it as a function to evaluate the estimate.  A parametric
    method based on a heavily modified Student-t distribution, which is extremely flexible.

    :param sample: 1D array of samples from which to estimate the probability distribution.
    :param device: device index of the sample sums (keyword only; default: that of `inference_amd._lib.Handle`).
    """

    def __init__(self, sample, *, device=None):
        self._setup(sample, device)
        self._density = _device.DeviceUnimodal(self.sample, device=device)  # no CPU fallback: raises without a GPU

        guesses, self.bounds = self.generate_guesses_and_bounds()
        self.min_result = fit(guesses, self.bounds, self.skip, self.posterior_batch, self._use_full_sample)
        self._set_map(self.min_result.x)

    @classmethod
    def from_fit(cls, sample, MAP, *, device=None):
        """The estimate of `sample` with known parameters `MAP` (those of an earlier fit, say): no fit and no device
        call are made; `min_result` is None.  `posterior` uploads the sample when it is first asked for.  This is an
        addition to the reference's surface."""
        self = cls.__new__(cls)
        self._setup(sample, device)
        _, self.bounds = self.generate_guesses_and_bounds()
        self._use_full_sample()
        self.min_result = None
        self._set_map(array(MAP, dtype=float))
        return self

    def _setup(self, sample, device):
        self.sample = array(sample).flatten()
        self.n_samps = self.sample.size
        self.device = device
        self._density = None

        # chebyshev quadrature weights and axes
        self.sd = 0.2
        self.n_nodes = 128
        self.u, self.w = chebyshev_nodes(self.n_nodes, self.sd)

        # the first minimisation uses a slice of the sample, if it is large enough
        self.cutoff = 2000
        self.skip = max(self.n_samps // self.cutoff, 1)
        self.fitted_samples = self.sample[:: self.skip]
        self._stride = self.skip

    def _use_full_sample(self):
        self.fitted_samples = self.sample
        self._stride = 1

    def _set_map(self, MAP):
        self.MAP = MAP
        self.mode = self.MAP[0]
        # normalising constant for the MAP estimate curve
        self.map_lognorm = log(self.norm(self.MAP))
        # bounds for the confidence limits calculation
        self.lwr_limit, self.upr_limit = map_limits(self.MAP)

    def generate_guesses_and_bounds(self):
        return guesses_and_bounds(self.sample, self.fitted_samples)

    @staticmethod
    def sample_moments(samples):
        return sample_moments(samples)

    def __call__(self, x):
        """Estimate of the PDF at the given location(s)."""
        return exp(self.log_pdf_model(x, self.MAP) - self.map_lognorm)

    def cdf(self, x):
        """Estimate of the CDF at the given location(s): an array, or a scalar for a single point."""
        return model_cdf(self.__call__, self.lwr_limit, x)

    def evaluate_model(self, x, theta):
        return self.pdf_model(x, theta) / self.norm(theta)

    def posterior_batch(self, thetas):
        """Log-probability of the fitted samples for every parameter vector of `thetas`: one device call."""
        if self._density is None:
            self._density = _device.DeviceUnimodal(self.sample, device=self.device)
        thetas = [np.asarray(t, dtype=np.float64) for t in thetas]
        sums = self._density.sums(thetas, stride=self._stride)
        return [s - self.fitted_samples.size * log(self.norm(t)) for s, t in zip(sums, thetas)]

    def posterior(self, theta):
        return self.posterior_batch([theta])[0]

    def norm(self, theta):
        return model_norm(theta, self.u, self.w, self.sd)

    def pdf_model(self, x, theta):
        return pdf_model(x, theta)

    def log_pdf_model(self, x, theta):
        return log_pdf_model(x, theta)

    def moments(self):
        """Mean, variance, skewness and excess kurtosis of the estimated PDF."""
        return model_moments(self, self.mode, self.MAP[1], self.MAP[3])
