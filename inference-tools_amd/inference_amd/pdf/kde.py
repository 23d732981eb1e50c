"""
Gaussian kernel-density estimate of a 1D sample (reference: pdf/kde.py:13-233 and its BinaryTree, :283-325).

The pdf and the cdf are truncated sums, as in the reference: the axis between the smallest and the largest sample is cut
into 2^k equal regions, and a point sums only over the samples within 4 h of its region's midpoint (its slice); the cdf
adds lo / n for the samples below the slice.  The slice sums and the cross-validation log-probabilities run on the
device (csrc/kde.hip); the region table, the region lookup, the bandwidth grid search and the SciPy searches for the
mode and the interval run on the host, where the CPU tests drive them through the plain functions below.
"""
import numpy as np
from numpy import arange, argmax, argsort, array, atleast_1d, exp, linspace, log, pi, searchsorted, sort, sqrt, std
from numpy.random import random
from scipy.integrate import simpson
from scipy.optimize import minimize_scalar

from inference_amd.pdf import _device
from inference_amd.pdf import _messages as msg
from inference_amd.pdf.base import DensityEstimator
from inference_amd.pdf.hdi import sample_hdi


# ---- host logic (plain functions) -----------------------------------------------------------------------------------
def rule_of_thumb_bandwidth(sorted_sample) -> float:
    """The simple estimate, which assumes a distribution close to a Gaussian (kde.py:135-137)."""
    return 1.06 * std(sorted_sample) / (sorted_sample.size**0.2)


def region_table(sorted_sample, h):
    """Regions of the reference (kde.py:76-91, BinaryTree.__init__ :293-299) for bandwidth h:
    (layers, edges, regions, lwr_inds, upr_inds).  Region r covers the samples [lwr_inds[r], upr_inds[r]).  A bandwidth
    of inf raises OverflowError, as in the reference."""
    s = sorted_sample
    cutoff = h * 4
    layers = int(log((s[-1] - s[0]) / h) / log(2)) + 1
    mids = linspace(s[0], s[-1], 2**layers + 1)
    mids = 0.5 * (mids[1:] + mids[:-1])
    lwr_inds = searchsorted(s, mids - cutoff)
    upr_inds = searchsorted(s, mids + cutoff)
    edges = linspace(s[0], s[-1], 2**layers + 1)
    regions = arange(-1, edges.size)
    regions[0] = 0
    regions[-1] = edges.size - 2
    return layers, edges, regions, lwr_inds, upr_inds


def region_of(edges, regions, x):
    """Region of every point (BinaryTree.region_groups, kde.py:301-307): points below the first edge go to region 0,
    points above the last to the last region, a point exactly on an interior edge to the region on its left."""
    return regions[searchsorted(edges, x)]


def cv_subsample(sorted_sample, max_cv_samples):
    """The cross-validation sample (kde.py:144-149): the whole sample, or a random subset of max_cv_samples drawn with
    the legacy global generator, so that seeded runs pick the same subset and leave the generator in the same state."""
    if len(sorted_sample) > max_cv_samples:
        scrambler = argsort(random(size=len(sorted_sample)))
        return (sorted_sample[scrambler])[:max_cv_samples]
    return sorted_sample


def cv_bandwidth_search(initial_h, objective):
    """The reference's grid search over log-bandwidth (kde.py:151-193), with its requests batched: objective(widths)
    returns the log-probabilities of a list of widths, and is called with 5 widths first, then 1 per extension of the
    grid and 2 per refinement round.  The grid is centred on `initial_h` taken as a LOG-bandwidth (the reference passes
    the linear rule-of-thumb h); a maximum at the left edge makes the refinement read log_h[-1], one at the right edge
    raises IndexError - both as in the reference."""
    dh = 0.5
    log_h = [initial_h + m * dh for m in (-2, -1, 0, 1, 2)]
    log_p = list(objective([exp(h) for h in log_h]))

    # if the maximum log-probability is at the edge of the grid, extend it
    for i in range(5):
        max_ind = argmax(log_p)
        if 0 < max_ind < len(log_h) - 1:
            break
        if max_ind == 0:
            new_h = log_h[0] - dh
            (new_lp,) = objective([exp(new_h)])
            log_h.insert(0, new_h)
            log_p.insert(0, new_lp)
        else:
            new_h = log_h[-1] + dh
            (new_lp,) = objective([exp(new_h)])
            log_h.append(new_h)
            log_p.append(new_lp)

    # recursive refinement around the maximum, assuming a single maximum
    for refine in range(6):
        max_ind = int(argmax(log_p))
        lwr_h = 0.5 * (log_h[max_ind - 1] + log_h[max_ind])
        upr_h = 0.5 * (log_h[max_ind] + log_h[max_ind + 1])
        lwr_lp, upr_lp = objective([exp(lwr_h), exp(upr_h)])
        log_h.insert(max_ind, lwr_h)
        log_p.insert(max_ind, lwr_lp)
        log_h.insert(max_ind + 2, upr_h)
        log_p.insert(max_ind + 2, upr_lp)

    return exp(log_h[argmax(log_p)])


# ---- the estimator --------------------------------------------------------------------------------------------------
class GaussianKDE(DensityEstimator):
    """
    Gaussian kernel-density estimate of the PDF of a 1D sample; call it as a function to evaluate the estimate.

    :param sample: 1D array of samples from which to estimate the probability distribution.
    :param float bandwidth: Width of the Gaussian kernels. If not specified, it is estimated from the sample.
    :param bool cross_validation: Select the bandwidth by maximising the leave-one-out cross-validation
        log-probability instead of using the simple rule of thumb.
    :param int max_cv_samples: The cross-validation uses a random sub-sample of this size when the sample is larger.
    :param device: device index of the evaluations (keyword only; default: that of `inference_amd._lib.Handle`).
    """

    def __init__(self, sample, bandwidth: float = None, cross_validation: bool = False, max_cv_samples=5000, *,
                 device=None):
        self.sample = sort(array(sample).flatten())  # sorted array of the samples
        self.max_cvs = max_cv_samples
        self.device = device

        if self.sample.size < 3:
            raise ValueError(msg.kde_too_few_samples())

        if bandwidth is None:
            self.h = self.simple_bandwidth_estimator()
            if cross_validation:
                self.h = self.cross_validation_bandwidth_estimator(self.h)
        else:
            self.h = bandwidth

        self.norm = 1.0 / (len(self.sample) * sqrt(2 * pi) * self.h)
        self.cutoff = self.h * 4
        self.q = 1.0 / (sqrt(2) * self.h)
        self.lwr_limit = self.sample[0] - self.cutoff * 0.5
        self.upr_limit = self.sample[-1] + self.cutoff * 0.5

        self.layers, self.edges, self.regions, lwr_inds, upr_inds = region_table(self.sample, self.h)
        self.lwr_inds, self.upr_inds = lwr_inds, upr_inds
        self.cdf_offsets = lwr_inds / self.sample.size
        self._density = _device.DeviceDensity(self.sample, lwr_inds, upr_inds, device=device)

        # the mode of the pdf, located when the estimate is created
        self.mode = self.locate_mode()

    def _sums(self, x, pdf, cdf):
        x = atleast_1d(np.asarray(x, dtype=np.float64)).ravel()
        r = region_of(self.edges, self.regions, x)
        ps, cs = self._density.sums(x, r, self.q, pdf=pdf, cdf=cdf)
        return r, ps, cs

    def __call__(self, x):
        """Estimate of the PDF at the given location(s): an array, or a scalar for a single point."""
        _, ps, _ = self._sums(x, True, False)
        pdf = ps * self.norm
        return pdf if pdf.size > 1 else pdf[0]

    def cdf(self, x):
        """Estimate of the CDF at the given location(s): an array, or a scalar for a single point."""
        r, _, cs = self._sums(x, False, True)
        cdf = (0.5 / self.sample.size) * cs + self.cdf_offsets[r]
        return cdf if cdf.size > 1 else cdf[0]

    def _pdf_and_cdf(self, x):
        """pdf and cdf at the same points from one device call (the values of __call__ and cdf)."""
        r, ps, cs = self._sums(x, True, True)
        return ps * self.norm, (0.5 / self.sample.size) * cs + self.cdf_offsets[r]

    def simple_bandwidth_estimator(self):
        return rule_of_thumb_bandwidth(self.sample)

    def cross_validation_bandwidth_estimator(self, initial_h: float) -> float:
        """Bandwidth that maximises the leave-one-out cross-validation log-probability (kde.py:139-193)."""
        samples = cv_subsample(self.sample, self.max_cvs)
        return cv_bandwidth_search(initial_h, lambda widths: self.cross_validation_logprob(samples, widths))

    def cross_validation_logprob(self, samples, width, c=0.99):
        """Leave-one-out log-probability of `samples` for one width (a float) or several (a sequence)."""
        lp = _device.cv_logprob(samples, atleast_1d(width), c=c, device=self.device)
        return lp if np.ndim(width) else lp[0]

    def locate_mode(self):
        # with enough samples the 20 % HDI bounds the search, else the whole range of the sample
        if self.sample.size > 50:
            lwr, upr = sample_hdi(self.sample, 0.2)
        else:
            lwr, upr = self.sample[0], self.sample[-1]
        result = minimize_scalar(lambda x: -self(x), bounds=[lwr, upr], method="bounded")
        return result.x

    def moments(self):
        """Mean, variance, skewness and excess kurtosis of the estimated PDF (not of the sample values)."""
        N = int(5 * (self.upr_limit - self.lwr_limit) / self.h)
        x = linspace(self.lwr_limit, self.upr_limit, N)
        p = self(x)

        mu = simpson(p * x, x=x)
        dx = x - mu
        I = p * dx**2  # noqa: E741
        var = simpson(I, x=x)
        I *= dx
        skw = simpson(I, x=x) / var**1.5
        I *= dx
        kur = (simpson(I, x=x) / var**2) - 3.0
        return mu, var, skw, kur
