"""
Gaussian kernel-density estimate of a 2D sample (reference: pdf/kde.py:256-280).

The density at a point is the untruncated sum over every sample, norm * sum_j exp(-((x_j - a) q_x)^2 - ((y_j - b) q_y)^2).
The sums run on the device (csrc/kde2d.hip): a direct sum for scattered points, a direct sum with tile skipping for the
density at the samples themselves, and a factorised matrix product for full grids.  The bandwidths, the normalisation,
the argument handling of `__call__` and the NaN answer of a degenerate sample are host logic, which the CPU tests drive
through the plain functions below and through `KDE2D._raw_sums`.
"""
import numpy as np
from numpy import array, cov, pi, sqrt

from inference_amd.pdf import _device
from inference_amd.pdf import _messages as msg

# ---- host logic (plain functions) -----------------------------------------------------------------------------------
def estimate_bandwidth(x, y):
    """The reference's "very simple bandwidth estimate" (kde.py:277-280): the pair (s_x, s_y) from numpy.cov."""
    S = cov(x, y)
    p = S[0, 1] / sqrt(S[0, 0] * S[1, 1])
    return 1.06 * sqrt(S.diagonal() * (1 - p**2)) / (len(x) ** 0.2)


def scales(n, s_x, s_y):
    """(q_x, q_y, norm) of the reference (kde.py:262-264).  The normalisation divides by sqrt(2 pi) where the 2D
    Gaussian has 2 pi: the reference's densities integrate to sqrt(2 pi), and so do these."""
    q_x = 1.0 / (sqrt(2) * s_x)
    q_y = 1.0 / (sqrt(2) * s_y)
    norm = 1.0 / (n * sqrt(2 * pi) * s_x * s_y)
    return q_x, q_y, norm


def paired_points(x_vals, y_vals):
    """The points of `__call__(x_vals, y_vals)` for two iterables: zip-truncated to the shorter, as two float arrays."""
    pairs = list(zip(x_vals, y_vals))
    a = np.array([p[0] for p in pairs], dtype=np.float64)
    b = np.array([p[1] for p in pairs], dtype=np.float64)
    return a, b


# ---- the estimator --------------------------------------------------------------------------------------------------
class KDE2D:
    """
    Gaussian kernel-density estimate of the PDF of a 2D sample; call it as a function to evaluate the estimate.

    :param x: 1D array of the samples' first coordinate.
    :param y: 1D array of the samples' second coordinate, of the same length (at least 2).
    :param device: device index of the evaluations (keyword only; default: that of `inference_amd._lib.Handle`).

    Only one-dimensional inputs of equal length >= 2 are accepted; anything else raises ValueError (the reference
    broadcasts such inputs, or fails inside NumPy).  Perfectly correlated columns give infinite `q_x`, `q_y` and
    `norm`, as in the reference, and every density is then NaN.  `grid` and `at_samples` are additions of this package.
    """

    def __init__(self, x, y, *, device=None):
        self.x = array(x)
        self.y = array(y)
        self.device = device
        if self.x.ndim != 1 or self.y.ndim != 1 or self.x.size != self.y.size or self.x.size < 2:
            raise ValueError(msg.kde2d_bad_samples(self.x.shape, self.y.shape))
        # very simple bandwidth estimate
        s_x, s_y = self.estimate_bandwidth(self.x, self.y)
        self.q_x, self.q_y, self.norm = scales(len(self.x), s_x, s_y)
        self._density = None if self.degenerate else self._open_device()

    @property
    def degenerate(self) -> bool:
        """True when the scales are not finite and positive (perfectly correlated columns): every density is NaN."""
        q = np.array([self.q_x, self.q_y, self.norm], dtype=np.float64)
        return not bool(np.all(np.isfinite(q) & (q > 0)))

    def _open_device(self):
        return _device.DeviceDensity2D(self.x, self.y, device=self.device)

    def estimate_bandwidth(self, x, y):
        return estimate_bandwidth(x, y)

    # -- raw sums: the only methods that reach the device -----------------------------------------------------------------
    def _raw_sums(self, a, b):
        """sum_j exp(-((x_j - a_i) q_x)^2 - ((y_j - b_i) q_y)^2) for the scattered points (a_i, b_i), one device call."""
        return self._density.sums(a, b, self.q_x, self.q_y)

    def _raw_self_sums(self):
        """The raw sums at every sample (the device skips tiles of samples whose terms cannot change a sum >= 1)."""
        return self._density.self_sums(self.q_x, self.q_y)

    def _raw_grid_sums(self, x_axis, y_axis):
        """The raw sums on the grid of the two axes, shape (len(y_axis), len(x_axis)): the factorised product, which on
        the MI355X beat the direct sum of the grid's points at every size measured (50 x 50 and 200 x 200 cells, 10^5 and
        10^6 samples: 2.6 to 8.7 times, profiles/r08_kde2d.txt)."""
        return self._density.grid_sums(x_axis, y_axis, self.q_x, self.q_y)

    # -- the reference's surface ---------------------------------------------------------------------------------------
    def __call__(self, x_vals, y_vals):
        """A list of densities when both arguments are iterable (paired, truncated to the shorter), else one density."""
        if hasattr(x_vals, "__iter__") and hasattr(y_vals, "__iter__"):
            a, b = paired_points(x_vals, y_vals)
            if self.degenerate:
                return [np.float64(np.nan)] * a.size
            return list(self._raw_sums(a, b) * self.norm) if a.size else []
        return self.density(x_vals, y_vals)

    def density(self, x, y):
        """The estimate at the single point (x, y): two scalars (the reference broadcasts an array against the sample,
        or fails inside NumPy; here that is a ValueError)."""
        if self.degenerate:
            return np.float64(np.nan)
        a = np.array([x], dtype=np.float64).ravel()
        b = np.array([y], dtype=np.float64).ravel()
        if a.size != 1 or b.size != 1:
            raise ValueError(msg.kde2d_bad_point(np.shape(x), np.shape(y)))
        return (self._raw_sums(a, b) * self.norm)[0]

    # -- additions -------------------------------------------------------------------------------------------------------
    def grid(self, x_axis, y_axis):
        """(Not in the reference.)  The estimate on the grid of two axes as an array of shape (len(y_axis), len(x_axis)):
        array(pdf(X.flatten(), Y.flatten())).reshape(...) of X, Y = meshgrid(x_axis, y_axis)."""
        xa = np.asarray(x_axis, dtype=np.float64)
        ya = np.asarray(y_axis, dtype=np.float64)
        if xa.ndim != 1 or ya.ndim != 1:
            raise ValueError(msg.kde2d_bad_axes(xa.shape, ya.shape))
        if self.degenerate:
            return np.full((ya.size, xa.size), np.nan)
        if xa.size == 0 or ya.size == 0:
            return np.empty((ya.size, xa.size))
        return self._raw_grid_sums(xa, ya) * self.norm

    def at_samples(self):
        """(Not in the reference.)  The estimate at every sample: array(pdf(x, y)) of the sample columns."""
        if self.degenerate:
            return np.full(self.x.size, np.nan)
        return self._raw_self_sums() * self.norm
