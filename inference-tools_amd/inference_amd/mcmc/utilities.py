"""Chain diagnostics (reference: mcmc/utilities.py:83-95) and parameter bounds (:98-162).  `effective_sample_size` is
the host function with the reference's exact semantics; `effective_sample_size_batch` answers every column of a sample
in one device call (csrc/acf.hip); `sample_covariance` is numpy.cov of a tall sample on the device (csrc/cov.hip), the
covariance that `PcaChain` takes its directions from.  `Bounds` holds the box a `HamiltonianChain` is reflected into."""
from numpy import array, asarray, cov as np_cov, divmod as np_divmod, empty, float64, int64, ndarray
from numpy.fft import irfft, rfft

from inference_amd.pdf import _device
from inference_amd.pdf import _messages as msg


def effective_sample_size(x: ndarray) -> int:
    """
    Estimate of the effective sample size of a 1D sample: its length over the sum of the normalised autocorrelation
    up to the first negative lag.

    The autocorrelation is the inverse real FFT of the power spectrum, of which the first half is kept.  For an odd
    length the inverse transform returns one point fewer than the sample has (numpy's default output length), as in
    the reference, and that is kept: the integer is the reference's for every length.  A sample without a negative
    lag in that half (two points, a constant sample, one holding a NaN) raises the reference's ``IndexError``.
    """
    x = asarray(x)
    power = abs(rfft(x - x.mean())) ** 2
    acf = irfft(power)
    acf = acf[: acf.size // 2]
    if acf[0] < 0.0:
        raise ValueError(msg.ess_negative_first())
    cut = (acf < 0.0).argmax()  # 0 when no lag is negative: nothing is left, and acf[0] below raises IndexError
    acf = acf[:cut]
    return int(x.size / (acf.sum() / acf[0]))


def effective_sample_size_batch(sample, *, device=None, details=False):
    """
    The effective sample size of every column of `sample`, in one device call.  A 2D sample of shape ``(n, p)`` gives an
    int64 array of shape ``(p,)``, a 1D sample one of shape ``(1,)``.  With ``details=True`` the return value is
    ``(ess, f0, sum, cut)``: the zero-lag autocorrelation, its sum up to the first negative lag and that lag, per column.

    The device sums the circular autocorrelation of length n directly, lag by lag, until a column meets its first
    negative lag, and the integer is finished here as ``int(n / (sum / f0))``.  For even n that is the number
    `effective_sample_size` gives; for odd n the host function follows the reference's shorter inverse transform and
    this one does not (the two can differ by one or so for short samples).  The sample is converted to float64 (a
    float32 sample is widened).  A column without an answer - one that holds a NaN or an infinity, or has no negative
    lag below ``n // 2`` - is handed to `effective_sample_size`, which raises what the reference raises for it.  There
    is no host route by size: without a GPU the call raises `GpmiUnavailable`.
    """
    s = asarray(sample, dtype=float64)
    if s.ndim == 1:
        s = s.reshape(s.size, 1)
    if s.ndim != 2:
        raise ValueError("effective_sample_size_batch takes a one- or two-dimensional sample")
    n, p = s.shape
    f0, total, cut, flags = _device.acf_columns(s, device=device)
    ess = empty(p, dtype=int64)
    for c in range(p):
        if flags[c]:
            ess[c] = effective_sample_size(s[:, c])
        else:
            ess[c] = int(n / (total[c] / f0[c]))
    return (ess, f0, total, cut) if details else ess


def sample_covariance(sample, *, device=None, return_mean=False):
    """
    The covariance matrix of the columns of `sample`, ``numpy.cov(sample.T)``, in one device call.  A 2D sample of shape
    ``(n, p)`` gives a float64 array of shape ``(p, p)``, a 1D sample (one column) one of shape ``(1, 1)``; with
    ``return_mean=True`` the return value is ``(cov, mean)`` with the column means, shape ``(p,)``.

    The device takes the means first and then the products of the centred columns on the fp64 matrix cores, in an order
    of summation that depends on n alone: the entry of two columns has the same bits whatever else is in the sample, the
    matrix is symmetric bit for bit, and integer-valued data with an exact mean and sums below 2^53 gives NumPy's bits.
    The sample is converted to float64 (a float32 sample is widened) and read in place when it is dense in either order.
    It takes at least two rows and at most 512 columns.  If any column holds a NaN or an infinity the whole answer is
    NumPy's, computed on the host.  There is no host route by size: without a GPU the call raises `GpmiUnavailable`.
    """
    s = asarray(sample, dtype=float64)
    if s.ndim == 1:
        s = s.reshape(s.size, 1)
    if s.ndim != 2:
        raise ValueError("sample_covariance takes a one- or two-dimensional sample")
    n, p = s.shape
    if n < 2:
        raise ValueError(f"sample_covariance needs at least two rows, the sample has {n}")
    if p < 1 or p > _device.COV_MAX_COLUMNS:
        raise ValueError(f"sample_covariance takes 1 to {_device.COV_MAX_COLUMNS} columns, the sample has {p}")
    mean, cov, flags = _device.cov_columns(s, device=device)
    if flags.any():
        cov = np_cov(s.T).reshape(p, p)
        mean = s.mean(axis=0)
    return (cov, mean) if return_mean else cov


class Bounds:
    """
    Lower and upper limits of every parameter, and the reflection of points that left them.

    :param lower: one-dimensional array of lower limits.
    :param upper: one-dimensional array of upper limits, each above its lower limit.
    :param error_source: the name that the error messages carry.
    """

    def __init__(self, lower, upper, error_source="Bounds"):
        self.lower = lower if isinstance(lower, ndarray) else array(lower).squeeze()
        self.upper = upper if isinstance(upper, ndarray) else array(upper).squeeze()
        if self.lower.ndim > 1 or self.upper.ndim > 1:
            raise ValueError(msg.bounds_not_1d(error_source, self.lower.ndim, self.upper.ndim))
        if self.lower.size != self.upper.size:
            raise ValueError(msg.bounds_sizes(error_source, self.lower.size, self.upper.size))
        if (self.lower >= self.upper).any():
            raise ValueError(msg.bounds_order(error_source))
        self.width = self.upper - self.lower
        self.n_bounds = self.width.size

    def validate_start_point(self, start: ndarray, error_source="Bounds"):
        if self.n_bounds != start.size:
            raise ValueError(msg.bounds_start_size(error_source, start.size, self.n_bounds))
        if not self.inside(start):
            raise ValueError(msg.bounds_start_outside(error_source))

    def _fold(self, theta):
        """A triangle wave of period 2 width: the point after as many reflections as it takes, and the sign (+1 or -1)
        that the reflections leave on the velocity along each axis."""
        bounces, inside = np_divmod(theta - self.lower, self.width)
        odd = bounces % 2
        sign = 1 - 2 * odd
        return self.lower + sign * inside + odd * self.width, sign

    def reflect(self, theta: ndarray) -> ndarray:
        return self._fold(theta)[0]

    def reflect_momenta(self, theta: ndarray):
        return self._fold(theta)

    def inside(self, theta: ndarray) -> bool:
        return ((theta >= self.lower) & (theta <= self.upper)).all()
