"""Highest-density interval of a sample (reference: pdf/hdi.py:6-105).  `sample_hdi` is the host function, a sort and
one pass; `sample_hdi_batch` answers several fractions for every column of a sample in one device call (csrc/hdi.hip)."""
import warnings
from typing import Sequence
from warnings import warn

from numpy import array, asarray, empty, expand_dims, float64, ndarray, take_along_axis, zeros

from inference_amd.pdf import _device
from inference_amd.pdf import _messages as msg


def sample_hdi(sample: ndarray, fraction: float) -> ndarray:
    """
    Estimate the highest-density interval(s) for a given sample: the shortest interval which contains a chosen
    fraction of the elements.  A 2D sample of shape ``(m, n)`` gives the ``n`` intervals of its columns as an array of
    shape ``(2, n)``; a 1D sample gives ``[lower, upper]``.
    """
    if not 0.0 < fraction < 1.0:
        raise ValueError(msg.hdi_bad_fraction(fraction))

    if isinstance(sample, ndarray):
        s = sample.copy()
    elif isinstance(sample, Sequence):
        s = array(sample)
    else:
        raise ValueError(msg.hdi_bad_type(type(sample)))

    if s.ndim > 2 or s.ndim == 0:
        raise ValueError(msg.hdi_bad_ndim(s.ndim))

    if s.ndim == 1:
        s.resize([s.size, 1])

    n_samples, n_intervals = s.shape
    L = int(fraction * n_samples)

    if n_samples < 2:
        raise ValueError(msg.hdi_too_short())

    if n_samples <= L:
        warn(msg.hdi_insufficient())
    elif n_samples - L < 20:
        warn(msg.hdi_inaccurate())

    s.sort(axis=0)
    hdi = zeros([2, n_intervals])
    if n_samples > L:
        # the optimal single interval: the narrowest window of L + 1 sorted samples
        widths = s[L:, :] - s[: n_samples - L, :]
        i = expand_dims(widths.argmin(axis=0), axis=0)
        hdi[0, :] = take_along_axis(s, i, 0).squeeze()
        hdi[1, :] = take_along_axis(s, i + L, 0).squeeze()
    else:
        hdi[0, :] = s[0, :]
        hdi[1, :] = s[-1, :]
    return hdi.squeeze()


def sample_hdi_batch(sample, fractions, *, device=None) -> ndarray:
    """
    The highest-density intervals of `sample` for every fraction of `fractions`, in one device call: what
    ``[sample_hdi(sample, f) for f in fractions]`` returns, stacked.  A 2D sample of shape ``(n, m)`` gives an array of
    shape ``(len(fractions), 2, m)``, a 1D sample one of shape ``(len(fractions), 2)``.

    The checks, their texts and the warnings are `sample_hdi`'s, raised once per fraction before the device is touched,
    and the window length ``int(fraction * n)`` is taken here, in Python, as the reference takes it: the device sorts
    each column once and is given window lengths, never a fraction.  The sample is converted to float64: integers stay
    exact, and a float32 sample is widened, whereas the reference subtracts in float32 (the bounds are elements of the
    sample either way; which of two nearly equal windows wins can differ).  A 2D sample is read in place in C order or
    as the transpose of a C-ordered array.  Columns that hold a NaN or an infinity are recomputed by `sample_hdi` on
    the host, which gives NumPy's answer for them (NaN sorts last, argmin returns the first NaN).  There is no host
    route by size: without a GPU the call raises `GpmiUnavailable`.
    """
    fractions = [f for f in fractions]
    for fraction in fractions:
        if not 0.0 < fraction < 1.0:
            raise ValueError(msg.hdi_bad_fraction(fraction))

    if isinstance(sample, ndarray):
        s = sample
    elif isinstance(sample, Sequence):
        s = array(sample)
    else:
        raise ValueError(msg.hdi_bad_type(type(sample)))

    if s.ndim > 2 or s.ndim == 0:
        raise ValueError(msg.hdi_bad_ndim(s.ndim))

    one_d = s.ndim == 1
    s = asarray(s, dtype=float64)
    if one_d:
        s = s.reshape(s.size, 1)

    n_samples, n_intervals = s.shape
    if n_samples < 2:
        raise ValueError(msg.hdi_too_short())

    Ls = [int(fraction * n_samples) for fraction in fractions]
    for L in Ls:
        if n_samples <= L:
            warn(msg.hdi_insufficient())
        elif n_samples - L < 20:
            warn(msg.hdi_inaccurate())

    if not fractions:
        hdi = empty([0, 2, n_intervals])
    else:
        hdi, flags = _device.hdi_columns(s, Ls, device=device)
        for c in flags.nonzero()[0]:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for k, fraction in enumerate(fractions):
                    hdi[k, :, c] = sample_hdi(s[:, c], fraction)
    return hdi[:, :, 0] if one_d else hdi
