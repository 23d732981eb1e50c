"""Highest-density interval of a sample (reference: pdf/hdi.py:6-105).  Host-only: a sort and one pass."""
from typing import Sequence
from warnings import warn

from numpy import array, expand_dims, ndarray, take_along_axis, zeros

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
