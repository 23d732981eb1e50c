"""
Dense data-error covariances (`GpRegressor(..., y_cov=Y)`) shared by tests/golden/make_golden_ycov.py and the y_cov tests.

Both kinds are symmetric bit for bit, as the constructor demands (`Y == Y.T` exactly, regression.py:383):
  (a) `correlated_cov`  an exponential correlation over random "times" t plus a diagonal share, scaled by s_i s_j.  The
      product s_i s_j is formed first: s_i C_ij s_j in that order is not symmetric in floating point.  The fixture stores
      this matrix itself.
  (b) `kms_cov`         a permuted Kac-Murdock-Szego matrix (s_i s_j) 2^-|p_i - p_j| with s_i = 2^-4 (1 + (i mod 7) / 8).
      Every operation is exact or correctly rounded, so any machine rebuilds it bit for bit from the permutation p; the
      fixture stores p and a few probe entries.  Its large entries lie far from the diagonal: a kernel that adds Y only
      near the diagonal drops most of it.
"""
import numpy as np


def correlated_cov(t, s, tau=0.02):
    """Kind (a): Y = (s s^T) o C,  C = 0.5 exp(-|t_i - t_j| / tau) + 0.5 I."""
    t = np.asarray(t, dtype=float)
    s = np.asarray(s, dtype=float)
    C = 0.5 * np.exp(-np.abs(t[:, None] - t[None, :]) / tau)
    C[np.diag_indices_from(C)] += 0.5
    return (s[:, None] * s[None, :]) * C


def correlated_cov_inputs(rng, n):
    """Random times in [0, 1) and scales s ~ 0.05 for `correlated_cov`."""
    return rng.uniform(0, 1, n), 0.05 * (1.0 + 0.2 * rng.uniform(size=n))


def kms_scales(n):
    return 0.0625 * (1.0 + (np.arange(n) % 7) / 8.0)


def kms_cov(p, s=None):
    """Kind (b): Y_ij = (s_i s_j) 2^-|p_i - p_j| for a permutation p (default scales `kms_scales`)."""
    p = np.asarray(p, dtype=np.int64)
    s = kms_scales(p.size) if s is None else np.asarray(s, dtype=float)
    return (s[:, None] * s[None, :]) * np.ldexp(1.0, -np.abs(p[:, None] - p[None, :]))


def kms_probes(p, rng, count=64):
    """(count, 2) index pairs into kms_cov(p): half of them at random, half where |p_i - p_j| <= 8 (the large entries)."""
    n = len(p)
    inv = np.argsort(p)
    i = rng.integers(0, n, count)
    j = rng.integers(0, n, count)
    half = count // 2
    near = np.clip(p[i[half:]] + rng.integers(-8, 9, count - half), 0, n - 1)
    j[half:] = inv[near]
    return np.stack([i, j], axis=1)
