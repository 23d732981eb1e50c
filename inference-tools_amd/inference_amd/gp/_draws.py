"""
Argument handling shared by `GpRegressor.sample_posterior` and `GpLinearInverter.sample_posterior` (an addition: the
reference draws with numpy.random.multivariate_normal on the output of build_posterior / calculate_posterior).
"""
import numpy as np
from numpy.linalg import LinAlgError


def draw_arguments(owner, n_points, n_draws, seed, z, jitter, first_draw):
    """Checked (n_draws, seed, z, jitter, first_draw) of a `sample_posterior` call at `n_points` points.
    `z` (the caller's normals) excludes `seed` and a non-zero `first_draw`; with neither `z` nor `seed`, 64 bits from
    numpy.random.SeedSequence() seed the generator - the seed returned is the one to repeat the draw with."""
    n_draws, first_draw, jitter = int(n_draws), int(first_draw), float(jitter)
    if n_draws < 1:
        raise ValueError(f"[ {owner}.sample_posterior ] n_draws must be at least 1, got {n_draws}")
    if first_draw < 0:
        raise ValueError(f"[ {owner}.sample_posterior ] first_draw must not be negative, got {first_draw}")
    if not (np.isfinite(jitter) and jitter >= 0.0):
        raise ValueError(f"[ {owner}.sample_posterior ] jitter must be finite and not negative, got {jitter}")
    if z is not None:
        if seed is not None or first_draw != 0:
            raise ValueError(f"[ {owner}.sample_posterior ] 'z' holds the normal variates themselves: it cannot be "
                             "combined with 'seed' or a non-zero 'first_draw'")
        z = np.ascontiguousarray(z, dtype=float)
        if z.shape != (n_draws, n_points):
            raise ValueError(f"[ {owner}.sample_posterior ] 'z' must have shape (n_draws, M) = ({n_draws}, {n_points}), "
                             f"got {z.shape}")
        return n_draws, None, z, jitter, 0
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    return n_draws, int(seed), None, jitter, first_draw


def raise_if_not_positive_definite(owner, info, jitter, eps):
    if info != 0:
        raise LinAlgError(f"[ {owner}.sample_posterior ] the posterior covariance + eps I is not positive definite: leading "
                          f"minor of order {info} (jitter = {jitter:g}, eps = jitter * max diag = {eps:g}); "
                          "a larger 'jitter' may help")
