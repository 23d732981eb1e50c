"""Host-side checks of the hyper-parameter-marginalised prediction (no device): the host reference of
tests/predict_host.py against the closed-form moments of the mixture, the argument checks of `predict_samples` /
`predict_marginalised`, which run before anything touches the device, and the rule that nothing is computed without one."""
import numpy as np
import pytest

import predict_host as ph


def _case(seed):
    """T Gaussian components at m points: means around offsets up to 10, variances in [0.01, 1], random weights, and in
    every other case one failed row."""
    rng = np.random.default_rng(1000 + seed)
    T, m = int(rng.integers(1, 40)), int(rng.integers(1, 9))
    means = rng.normal(size=(T, m)) + rng.uniform(-10, 10, m)[None, :]
    variances = rng.uniform(0.01, 1.0, (T, m))
    weights = None if seed % 3 == 0 else rng.uniform(0.0, 1.0, T) + 1e-3
    bad = np.zeros(T, dtype=bool)
    if seed % 2 and T > 1:
        bad[int(rng.integers(0, T))] = True
        means[bad], variances[bad] = np.nan, np.nan
    return means, variances, weights, bad


@pytest.mark.parametrize("seed", range(10))
def test_host_mixture_against_closed_form_moments(seed):
    """Two passes in float64 against E[x^2] - E[x]^2 in longdouble.  |mean|^2 / var stays below 1e5 here, so the closed
    form loses at most 1e5 x 2^-63 = 1e-14 of the variance to its cancellation; the two passes sum at most 40 terms
    (40 x 2^-53 = 5e-15).  Bound: 1e-12."""
    means, variances, weights, bad = _case(seed)
    mean, var = ph.mixture(means, variances, weights, bad)
    bmean, bvar = ph.brute_force_mixture(means, variances, weights, bad)
    assert np.isfinite(mean).all() and np.isfinite(var).all() and (var > 0).all()
    assert np.abs(mean - bmean).max() <= 1e-12 * np.abs(bmean).max()
    assert np.abs(var - bvar).max() <= 1e-12 * np.abs(bvar).max()
    # the weights that count are those of the good rows, renormalised
    w = ph.normalise(weights, len(means), bad)
    assert abs(w.sum() - 1.0) < 1e-15 and not w[bad].any()


def test_host_mixture_identities():
    means, variances, _, _ = _case(4)
    T = len(means)
    one = np.zeros(T)
    one[T // 2] = 1.0
    mean, var = ph.mixture(means, variances, one)
    assert np.array_equal(mean, means[T // 2]) and np.array_equal(var, variances[T // 2])
    a, b = ph.mixture(means, variances, None), ph.mixture(means, variances, np.full(T, 1.0 / T))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _bare_regressor(n_hyperpars=3, d=1):
    """A GpRegressor with the attributes the argument checks read and no device behind it."""
    from inference_amd.gp import GpRegressor

    gp = GpRegressor.__new__(GpRegressor)
    gp.n_dimensions, gp.n_hyperpars = d, n_hyperpars
    return gp


@pytest.mark.parametrize("weights", [np.ones(3), np.ones(5), [1, -1, 1, 1], [1, np.nan, 1, 1], [1, np.inf, 1, 1],
                                     np.zeros(4), np.ones((4, 1))])
def test_bad_weights_are_refused(weights):
    gp = _bare_regressor()
    with pytest.raises(ValueError, match="weights"):
        gp.predict_marginalised(np.linspace(0, 1, 5), np.zeros((4, 3)), weights=weights)


def test_bad_theta_width_and_failed_value_are_refused():
    from inference_amd.gp import _messages as msg

    gp = _bare_regressor()
    pts = np.linspace(0, 1, 5)
    for call in (gp.predict_samples, gp.predict_marginalised):
        with pytest.raises(ValueError) as err:
            call(pts, np.zeros((4, 2)))
        assert str(err.value) == msg.wrong_hyperpar_count(3, 2)  # the error of set_hyperparameters
        with pytest.raises(ValueError, match="failed"):
            call(pts, np.zeros((4, 3)), failed="ignore")
        with pytest.raises(ValueError):
            call(np.zeros((2, 2, 2)), np.zeros((4, 3)))  # process_points


def test_weights_are_normalised_on_the_host():
    from inference_amd.gp import GpRegressor

    w = GpRegressor._mixture_weights([2.0, 0.0, 6.0, 0.0], 4)
    assert np.array_equal(w, [0.25, 0.0, 0.75, 0.0])
    assert np.array_equal(GpRegressor._mixture_weights([0, 0, 1], 3), [0.0, 0.0, 1.0])
    assert np.array_equal(GpRegressor._mixture_weights(None, 8), np.full(8, 0.125))
    assert np.array_equal(GpRegressor._mixture_weights(None, 7), GpRegressor._mixture_weights(np.full(7, 1 / 7), 7))


def test_symbol_is_bound():
    from inference_amd import _lib

    assert "gpmi_predict_batch" in _lib.SIGNATURES and "gpmi_predict_batch" in _lib.Handle._REPEATABLE
    lib = _lib.load()
    assert lib.gpmi_predict_batch.argtypes == _lib.SIGNATURES["gpmi_predict_batch"][1]
    # a NULL handle: GPMI_ERR_ARG, nothing touched
    args = [None] + [0] * (len(lib.gpmi_predict_batch.argtypes) - 1)
    for i, a in enumerate(lib.gpmi_predict_batch.argtypes):
        if i and a not in (_lib.C.c_int, _lib.C.c_int64):
            args[i] = None
    assert lib.gpmi_predict_batch(*args) == -1


def test_no_prediction_without_a_device():
    """Without a GPU nothing is predicted on the host instead: the engine behind the regressor cannot be created."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from inference_amd import _lib
    from inference_amd.gp import ConstantMean, SquaredExponential

    x, y, e = ph.dataset("a")
    gp = _bare_regressor(n_hyperpars=3, d=1)
    gp.x, gp.y, gp._noise_var, gp._y_cov = x, y, e**2, None
    gp._engine = gp._device = gp._mix = gp._het_slice = gp._sum_kernels = None
    gp._generic, gp._reserve = False, 0
    gp.cov, gp.mean = SquaredExponential(), ConstantMean()
    for call in (gp.predict_samples, gp.predict_marginalised):
        with pytest.raises(_lib.GpmiUnavailable):
            call(np.linspace(0, 1, 5), np.zeros((4, 3)))
