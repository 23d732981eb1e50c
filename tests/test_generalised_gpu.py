"""GeneralisedGpRegressor on the device against the NumPy mirror (tests/generalised_host.py).  Inputs, the mirror's
quantities and their allowances come from tests/golden/generalised.npz (golden/make_golden_generalised.py): an allowance is
ten times what 48 relative ripples of 1e-13 on the mirror's K move the mirror's own quantity, floored at 1e-10 of its scale;
the maker has checked that the mirror takes the same Newton steps and halvings under every ripple, so the device's counts
are compared exactly.

  case            likelihood, kernel                              N, d, M       reaches
  poisson_se      Poisson, SquaredExponential                     130, 3, 50    one row past a 128-row tile
  logistic_m52    Logistic with three 8 sigma outliers, Matern52  300, 2, 257   step halving
  binomial_rq     Binomial(trials=3), RationalQuadratic           257, 17, 1    the 64 KiB LDS builders
  poisson_m32     Poisson with y = 0 rows, exposures 1 .. 50, M32 640, 1, 129   a second 512-wide inverse block
"""
import warnings

import numpy as np
import pytest

import generalised_host as gh
from inference_amd import _lib
from inference_amd.gp import (Binomial, GeneralisedGpRegressor, Logistic, Matern32, Matern52, Poisson, RationalQuadratic,
                              SquaredExponential)
from inference_amd.gp.generalised import response_moments

pytestmark = pytest.mark.gpu

LIKS = {"Logistic": Logistic, "Poisson": Poisson, "Binomial": Binomial}
KERNELS = {gh.SE: SquaredExponential, gh.RQ: RationalQuadratic, gh.M32: Matern32, gh.M52: Matern52}
_FITS = {}


def fitted(golden, name):
    """The case's inputs (from the fixture) and its model, fitted once per session"""
    if name not in _FITS:
        g = golden("generalised")
        c = {k: g[f"{name}_{k}"] for k in ("x", "y", "aux", "theta", "theta2", "pts", "logq", "grad", "f", "g", "mean",
                                           "var", "newton", "offset")}
        c["allow"] = {k: float(g[f"{name}_allow_{k}"]) for k in ("logq", "grad", "f", "g", "mean", "var")}
        lik_name, kernel = gh.CASES[name][:2]
        gp = GeneralisedGpRegressor(c["x"], c["y"], likelihood=LIKS[lik_name](c["aux"]), kernel=KERNELS[kernel](),
                                    hyperpars=c["theta"])
        _FITS[name] = (c, gp)
    return _FITS[name]


def within(name, what, got, c):
    err = float(np.abs(np.asarray(got) - c[what]).max())
    print(f"{name:14s} {what:5s} error {err:9.2e}  allowance {c['allow'][what]:9.2e}")
    assert err <= c["allow"][what], (name, what, err, c["allow"][what])


@pytest.mark.parametrize("name", list(gh.CASES))
def test_device_against_mirror(golden, name):
    c, gp = fitted(golden, name)
    assert gp.offset == float(c["offset"])
    log = gp.newton_log
    assert log["converged"] and (log["iterations"], log["halvings"]) == tuple(c["newton"])
    if name == "logistic_m52":
        assert log["halvings"] >= 1
    within(name, "logq", gp._logq, c)
    within(name, "logq", gp.marginal_likelihood(c["theta"]), c)
    logq, grad = gp.marginal_likelihood_gradient(c["theta"])
    within(name, "logq", logq, c)
    within(name, "grad", grad, c)
    within(name, "f", gp.mode, c)
    within(name, "g", gp.alpha, c)
    mu, sig = gp(c["pts"])
    assert mu.shape == sig.shape == (len(c["pts"]),)
    within(name, "mean", mu, c)
    within(name, "var", sig**2, c)
    # psi of the log: -1/2 a^T (f - m) + sum log p at the downloaded mode, log q = psi - sum ln L_ii <= psi
    assert log["psi"] >= gp._logq


@pytest.mark.parametrize("name", ["poisson_se", "logistic_m52"])
def test_repeated_calls_are_bit_identical(golden, name):
    c, gp = fitted(golden, name)
    assert gp.marginal_likelihood(c["theta2"]) == gp.marginal_likelihood(c["theta2"])
    (l1, g1), (l2, g2) = gp.marginal_likelihood_gradient(c["theta2"]), gp.marginal_likelihood_gradient(c["theta2"])
    assert l1 == l2 and np.array_equal(g1, g2)
    (m1, s1), (m2, s2) = gp(c["pts"]), gp(c["pts"])
    assert np.array_equal(m1, m2) and np.array_equal(s1, s2)


@pytest.mark.parametrize("name", list(gh.CASES))
def test_fit_keeps_its_bits_across_evaluations_at_other_theta(golden, name):
    c, gp = fitted(golden, name)
    eng = gp.engine
    mu0, sig0 = gp(c["pts"])
    f0, g0 = eng.ggp_mode()
    gp.marginal_likelihood(c["theta2"])
    gp.marginal_likelihood_gradient(c["theta2"])
    mu1, sig1 = gp(c["pts"])
    f1, g1 = eng.ggp_mode()
    assert np.array_equal(mu0, mu1) and np.array_equal(sig0, sig1) and np.array_equal(f0, f1) and np.array_equal(g0, g1)
    # and a new fit at the same theta gives the same bits as the first
    logq = gp._logq
    gp.set_hyperparameters(c["theta"])
    mu2, sig2 = gp(c["pts"])
    assert gp._logq == logq and np.array_equal(mu0, mu2) and np.array_equal(sig0, sig2)


@pytest.mark.parametrize("name", ["poisson_se", "poisson_m32"])
def test_kv_kernel_bits_and_accuracy(golden, name):
    """One vector alone and as column 3 of 4 give the same bits; against numpy the error stays within
    (np + 4) 2^-53 sum_j |K_ij v_j| (np: the padded n - the summation's length; 4: K's own rounding on the device)"""
    c, gp = fitted(golden, name)
    n = len(c["y"])
    rng = np.random.default_rng(5)
    V = rng.normal(size=(4, n))
    kid = gh.CASES[name][1]
    alone = gp.engine.ggp_kv(kid, c["theta"], V[3:4])
    four = gp.engine.ggp_kv(kid, c["theta"], V)
    assert np.array_equal(alone[0], four[3])
    assert np.array_equal(four, gp.engine.ggp_kv(kid, c["theta"], V))
    K = gh.covariance(kid, c["x"], c["theta"])
    n_pad = -(-n // 128) * 128
    bound = (n_pad + 4) * 2.0**-53 * (np.abs(K) @ np.abs(V).T).T
    err = np.abs(four - (K @ V.T).T)
    print(name, "K V: worst error / bound", float((err / bound).max()))
    assert np.all(err <= bound)


def test_failures_are_reported_and_leave_the_handle_usable(golden):
    c, gp = fitted(golden, "poisson_se")
    eng, kid = gp.engine, gh.CASES["poisson_se"][1]
    good = gp.marginal_likelihood(c["theta"])
    mu0, sig0 = gp(c["pts"])
    # a^2 overflows: B is not finite
    big = c["theta"].copy()
    big[0] = 400.0
    with pytest.warns(RuntimeWarning) as rec:
        assert gp.marginal_likelihood(big) == -1e50
    assert len(rec) == 1
    with pytest.raises(RuntimeError):
        gp.marginal_likelihood_gradient(big)
    assert gp.marginal_likelihood(c["theta"]) == good
    # one Newton step is not enough: info = -1, and the next call is right
    logq, (iters, _), info = eng.ggp_logq(kid, c["theta"], gp.tol, 1)
    assert (logq, iters, info) == (-1e50, 1, -1)
    assert eng.ggp_logq_grad(kid, c["theta"], gp.tol, 1)[3] == -1
    assert eng.ggp_logq(kid, c["theta"], gp.tol, gp.max_iter)[0] == good
    # the fit has not been touched by any of this
    mu1, sig1 = gp(c["pts"])
    assert np.array_equal(mu0, mu1) and np.array_equal(sig0, sig1)


def test_failed_fit_raises_and_drops_the_fit(golden):
    c, _ = fitted(golden, "binomial_rq")
    gp = GeneralisedGpRegressor(c["x"], c["y"], likelihood=Binomial(c["aux"]), kernel=RationalQuadratic(),
                                hyperpars=c["theta"])
    logq = gp._logq
    big = c["theta"].copy()
    big[0] = 400.0
    with pytest.raises(RuntimeError):
        gp.set_hyperparameters(big)
    with pytest.raises(_lib.GpmiError):  # no fit: GPMI_ERR_ARG, not stale numbers
        gp(c["pts"])
    with pytest.raises(RuntimeError):
        GeneralisedGpRegressor(c["x"], c["y"], likelihood=Binomial(c["aux"]), kernel=RationalQuadratic(),
                               hyperpars=c["theta"], max_iter=1)
    gp.set_hyperparameters(c["theta"])
    assert gp._logq == logq
    within("binomial_rq", "mean", gp(c["pts"])[0], c)


def test_argument_errors_leave_the_next_call_right(golden):
    from inference_amd._engine import GpEngine

    c, gp = fitted(golden, "poisson_se")
    kid, theta, n = gh.CASES["poisson_se"][1], c["theta"], len(c["y"])
    eng = GpEngine(c["x"], np.zeros(n))
    good = gp.marginal_likelihood(theta)

    def refused(call, *args):
        with pytest.raises(_lib.GpmiError, match="status -1"):
            call(*args)

    refused(eng.ggp_logq, kid, theta, 1e-9, 50)  # before gpmi_ggp_set_observations
    refused(eng.ggp_set_observations, 7, c["y"], c["aux"], 0.0)
    refused(eng.ggp_set_observations, _lib.GGP_POISSON, c["y"] + 0.5, c["aux"], 0.0)
    refused(eng.ggp_set_observations, _lib.GGP_POISSON, c["y"], -c["aux"], 0.0)
    refused(eng.ggp_set_observations, _lib.GGP_BINOMIAL, c["y"] + 50.0, c["aux"], 0.0)
    refused(eng.ggp_set_observations, _lib.GGP_LOGISTIC, c["y"], 0.0 * c["aux"], 0.0)
    refused(eng.ggp_set_observations, _lib.GGP_POISSON, c["y"], c["aux"], np.inf)
    eng.ggp_set_observations(_lib.GGP_POISSON, c["y"], c["aux"], float(c["offset"]))
    refused(eng.ggp_mode)  # no fit yet
    refused(eng.ggp_predict, c["pts"])
    refused(eng.ggp_logq, kid, theta[:-1], 1e-9, 50)
    refused(eng.ggp_logq, _lib.KERNEL_SUM, theta, 1e-9, 50)
    refused(eng.ggp_logq, kid, theta, 0.0, 50)
    refused(eng.ggp_fit, kid, theta, 1e-9, 0)
    refused(eng.ggp_logq_grad, 17, theta, 1e-9, 50)
    refused(eng.ggp_kv, kid, theta, np.ones((5, n)))
    assert eng.ggp_logq(kid, theta, 1e-9, 50)[0] == good
    assert eng.ggp_fit(kid, theta, 1e-9, 50)[0] == gp._logq
    assert np.array_equal(eng.ggp_predict(c["pts"])[0], gp(c["pts"])[0])
    # a Gaussian fit on the same handle takes lane 0: the generalised queries are refused until the next gpmi_ggp_fit
    eng.fit(kid, theta, 0.1, np.zeros(n))
    refused(eng.ggp_predict, c["pts"])
    eng.close()


def test_constructor_search():
    """hyperpars=None: multi-start L-BFGS-B on the device gradient, N = 200"""
    rng = np.random.default_rng(8)
    x = np.sort(rng.uniform(0.0, 1.0, size=200))
    y = rng.poisson(4.0 * np.exp(np.sin(5.0 * x))).astype(float)
    np.random.seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        gp = GeneralisedGpRegressor(x, y, likelihood=Poisson(exposure=4.0), kernel=SquaredExponential(), n_starts=3)
    log = gp.search_log
    assert log["starts"].shape == (3, 2) and log["values"].shape == (3,)
    best = log["values"].max()
    assert best >= log["start_values"].max() and abs(gp._logq - best) <= 1e-9 * abs(best)
    # a stationary point inside the bounds, or a bound
    _, grad = gp.marginal_likelihood_gradient(gp.hyperpars)
    lwr, upr = np.array(gp.hp_bounds).T
    inside = (gp.hyperpars > lwr + 1e-8) & (gp.hyperpars < upr - 1e-8)
    assert np.all(np.abs(grad[inside]) <= 1e-3 * max(1.0, abs(best)))
    mu, sig = gp(np.linspace(0.1, 0.9, 5))
    assert np.all(np.abs(mu - np.sin(5.0 * np.linspace(0.1, 0.9, 5))) <= 6.0 * sig + 0.5)


@pytest.mark.parametrize("name", list(gh.CASES))
def test_predict_response(golden, name):
    c, gp = fitted(golden, name)
    lik = gp.likelihood
    m = len(c["pts"])
    aux = {"Poisson": 2.0, "Binomial": 5.0, "Logistic": None}[lik.name]
    mean, std = gp.predict_response(c["pts"], aux)
    assert mean.shape == std.shape == (m,) and np.all(std > 0.0)
    # the mirror's response moments, and how far the mirror's own allowances on mean and sigma can move them
    mu, sig = c["mean"], np.sqrt(c["var"])
    d_mu, d_sig = c["allow"]["mean"], c["allow"]["var"] / (2.0 * sig.min())
    ref = response_moments(lik, mu, sig, aux)
    spread = np.zeros(2)
    for sm in (-1.0, 1.0):
        for ss in (-1.0, 1.0):
            moved = response_moments(lik, mu + sm * d_mu, sig + ss * d_sig, aux)
            spread = np.maximum(spread, [np.abs(moved[0] - ref[0]).max(), np.abs(moved[1] - ref[1]).max()])
    for k, got in enumerate((mean, std)):
        allow = 2.0 * spread[k] + 1e-10 * np.abs(ref[k]).max()
        err = np.abs(got - ref[k]).max()
        print(name, ("response mean", "response std")[k], "error", err, "allowance", allow)
        assert err <= allow
