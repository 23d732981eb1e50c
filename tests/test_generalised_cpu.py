"""CPU-only checks of the generalised GP: the likelihood classes against scipy.stats and the reference's
LogisticLikelihood (tests/golden/generalised_lik.npz), their derivatives and the NumPy mirror's gradient
(tests/generalised_host.py) against fourth-order differences, the mirror's latent predictions against the dense definition
(K^-1 + W)^-1, the Gaussian limit of the Poisson model, `predict_response` against quadrature, and the constructor's
argument checks - which all run before the first device call, so they raise here, where there is no device."""
import numpy as np
import pytest
from scipy import stats
from scipy.integrate import quad

import generalised_host as gh
from inference_amd.gp import (Binomial, ChangePoint, GeneralisedGpRegressor, Logistic, Matern32, Matern52, Poisson,
                              RationalQuadratic, SquaredExponential, WhiteNoise)
from inference_amd.gp.generalised import response_moments
from inference_amd.gp.likelihood import logistic_parts

RNG = np.random.default_rng(12)


def fd4(fun, f, h):
    """fourth-order central difference of an element-wise function"""
    return (8.0 * (fun(f + h) - fun(f - h)) - (fun(f + 2 * h) - fun(f - 2 * h))) / (12.0 * h)


def triples():
    n = 400
    f = RNG.normal(0.0, 3.0, size=n)
    yield Logistic(0.7), RNG.normal(0.0, 4.0, size=n), f
    yield Poisson(RNG.uniform(0.5, 20.0, size=n)), RNG.poisson(5.0, size=n).astype(float), 0.5 * f
    yield Binomial(np.full(n, 7.0)), RNG.integers(0, 8, size=n).astype(float), f


def test_log_likelihoods_against_scipy():
    for lik, y, f in triples():
        aux = lik.bind(len(y))
        lik.check(y)
        mine = lik.log_prob(y, f, aux)
        if isinstance(lik, Logistic):
            ref = stats.logistic.logpdf(y, loc=f, scale=aux)
        elif isinstance(lik, Poisson):
            ref = stats.poisson.logpmf(y, aux * np.exp(f))
        else:
            ref = stats.binom.logpmf(y, aux, logistic_parts(f)[0])
        err = np.abs(mine - ref) / np.abs(ref)
        print(type(lik).__name__, "max relative difference from scipy.stats:", err.max())
        assert err.max() <= 1e-13


def test_logistic_equals_the_reference(golden):
    g = golden("generalised_lik")
    for y, sigma, f, value in zip(g["y"], g["sigma"], g["f"], g["value"]):
        lik = Logistic(sigma)
        aux = lik.bind(len(y))
        mine = lik.log_prob(y, f, aux).sum()
        assert abs(mine - value) <= 1e-13 * abs(value), (mine, value)


def test_derivatives_against_fourth_order_differences():
    for lik, y, f in triples():
        aux = lik.bind(len(y))
        g, W, d3 = lik.derivatives(y, f, aux)
        assert np.all(W >= 0.0)
        chain = [lambda t: lik.log_prob(y, t, aux), lambda t: lik.derivatives(y, t, aux)[0],
                 lambda t: -lik.derivatives(y, t, aux)[1]]
        for fun, exact, what in zip(chain, (g, -W, d3), ("g", "W", "d3")):
            d1, d2 = fd4(fun, f, 1e-3), fd4(fun, f, 2e-3)
            scale = np.abs(exact).max()
            allow = 10.0 * np.abs(d1 - d2).max() + 1e-9 * scale  # (the differences' own rounding: 1e-16 x scale / h)
            err = np.abs(d1 - exact).max()
            print(type(lik).__name__, what, "error", err, "allowance", allow)
            assert err <= allow


def small_problem(lik_name, d=2, n=40, seed=4):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, size=(n, d))
    f = gh._smooth(x)
    if lik_name == "Logistic":
        lik = Logistic(0.2)
        y = f + 0.2 * rng.normal(size=n)
        y[3] += 2.0
    elif lik_name == "Poisson":
        lik = Poisson(rng.uniform(1.0, 9.0, size=n))
        y = rng.poisson(lik.exposure * np.exp(f)).astype(float)
    else:
        lik = Binomial(4)
        y = rng.binomial(4, logistic_parts(2.0 * f)[0]).astype(float)
    aux = lik.bind(n)
    lik.check(y)
    return lik, x, y, aux, lik.default_offset(y, aux)


@pytest.mark.parametrize("kernel", [gh.SE, gh.RQ, gh.M32, gh.M52])
@pytest.mark.parametrize("lik_name", ["Logistic", "Poisson", "Binomial"])
def test_mirror_gradient_against_fourth_order_differences(kernel, lik_name):
    lik, x, y, aux, offset = small_problem(lik_name)
    theta = np.concatenate([[0.1], [0.4] if kernel == gh.RQ else [], np.log([0.5, 0.8])])

    def logq(th):
        res = gh.laplace(lik, x, y, aux, offset, kernel, th, tol=1e-12, max_iter=200)
        assert res["info"] == 0
        return res["logq"]

    res = gh.laplace(lik, x, y, aux, offset, kernel, theta, tol=1e-12, max_iter=200)
    assert res["info"] == 0
    assert np.abs(res["a"] - res["g"]).max() <= 1e-9 * np.abs(res["g"]).max()  # at the mode a = grad log p
    grad = gh.gradient(res, kernel, x, theta)
    for j in range(theta.size):
        e = np.zeros(theta.size)
        e[j] = 1.0
        d1, d2 = (fd4(lambda h: logq(theta + h * e), 0.0, step) for step in (1e-3, 2e-3))
        allow = 10.0 * abs(d1 - d2) + 1e-8 * np.abs(grad).max()  # (the differences' rounding: logq to ~1e-12 relative / h)
        assert abs(grad[j] - d1) <= allow, (j, grad[j], d1, d2)


@pytest.mark.parametrize("lik_name", ["Logistic", "Poisson", "Binomial"])
def test_latent_predictions_equal_the_dense_definition(lik_name):
    """mean = m + k^T K^-1 (f-hat - m), var = k_qq - k^T K^-1 k + k^T K^-1 (K^-1 + W)^-1 K^-1 k"""
    lik, x, y, aux, offset = small_problem(lik_name)
    theta = np.array([0.2, np.log(0.3), np.log(0.4)])
    res = gh.laplace(lik, x, y, aux, offset, gh.M32, theta, tol=1e-13, max_iter=200)
    assert res["info"] == 0
    pts = np.random.default_rng(9).uniform(0.0, 1.0, size=(17, 2))
    mean, var = gh.predict(res, gh.M32, x, theta, offset, pts)
    K = res["K"]
    kq = gh.cross_covariance(gh.M32, pts, x, theta)
    Ki = np.linalg.inv(K)
    Sigma = np.linalg.inv(Ki + np.diag(res["W"]))
    mean_d = offset + kq @ Ki @ (res["f"] - offset)
    var_d = np.exp(2 * theta[0]) - np.einsum("qi,ij,qj->q", kq, Ki - Ki @ Sigma @ Ki, kq)
    tol = 100.0 * np.linalg.cond(K) * 2.0**-53  # the dense form inverts K
    print(lik_name, "cond K", np.linalg.cond(K), "mean", np.abs(mean - mean_d).max(), "var", np.abs(var - var_d).max())
    assert np.abs(mean - mean_d).max() <= tol * max(1.0, np.abs(mean_d).max())
    assert np.abs(var - var_d).max() <= tol * np.exp(2 * theta[0])


def test_poisson_with_large_counts_approaches_gaussian_regression():
    """With counts of ~1e4 the Poisson log-likelihood in f is Gaussian about ln(y / e) with variance 1 / y up to a cubic
    term of relative size delta / 3, delta ~ y^-1/2 the posterior's width: the Laplace mode and variance approach the
    Gaussian GP on ln(y / e) with noise 1 / y to O(1 / y).  Measured on this seed (min y 7698, bound 3 / min y = 3.9e-4): mode 7.5e-5, sigma 2.6e-6."""
    rng = np.random.default_rng(21)
    n = 60
    x = rng.uniform(0.0, 1.0, size=(n, 1))
    e = rng.uniform(1.0, 3.0, size=n)
    y = rng.poisson(e * np.exp(9.0 + 0.5 * np.sin(4.0 * x[:, 0]))).astype(float)
    lik = Poisson(e)
    aux = lik.bind(n)
    offset = lik.default_offset(y, aux)
    theta = np.array([np.log(0.5), np.log(0.3)])
    res = gh.laplace(lik, x, y, aux, offset, gh.SE, theta, tol=1e-10)
    assert res["info"] == 0
    K = res["K"]
    z = np.log(y / e) - offset
    A = K + np.diag(1.0 / y)
    mode_g = offset + K @ np.linalg.solve(A, z)
    var_g = np.diag(K - K @ np.linalg.solve(A, K))
    V = np.linalg.solve(res["L"], res["sw"][:, None] * K)
    var_l = np.diag(K) - (V * V).sum(axis=0)
    gap_mode = np.abs(res["f"] - mode_g).max()
    gap_sig = np.abs(np.sqrt(var_l) - np.sqrt(var_g)).max()
    print("min y", y.min(), "mode gap", gap_mode, "sigma gap", gap_sig)
    assert gap_mode <= 3.0 / y.min() and gap_sig <= 3.0 / y.min()


def test_response_moments_against_quadrature():
    mu, sig = np.array([-1.0, 0.3, 2.0]), np.array([0.2, 0.7, 0.05])

    def moments(fun_mean, fun_second):
        out = []
        for m, s in zip(mu, sig):
            pdf = lambda f: stats.norm.pdf(f, m, s)
            m1 = quad(lambda f: fun_mean(f) * pdf(f), m - 12 * s, m + 12 * s, epsabs=1e-13, epsrel=1e-13)[0]
            m2 = quad(lambda f: fun_second(f) * pdf(f), m - 12 * s, m + 12 * s, epsabs=1e-13, epsrel=1e-13)[0]
            out.append((m1, np.sqrt(m2 - m1**2)))
        return np.array(out).T

    e = 2.5
    mean, std = response_moments(Poisson(), mu, sig, e)  # E[y^2 | f] = lam + lam^2
    ref = moments(lambda f: e * np.exp(f), lambda f: e * np.exp(f) + (e * np.exp(f)) ** 2)
    assert np.allclose(mean, ref[0], rtol=1e-10) and np.allclose(std, ref[1], rtol=1e-9)
    n = 6.0
    p = lambda f: logistic_parts(f)[0]
    mean, std = response_moments(Binomial(), mu, sig, n)  # E[y^2 | f] = n p (1 - p) + n^2 p^2
    ref = moments(lambda f: n * p(f), lambda f: n * p(f) * (1 - p(f)) + (n * p(f)) ** 2)
    assert np.allclose(mean, ref[0], rtol=1e-10) and np.allclose(std, ref[1], rtol=1e-8)
    lik = Logistic(0.3)
    lik.bind(3)
    mean, std = response_moments(lik, mu, sig)
    assert np.array_equal(mean, mu) and np.allclose(std, np.sqrt(sig**2 + 0.09), rtol=1e-15)


def test_argument_checks_run_before_any_device_call():
    x = RNG.uniform(size=(12, 2))
    counts = RNG.poisson(3.0, size=12).astype(float)
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts - 0.5, likelihood=Poisson(), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, -counts - 1.0, likelihood=Poisson(), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Poisson(exposure=0.0), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts + 9.0, likelihood=Binomial(trials=3), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Binomial(trials=0), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Logistic(sigma=-1.0), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, np.where(counts > 2, np.nan, counts), likelihood=Logistic(), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(RNG.uniform(size=(12, 65)), counts, likelihood=Poisson(), hyperpars=np.zeros(66))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Poisson(np.ones(5)), hyperpars=np.zeros(3))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Poisson(), hyperpars=np.zeros(4))
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Poisson(), hyperpars=np.zeros(3), offset=np.inf)
    with pytest.raises(ValueError):
        GeneralisedGpRegressor(x, counts, likelihood=Poisson(), hyperpars=np.zeros(3), tol=0.0)
    for kernel in (SquaredExponential() + WhiteNoise(), SquaredExponential() + Matern32(),
                   ChangePoint(kernels=[SquaredExponential, RationalQuadratic])):
        with pytest.raises(NotImplementedError):
            GeneralisedGpRegressor(x, counts, likelihood=Poisson(), kernel=kernel, hyperpars=np.zeros(3))
    with pytest.raises(NotImplementedError):
        GeneralisedGpRegressor(x, counts, likelihood=object(), kernel=Matern52, hyperpars=np.zeros(3))


def test_pair_regime_fixture_belongs_to_its_seeded_case(golden):
    """tests/golden/generalised_pair.npz holds results only; tests/test_pair_regime_gpu.py regenerates the inputs from the
    seed.  The two must belong together: shapes, the offset, and the mirror's own stationarity at the stored mode -
    g = grad log p(y | f) for the regenerated y, which no other data set would satisfy."""
    g = golden("generalised_pair")
    for name, (lik_name, kernel, n, d, m, seed) in gh.PAIR_CASES.items():
        c = gh.make_case(name)
        assert c["x"].shape == (n, d) and c["pts"].shape == (m, d) and -(-n // 128) * 128 >= 5120
        assert np.array_equal(c["y"], gh.make_case(name)["y"])
        lik = Poisson(c["aux_arg"])
        aux = lik.bind(n)
        assert float(g[f"{name}_offset"]) == lik.default_offset(c["y"], aux)
        assert g[f"{name}_f"].shape == g[f"{name}_g"].shape == (n,) and g[f"{name}_mean"].shape == g[f"{name}_var"].shape == (m,)
        assert g[f"{name}_newton"][0] >= 2 and f"{name}_grad" not in g and f"{name}_x" not in g
        grad = lik.derivatives(c["y"], g[f"{name}_f"], aux)[0]
        assert np.abs(grad - g[f"{name}_g"]).max() <= 1e-12 * np.abs(grad).max()
        for k in ("logq", "f", "g", "mean", "var"):
            assert float(g[f"{name}_allow_{k}"]) >= 1e-10 * np.abs(g[f"{name}_{k}"]).max() > 0.0
