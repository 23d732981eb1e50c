"""
GPU tests of the Matern32 / Matern52 device kernels through the whole GpRegressor surface, GpLinearInverter and
GpOptimiser.  The reference has no Matern: the yardstick is the NumPy / SciPy oracle of tests/matern_host.py and, as a
second way to the same numbers, the package's generic route driven by that module's plugin kernel.  Sizes sit around the
64-wide tile of the covariance kernels.  Tolerances are the project's own for the same quantities of SquaredExponential /
RationalQuadratic: 1e-13 of the largest element for covariance elements, 1e-10 relative for everything behind a
factorisation.  Every test runs with the engine's dense host-composition entry points (`*_dense`) made to raise, so a
fall back off the device path fails; the plugin route, which lives on those entry points, is computed inside
`dense_allowed()`.
"""
import contextlib
import math
import warnings

import numpy as np
import pytest

import matern_host as mh

pytestmark = pytest.mark.gpu

RTOL = 1e-10
KINDS = {"m32": "Matern32", "m52": "Matern52"}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, tol=RTOL, what=""):
    r = rel(a, b)
    print(f"{what}: {r:.2e}")
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"
    return r


_originals = {}


@pytest.fixture(autouse=True)
def no_dense_path(monkeypatch):
    from inference_amd._engine import GpEngine

    def tripwire(name):
        def fail(*args, **kwargs):
            raise AssertionError(f"GpEngine.{name} called: a Matern model left the device path")

        return fail

    for name in dir(GpEngine):
        if name.endswith("_dense"):
            _originals[name] = getattr(GpEngine, name)
            monkeypatch.setattr(GpEngine, name, tripwire(name))


@contextlib.contextmanager
def dense_allowed():
    """The plugin route (host-built matrices through gpmi_*_dense) for the comparison values."""
    from inference_amd._engine import GpEngine

    with pytest.MonkeyPatch.context() as mp:
        for name, fn in _originals.items():
            mp.setattr(GpEngine, name, fn)
        yield


def _cls(kind):
    import inference_amd.gp as gp

    return {"m32": gp.Matern32, "m52": gp.Matern52, "se": gp.SquaredExponential, "rq": gp.RationalQuadratic,
            "wn": gp.WhiteNoise, "het": gp.HeteroscedasticNoise}[kind]


def _device_cov(parts):
    import inference_amd.gp as gp

    objs = [gp.ChangePoint([_cls(k)() for k in p[1]], axis=p[2]) if p[0] == "cp" else _cls(p[0])() for p in parts]
    cov = objs[0]
    for o in objs[1:]:
        cov = cov + o
    return cov


def _plugin_cov(parts):
    import inference_amd.gp as gp

    def one(k):
        return _cls(k)() if k in ("wn", "het") else mh.HostKernel(k)

    objs = [gp.ChangePoint([one(k) for k in p[1]], axis=p[2]) if p[0] == "cp" else one(p[0]) for p in parts]
    cov = objs[0]
    for o in objs[1:]:
        cov = cov + o
    return cov


def _theta(parts, x, seed=0):
    """[mean, the parts' parameters back to back]"""
    n, d = x.shape
    out = [0.1]
    for i, p in enumerate(parts):
        if p[0] == "wn":
            out.append(np.log(0.15))
        elif p[0] == "het":
            out.extend(np.log(np.linspace(0.05, 0.2, n)))
        elif p[0] == "cp":
            for j, k in enumerate(p[1]):
                out.extend(mh.theta_for(k, d, seed + 10 * j))
            out.extend([2.0, 0.5])
        else:
            th = mh.theta_for(p[0], d, seed + i)
            th[0] -= 0.3 * i
            out.extend(th)
    return np.array(out, dtype=float)


def _gp(parts, x, y, e, theta, **kw):
    from inference_amd.gp import GpRegressor

    return GpRegressor(x, y, y_err=e, kernel=_device_cov(parts), hyperpars=theta, **kw)


# ------------------------------------------------------------------------------------------------ 1. build
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("n", [63, 64, 65, 130])
@pytest.mark.parametrize("kind", list(KINDS))
def test_build(kind, n, d):
    x, _, _ = mh.dataset(n, d)
    theta = mh.theta_for(kind, d)
    cov = _cls(kind)()
    cov.pass_spatial_data(x)
    K = cov.build_covariance(theta)
    Ko = mh.build(kind, x, theta)
    assert not np.isnan(K).any()
    check(K, Ko, 1e-13, "build_covariance")
    assert np.array_equal(K, K.T)
    a = math.exp(theta[0])
    assert K[0, 1] == a * a == K[1, 0]               # the duplicated point: C(0) = 1 exactly
    assert not K[-1, :-1].any() and not K[:-1, -1].any()  # the far point: exactly 0.0 off the diagonal
    rng = np.random.default_rng(n + d)
    for m in (1, 65):
        u = rng.uniform(0.0, 4.0, size=(m, d))
        u[0] = x[2]  # a query point on a training point
        Kq = cov(u, x, theta)
        assert Kq.shape == (m, n) and not np.isnan(Kq).any()
        check(Kq, mh.cross(kind, u, x, theta), 1e-13, f"cov(u, x) m={m}")
        assert Kq[0, 2] == a * a and not Kq[:, -1].any()
    Kg, grads = cov.covariance_and_gradients(theta)
    _, go = mh.build_and_grads(kind, x, theta)
    assert np.array_equal(Kg, K) and len(grads) == len(go) == d + 1
    for j, (g1, g2) in enumerate(zip(grads, go)):
        assert not np.isnan(g1).any()
        check(g1, g2, 1e-13, f"dK/dtheta_{j}")


# ------------------------------------------------------------------------------------------------ 2. fit ... LOO
@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(n, d):
        if (n, d) not in cache:
            x, y, e = mh.dataset(n, d)
            pts = np.random.default_rng(n).uniform(0.0, 4.0, size=(65, d))
            cache[(n, d)] = (x, y, e, pts)
        return cache[(n, d)]

    return get


@pytest.mark.parametrize("wn", [False, True])
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fit_predict_lml_gradient_loo(problems, kind, n, wn):
    x, y, e, pts = problems(n, 3)
    parts = [(kind,)] + ([("wn",)] if wn else [])
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    assert gp._generic is False and gp._kernel_id == {"m32": 3, "m52": 4}[kind]
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta)
    check(gp.K_xx, orc.K, 1e-13, "K_xx")
    check(gp.alpha, orc.alpha, what="alpha")
    mu, sig = gp(pts)
    omu, osig = orc(pts)
    check(mu, omu, what="mu")
    check(sig, osig, what="sigma")
    pm, pc = gp.build_posterior(pts)
    om, oc = orc.build_posterior(pts)
    check(pm, om, what="posterior mean")
    check(pc, oc, what="posterior covariance")
    other = theta + 0.1 * np.random.default_rng(1).standard_normal(theta.size)
    for t in (theta, other):
        check(gp.marginal_likelihood(t), orc.marginal_likelihood(t), what="lml")
        v, g = gp.marginal_likelihood_gradient(t)
        ov, og = orc.marginal_likelihood_gradient(t)
        check(v, ov, what="lml (gradient call)")
        check(g, og, what="lml gradient")
        check(gp.loo_likelihood(t), orc.loo_likelihood(t), what="loo")
        v, g = gp.loo_likelihood_gradient(t)
        ov, og = orc.loo_likelihood_gradient(t)
        check(v, ov, what="loo (gradient call)")
        check(g, og, what="loo gradient")
    assert gp._generic is False


@pytest.mark.parametrize("kind", list(KINDS))
def test_heteroscedastic_noise(kind):
    x, y, e = mh.dataset(65, 1)
    parts = [(kind,), ("het",)]
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    assert gp._generic is False and gp._het_slice is not None
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta)
    check(gp.marginal_likelihood(theta), orc.marginal_likelihood(theta), what="lml")
    v, g = gp.marginal_likelihood_gradient(theta)
    ov, og = orc.marginal_likelihood_gradient(theta)
    check(v, ov, what="lml (gradient call)")
    check(g, og, what="lml gradient (all N + d + 2 components)")


# ------------------------------------------------------------------------------------------------ 3. batches
@pytest.mark.parametrize("kind", list(KINDS))
def test_batches(problems, kind):
    x, y, e, _ = problems(65, 3)
    parts = [(kind,), ("wn",)]
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    thetas = theta[None, :] + 0.1 * np.random.default_rng(2).standard_normal((5, theta.size))
    single_lml = np.array([gp.marginal_likelihood(t) for t in thetas])
    single_grad = [gp.marginal_likelihood_gradient(t) for t in thetas]
    single_loo = [gp.loo_likelihood_gradient(t) for t in thetas]
    for T in (1, 5):
        check(gp.marginal_likelihood_batch(thetas[:T]), single_lml[:T], what=f"lml batch T={T}")
        v, g = gp.marginal_likelihood_gradient_batch(thetas[:T])
        check(v, [s[0] for s in single_grad[:T]], what=f"gradient batch T={T}: lml")
        check(g, np.array([s[1] for s in single_grad[:T]]), what=f"gradient batch T={T}: gradient")
        v, g = gp.loo_likelihood_gradient_batch(thetas[:T])
        check(v, [s[0] for s in single_loo[:T]], what=f"loo gradient batch T={T}: loo")
        check(g, np.array([s[1] for s in single_loo[:T]]), what=f"loo gradient batch T={T}: gradient")
    gp.batch_independent_values(True)
    one, five = gp.marginal_likelihood_batch(thetas[:1]), gp.marginal_likelihood_batch(thetas)
    assert one[0] == five[0]
    g1, g5 = gp.marginal_likelihood_gradient_batch(thetas[:1]), gp.marginal_likelihood_gradient_batch(thetas)
    assert g1[0][0] == g5[0][0] and np.array_equal(g1[1][0], g5[1][0])
    gp.batch_independent_values(False)


@pytest.mark.parametrize("kind", list(KINDS))
def test_batch_sentinel_as_for_se(problems, kind):
    from numpy.linalg import LinAlgError

    x, y, e, _ = problems(65, 3)
    results = {}
    for k in (kind, "se"):
        parts = [(k,)]
        theta = _theta(parts, x)
        bad = theta.copy()
        bad[1] = 400.0  # a^2 overflows: no factorisation
        gp = _gp(parts, x, y, e, theta)
        thetas = np.array([theta, bad, theta])
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            values, grads = gp.marginal_likelihood_gradient_batch(thetas, failed="sentinel")
        n_warn = len([w for w in caught if "Cholesky decomposition failure" in str(w.message)])
        with pytest.raises(LinAlgError):
            gp.marginal_likelihood_gradient_batch(thetas, failed="raise")
        sv, sg = gp.marginal_likelihood_gradient(theta)
        for row in (0, 2):
            check(values[row], sv, what="good row beside a failed one: lml")
            check(grads[row], sg, what="good row beside a failed one: gradient")
        results[k] = (n_warn, values[1], bool(grads[1].any()))
    assert results[kind] == results["se"] == (1, -1e50, False)


# ------------------------------------------------------------------------------------------------ 4. sums and mixtures
SUMS = {
    "m52+se": [("m52",), ("se",)],
    "m32+rq+wn": [("m32",), ("rq",), ("wn",)],
    "cp[m52,se]": [("cp", ("m52", "se"), 0)],
}


@pytest.mark.parametrize("tag", list(SUMS))
def test_sums_and_mixtures(problems, tag):
    from inference_amd import _lib
    from inference_amd.gp import GpRegressor

    parts = SUMS[tag]
    x, y, e, pts = problems(130, 3)
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    assert gp._generic is False and gp._kernel_id == (-1 if tag.startswith("cp") else _lib.KERNEL_SUM)
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta)
    with dense_allowed():
        plug = GpRegressor(x, y, y_err=e, kernel=_plugin_cov(parts), hyperpars=theta)
        assert plug._generic
        p_mu, p_sig = plug(pts)
        p_lml = plug.marginal_likelihood(theta)
        p_grad = plug.marginal_likelihood_gradient(theta)[1]
    check(gp.alpha, orc.alpha, what="alpha")
    mu, sig = gp(pts)
    omu, osig = orc(pts)
    check(mu, omu, what="mu vs oracle")
    check(sig, osig, what="sigma vs oracle")
    check(mu, p_mu, what="mu vs plugin route")
    check(sig, p_sig, what="sigma vs plugin route")
    lml = gp.marginal_likelihood(theta)
    check(lml, orc.marginal_likelihood(theta), what="lml vs oracle")
    check(lml, p_lml, what="lml vs plugin route")
    v, g = gp.marginal_likelihood_gradient(theta)
    ov, og_lml = orc.marginal_likelihood_gradient(theta)
    check(v, ov, what="lml (gradient call)")
    check(g, og_lml, what="lml gradient vs oracle")
    check(g, p_grad, what="lml gradient vs plugin route")
    check(gp.loo_likelihood(theta), orc.loo_likelihood(theta), what="loo vs oracle")
    v, g = gp.loo_likelihood_gradient(theta)
    ov, og = orc.loo_likelihood_gradient(theta)
    check(g, og, what="loo gradient vs oracle")
    thetas = np.array([theta, theta + 0.05])
    check(gp.marginal_likelihood_gradient_batch(thetas)[1][0], og_lml, what="gradient batch vs oracle")


# ------------------------------------------------------------------------------------------------ 5. spatial gradients
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_spatial_gradients(kind, d):
    x, y, e = mh.dataset(130, d, far=False)
    parts = [(kind,)]
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta)
    scales = np.exp(theta[2:])
    rng = np.random.default_rng(9)
    for m in (1, 3, 65):
        q = rng.uniform(0.2, 3.8, size=(m, d))
        q[0] = x[3]  # a query point on a training point: no division by r anywhere
        gmu, gcov = gp.gradient(q)
        omu, ocov = orc.gradient(q, kind)
        check(np.reshape(gmu, (m, d)), omu, what=f"gradient mean m={m}")
        check(np.reshape(gcov, (m, d, d)), ocov, what=f"gradient covariance m={m}")
        dmu, dvar = gp.spatial_derivatives(q)
        odmu, odvar = orc.spatial_derivatives(q, kind)
        check(np.reshape(dmu, (m, d)), odmu, what=f"d mu / dx m={m}")
        check(np.reshape(dvar, (m, d)), odvar, what=f"d var / dx m={m}")
        bmu, bvar = gp.spatial_derivatives_batch(q)
        assert bmu.shape == bvar.shape == (m, d)
        check(bmu, odmu, what=f"batch d mu / dx m={m}")
        check(bvar, odvar, what=f"batch d var / dx m={m}")
    # central differences of the device's own prediction, step 1e-5 l, away from the data points (Matern32 is only once
    # differentiable at r = 0): truncation ~ 1e-10, rounding ~ 1e-16 / 1e-5 - 1e-6 of the largest component
    q = rng.uniform(0.2, 3.8, size=(3, d))
    dmu, dvar = gp.spatial_derivatives_batch(q)
    for i in range(d):
        h = np.zeros(d)
        h[i] = 1e-5 * scales[i]
        mp, sp = gp(q + h)
        mm, sm = gp(q - h)
        assert np.abs(dmu[:, i] - (mp - mm) / (2 * h[i])).max() <= 1e-6 * np.abs(dmu).max()
        assert np.abs(dvar[:, i] - (sp**2 - sm**2) / (2 * h[i])).max() <= 1e-6 * np.abs(dvar).max()


def test_rational_quadratic_still_raises(problems):
    from inference_amd.gp import ChangePoint, GpRegressor, Matern52, RationalQuadratic, SquaredExponential

    x, y, e, pts = problems(65, 3)
    gp = _gp([("rq",)], x, y, e, _theta([("rq",)], x))
    for call in (gp.gradient, gp.spatial_derivatives, gp.spatial_derivatives_batch):
        with pytest.raises(NotImplementedError, match="Gradient calculations are not yet available"):
            call(pts[:3])
    parts = [("cp", ("m52", "se"), 0)]
    cp = _gp(parts, x, y, e, _theta(parts, x))
    with pytest.raises(NotImplementedError, match="Gradient calculations are not yet available"):
        cp.spatial_derivatives(pts[:3])
    parts = [("m52",), ("se",)]
    sm = _gp(parts, x, y, e, _theta(parts, x))
    with pytest.raises(NotImplementedError, match="Gradient calculations are not yet available"):
        sm.gradient(pts[:3])


# ------------------------------------------------------------------------------------------------ 6. marginalised prediction
@pytest.mark.parametrize("kind", list(KINDS))
def test_marginalised_prediction(problems, kind):
    x, y, e, pts = problems(130, 3)
    parts = [(kind,), ("wn",)]
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    assert gp._lockstep_predict_ok()
    before = (np.array(gp.hyperpars), gp.alpha.copy(), gp.L.copy(), gp(pts))
    thetas = theta[None, :] + 0.1 * np.random.default_rng(4).standard_normal((3, theta.size))
    means, sigs = gp.predict_samples(pts, thetas)
    mix_mu, mix_sig = gp.predict_marginalised(pts, thetas)
    after = (np.array(gp.hyperpars), gp.alpha.copy(), gp.L.copy(), gp(pts))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[2], after[2])
    assert np.array_equal(before[3][0], after[3][0]) and np.array_equal(before[3][1], after[3][1])
    loop = _gp(parts, x, y, e, theta)
    lm, ls = [], []
    for t in thetas:
        loop.set_hyperparameters(t)
        a, b = loop(pts)
        lm.append(a)
        ls.append(b)
    lm, ls = np.array(lm), np.array(ls)
    check(means, lm, what="predict_samples: means")
    check(sigs, ls, what="predict_samples: sigmas")
    mean = lm.mean(axis=0)
    check(mix_mu, mean, what="predict_marginalised: mean")
    check(mix_sig, np.sqrt((ls**2 + (lm - mean) ** 2).mean(axis=0)), what="predict_marginalised: sigma")


# ------------------------------------------------------------------------------------------------ 7. GpLinearInverter
def test_linear_inverter_with_a_matern52_prior():
    from scipy.linalg import cholesky, solve_triangular

    from inference_amd.gp import GpLinearInverter, Matern52

    n, m = 40, 25
    pos = np.linspace(0.0, 4.0, n)[:, None]
    centres = np.linspace(0.3, 3.7, m)
    A = np.exp(-0.5 * ((centres[:, None] - pos[None, :, 0]) / 0.35) ** 2)
    A /= A.sum(axis=1, keepdims=True)
    rng = np.random.default_rng(8)
    y = A @ (np.sin(1.3 * pos[:, 0]) + 0.5) + 0.1 * rng.standard_normal(m)
    y_err = np.full(m, 0.1)
    gli = GpLinearInverter(y=y, y_err=y_err, model_matrix=A, parameter_spatial_positions=pos,
                           prior_covariance_function=Matern52())
    assert gli._dense is False
    theta = np.array([0.3, 0.2, np.log(0.9)])
    K, dK = mh.build_and_grads("m52", pos, theta[1:])
    r = y - A @ np.full(n, theta[0])
    L = cholesky(A @ K @ A.T + np.diag(y_err**2), lower=True)
    iJ = solve_triangular(L, np.eye(m), lower=True)
    iJ = iJ.T @ iJ
    alpha = iJ @ r
    o_lml = -0.5 * r @ alpha - np.log(np.diag(L)).sum()
    w = A.T @ alpha
    Q = np.outer(w, w) - A.T @ iJ @ A
    o_grad = np.concatenate([[w.sum()], [0.5 * (Q * G).sum() for G in dK]])
    o_mean = theta[0] + K @ w
    o_cov = K - K @ A.T @ iJ @ A @ K
    check(gli.marginal_likelihood(theta), o_lml, what="lml")
    v, g = gli.marginal_likelihood_gradient(theta)
    check(v, o_lml, what="lml (gradient call)")
    check(g, o_grad, what="lml gradient")
    pm, pc = gli.calculate_posterior(theta)
    check(pm, o_mean, what="posterior mean")
    check(pc, o_cov, what="posterior covariance")
    check(gli.calculate_posterior_mean(theta), o_mean, what="posterior mean only")


# ------------------------------------------------------------------------------------------------ 8. callers
def test_default_search():
    from inference_amd.gp import GpRegressor, Matern52

    x, y, e = mh.dataset(65, 2, far=False)
    np.random.seed(11)
    gp = GpRegressor(x, y, y_err=e, kernel=Matern52())
    assert gp._generic is False
    th = np.asarray(gp.hyperpars, float)
    for v, (lo, hi) in zip(th, gp.hp_bounds):
        assert lo <= v <= hi
    best = gp.marginal_likelihood(th)
    assert len(gp.search_log) >= 2
    for start, _, _ in gp.search_log:
        assert best >= gp.marginal_likelihood(start)


def test_optimiser_proposal_and_ei_gradient():
    from inference_amd.gp import GpOptimiser, Matern52

    rng = np.random.default_rng(21)
    bounds = [(0.0, 4.0), (0.0, 4.0)]
    x = rng.uniform(0.0, 4.0, size=(20, 2))
    y = np.sin(x[:, 0]) * np.cos(0.7 * x[:, 1]) + 0.05 * rng.standard_normal(20)
    theta = np.array([0.0, -0.3, np.log(1.1), np.log(1.4)])
    opt = GpOptimiser(x, y, bounds=bounds, y_err=np.full(20, 0.05), hyperpars=theta, kernel=Matern52)
    assert opt.gp._generic is False and opt.gp._kernel_id == 4
    np.random.seed(5)
    prop = np.asarray(opt.propose_evaluation())
    assert prop.shape == (2,)
    for v, (lo, hi) in zip(prop, bounds):
        assert lo <= v <= hi
    # the analytic gradient of -ln EI against central differences of it (step 1e-5, tolerance 1e-5 of the gradient)
    for q in rng.uniform(0.5, 3.5, size=(3, 2)):
        val, grad = opt.acquisition.opt_func_gradient(q)
        fd = np.zeros(2)
        for i in range(2):
            h = np.zeros(2)
            h[i] = 1e-5
            fd[i] = (opt.acquisition.opt_func(q + h) - opt.acquisition.opt_func(q - h)) / 2e-5
        check(val, opt.acquisition.opt_func(q), 1e-12, "-ln EI")
        check(grad, fd, 1e-5, "EI gradient vs central differences")
