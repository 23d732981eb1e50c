"""
GPU tests of the Periodic device kernel (GPMI_KERNEL_PER) through the GpRegressor surface, GpOptimiser and the C-ABI.
The reference has no periodic kernel: the yardsticks are the NumPy mirror of tests/periodic_host.py - in long double for
the element-wise bound on the covariance build - and the package's generic route driven by that module's plugin kernel,
at the project's 1e-10 relative for everything behind a factorisation.  Sizes sit around the 64-wide tile of the
covariance kernels.  Every test runs with the engine's dense host-composition entry points (`*_dense`) made to raise, so a
fall back off the device path fails; the plugin route, which lives on those entry points, is computed inside
`dense_allowed()`.
"""
import contextlib
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import matern_host as mh
import periodic_host as ph

pytestmark = pytest.mark.gpu

RTOL = 1e-10


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
            raise AssertionError(f"GpEngine.{name} called: a Periodic model left the device path")

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


# a model: a list of parts ("per", dims) | ("se",) | ("rq",) | ("m52",) | ("wn",) | ("het",), summed in that order
def _device_cov(parts):
    import inference_amd.gp as gp

    cls = {"se": gp.SquaredExponential, "rq": gp.RationalQuadratic, "m52": gp.Matern52, "wn": gp.WhiteNoise,
           "het": gp.HeteroscedasticNoise}
    objs = [gp.Periodic(periodic_dims=p[1]) if p[0] == "per" else cls[p[0]]() for p in parts]
    cov = objs[0]
    for o in objs[1:]:
        cov = cov + o
    return cov


def _plugin_cov(parts):
    import inference_amd.gp as gp

    def one(p):
        if p[0] == "per":
            return ph.HostKernel(p[1])
        return {"wn": gp.WhiteNoise, "het": gp.HeteroscedasticNoise}[p[0]]() if p[0] in ("wn", "het") else mh.HostKernel(p[0])

    objs = [one(p) for p in parts]
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
        elif p[0] == "per":
            dims = list(range(d)) if p[1] is None else p[1]
            th = ph.theta_for(d, dims, seed + i)
            th[0] -= 0.3 * i
            out.extend(th)
        else:
            th = mh.theta_for(p[0], d, seed + i)
            th[0] -= 0.3 * i
            out.extend(th)
    return np.array(out, dtype=float)


def _gp(parts, x, y, e, theta, **kw):
    from inference_amd.gp import GpRegressor

    return GpRegressor(x, y, y_err=e, kernel=_device_cov(parts), hyperpars=theta, **kw)


def _plug(parts, x, y, e, theta):
    from inference_amd.gp import GpRegressor

    plug = GpRegressor(x, y, y_err=e, kernel=_plugin_cov(parts), hyperpars=theta)
    assert plug._generic
    return plug


# ------------------------------------------------------------------------------------------------ 1. build
def _check_elements(K, u, v, theta, dims, what):
    """|K - K_true| <= the bound of periodic_host.element_bound element by element; returns the largest ratio."""
    true = ph.cross(u, v, theta, dims, np.longdouble)
    err = np.abs(K.astype(np.longdouble) - true)
    ratio = float((err / ph.element_bound(u, v, theta, dims)).max())
    a2 = math.exp(2 * theta[0])
    print(f"{what}: max |dK| / bound = {ratio:.3f}, worst element {float(err.max()) / a2:.2e} a^2")
    assert ratio <= 1.0, f"{what}: an element misses its bound by a factor {ratio:.3f}"
    return ratio


BUILDS = [(n, d, dims) for (d, dims) in [(1, None), (3, [1]), (3, [0, 2]), (3, None)] for n in (63, 64, 65, 130)]
BUILDS += [(65, 17, [0, 16]), (64, 8, None)]  # the 64 KiB LDS path; the cap of 8 periodic dimensions


@pytest.mark.parametrize("n,d,dims", BUILDS)
def test_build(n, d, dims):
    """Square and cross builds against the long-double mirror, element by element:
       |dK_ij| <= a^2 e^-s [(d + 4) s + 4 + sum_periodic (2 / l_k^2)(3 pi |u_k| + 8) + sum_plain 4 w_k / l_k^2] 2^-53
    (three roundings on u = D / p, each worth pi |u| 2^-53 in sin^2; 4 x 2^-53 of sinpi_sq; the fma chain; the exp).
    Largest ratio measured on an MI355X over these cases: see DESIGN.md (Periodic kernel)."""
    from inference_amd.gp import Periodic

    x, _, _ = ph.dataset(n, d)
    pd = list(range(d)) if dims is None else dims
    theta = ph.theta_for(d, pd)
    cov = Periodic(periodic_dims=dims)
    cov.pass_spatial_data(x)
    K = cov.build_covariance(theta)
    assert K.shape == (n, n) and not np.isnan(K).any()
    a = math.exp(theta[0])
    off = K.copy()
    off[np.diag_indices(n)] = (a * a) * 1.0  # the diagonal carries a^2 (1 + 1e-12): compared on its own
    _check_elements(off, x, x, theta, pd, f"square n={n} d={d} dims={dims}")
    assert np.array_equal(np.diag(K), np.full(n, (a * a) * (1.0 + 1e-12)))
    assert np.array_equal(K, K.T)
    assert K[0, 1] == a * a == K[1, 0]  # the duplicated point: w = 0, e^0 = 1 exactly
    Kg, grads = cov.covariance_and_gradients(theta)
    _, go = ph.build_and_grads(x, theta, pd)
    assert np.array_equal(Kg, K) and len(grads) == len(go) == 1 + d + len(pd)
    for j, (g1, g2) in enumerate(zip(grads, go)):
        check(g1, g2, 1e-12, f"dK/dtheta_{j}")


@pytest.mark.parametrize("m,n", [(1, 65), (130, 63)])
@pytest.mark.parametrize("d,dims", [(1, None), (3, [1]), (3, [0, 2]), (3, None), (17, [0, 16]), (8, None)])
def test_cross_build(d, dims, m, n):
    from inference_amd.gp import Periodic

    x, _, _ = ph.dataset(n, d)
    pd = list(range(d)) if dims is None else dims
    theta = ph.theta_for(d, pd)
    cov = Periodic(periodic_dims=dims)
    cov.pass_spatial_data(x)
    u = np.random.default_rng(n + d).uniform(0.0, ph.SPAN, size=(m, d))
    u[0] = x[2]  # a query point on a training point
    Kq = cov(u, x, theta)
    assert Kq.shape == (m, n) and not np.isnan(Kq).any()
    _check_elements(Kq, u, x, theta, pd, f"cross ({m}, {n}) d={d} dims={dims}")
    a = math.exp(theta[0])
    assert Kq[0, 2] == a * a


# ------------------------------------------------------------------------------------------------ 2. fit ... LOO
def _compare_with_plugin_route(parts, x, y, e, pts, kernel_id):
    theta = _theta(parts, x)
    other = theta + 0.05 * np.random.default_rng(1).standard_normal(theta.size)
    gp = _gp(parts, x, y, e, theta)
    assert gp._generic is False and gp._kernel_id == kernel_id
    with dense_allowed():
        plug = _plug(parts, x, y, e, theta)
        ref = dict(K=plug.K_xx, alpha=plug.alpha, pred=plug(pts), post=plug.build_posterior(pts))
        ref["loo_pred"] = plug.loo_predictions()
        for tag, t in (("fit", theta), ("other", other)):
            ref[tag] = (plug.marginal_likelihood(t), plug.marginal_likelihood_gradient(t), plug.loo_likelihood(t),
                        plug.loo_likelihood_gradient(t))
    check(gp.K_xx, ref["K"], 1e-13, "K_xx")
    check(gp.alpha, ref["alpha"], what="alpha")
    mu, sig = gp(pts)
    check(mu, ref["pred"][0], what="mu")
    check(sig, ref["pred"][1], what="sigma")
    pm, pc = gp.build_posterior(pts)
    check(pm, ref["post"][0], what="posterior mean")
    check(pc, ref["post"][1], what="posterior covariance")
    lm, ls = gp.loo_predictions()
    check(lm, ref["loo_pred"][0], what="LOO means")
    check(ls, ref["loo_pred"][1], what="LOO sigmas")
    for tag, t in (("fit", theta), ("other", other)):
        lml, (lv, lg), loo, (ov, og) = ref[tag]
        check(gp.marginal_likelihood(t), lml, what=f"lml ({tag})")
        v, g = gp.marginal_likelihood_gradient(t)
        check(v, lv, what=f"lml, gradient call ({tag})")
        check(g, lg, what=f"lml gradient ({tag})")
        check(gp.loo_likelihood(t), loo, what=f"loo ({tag})")
        v, g = gp.loo_likelihood_gradient(t)
        check(v, ov, what=f"loo, gradient call ({tag})")
        check(g, og, what=f"loo gradient ({tag})")
    assert gp._generic is False
    return gp, theta


FITS = {
    "N=130 d=3 [1]": (130, 3, [("per", [1])]),
    "N=300 d=2 [0] + WhiteNoise": (300, 2, [("per", [0]), ("wn",)]),
    "N=640 d=1": (640, 1, [("per", None)]),  # a second 512-wide inverse block
    "N=130 d=2 [1] + HeteroscedasticNoise": (130, 2, [("per", [1]), ("het",)]),
}


@pytest.mark.parametrize("tag", list(FITS))
def test_fit_predict_lml_gradient_loo(tag):
    from inference_amd import _lib

    n, d, parts = FITS[tag]
    x, y, e = ph.dataset(n, d)
    pts = np.random.default_rng(n).uniform(0.0, ph.SPAN, size=(65, d))
    gp, _ = _compare_with_plugin_route(parts, x, y, e, pts, _lib.KERNEL_PER)
    assert (gp._het_slice is not None) == ("Heteroscedastic" in tag)


# ------------------------------------------------------------------------------------------------ 3. sums
SUMS = {
    "se+per[0]+wn": [("se",), ("per", [0]), ("wn",)],
    "per[0]+per[0]": [("per", [0]), ("per", [0])],
    "m52+per[1]+rq": [("m52",), ("per", [1]), ("rq",)],
}


@pytest.mark.parametrize("tag", list(SUMS))
def test_sums(tag):
    from inference_amd import _lib

    x, y, e = ph.dataset(200, 2)
    pts = np.random.default_rng(200).uniform(0.0, ph.SPAN, size=(65, 2))
    gp, theta = _compare_with_plugin_route(SUMS[tag], x, y, e, pts, _lib.KERNEL_SUM)
    thetas = np.array([theta, theta + 0.02])
    v, g = gp.marginal_likelihood_gradient_batch(thetas)
    sv, sg = gp.marginal_likelihood_gradient(theta)
    check(v[0], sv, what="gradient batch: lml")
    check(g[0], sg, what="gradient batch: gradient")
    with pytest.raises(NotImplementedError, match="Gradient calculations are not yet available"):
        gp.spatial_derivatives(pts[:3])  # sums stay refused, as before


# ------------------------------------------------------------------------------------------------ 4. lockstep
def test_lockstep_batches():
    """T = 5 rows, row 2 with ln p = -800 (1 / p overflows: the diagonal's 0 x inf is NaN and the row does not factorise).
    `loo_likelihood_gradient_batch` has no `failed` argument: a row that does not factorise raises for the whole batch, as
    for every other kernel."""
    from numpy.linalg import LinAlgError

    parts = [("per", [1]), ("wn",)]
    x, y, e = ph.dataset(130, 3)
    pts = np.random.default_rng(3).uniform(0.0, ph.SPAN, size=(40, 3))
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    assert gp._lockstep_predict_ok()
    thetas = theta[None, :] + 0.05 * np.random.default_rng(2).standard_normal((5, theta.size))
    thetas[2, 1 + 1 + 3] = -800.0  # [mean, ln a, ln l x 3, ln p, ln sigma]
    good = [0, 1, 3, 4]
    single_lml = {t: gp.marginal_likelihood(thetas[t]) for t in good}
    single_grad = {t: gp.marginal_likelihood_gradient(thetas[t]) for t in good}
    single_loo = {t: gp.loo_likelihood_gradient(thetas[t]) for t in good}
    gp.batch_independent_values(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lml = gp.marginal_likelihood_batch(thetas)
        gv, gg = gp.marginal_likelihood_gradient_batch(thetas, failed="sentinel")
        mix_mu, mix_sig, means, sigs = gp.predict_marginalised(pts, thetas, return_samples=True, failed="skip")
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_gradient_batch(thetas, failed="raise")
    with pytest.raises(LinAlgError):
        gp.loo_likelihood_gradient_batch(thetas)
    with pytest.raises(LinAlgError):
        gp.predict_marginalised(pts, thetas)
    assert lml[2] == -1e50 and gv[2] == -1e50 and not gg[2].any()
    assert np.isnan(means[2]).all() and np.isnan(sigs[2]).all()
    assert not np.isnan(lml).any() and not np.isnan(mix_mu).any() and not np.isnan(mix_sig).any()
    lv, lg = gp.loo_likelihood_gradient_batch(thetas[good])
    for i, t in enumerate(good):
        one = thetas[t:t + 1]
        # a row of the batch of five == the same row in a batch of one, bit for bit
        assert gp.marginal_likelihood_batch(one)[0] == lml[t]
        v1, g1 = gp.marginal_likelihood_gradient_batch(one)
        assert v1[0] == gv[t] and np.array_equal(g1[0], gg[t])
        o1, og1 = gp.loo_likelihood_gradient_batch(one)
        assert o1[0] == lv[i] and np.array_equal(og1[0], lg[i])
        m1, s1 = gp.predict_samples(pts, one)
        assert np.array_equal(m1[0], means[t]) and np.array_equal(s1[0], sigs[t])
        # ... and the single-evaluation entry point to 1e-10
        check(lml[t], single_lml[t], what=f"row {t}: lml batch")
        check(gv[t], single_grad[t][0], what=f"row {t}: gradient batch, lml")
        check(gg[t], single_grad[t][1], what=f"row {t}: gradient batch, gradient")
        check(lv[i], single_loo[t][0], what=f"row {t}: loo gradient batch, loo")
        check(lg[i], single_loo[t][1], what=f"row {t}: loo gradient batch, gradient")
    gp.batch_independent_values(False)
    loop = _gp(parts, x, y, e, theta)
    lm, lsd = [], []
    for t in good:
        loop.set_hyperparameters(thetas[t])
        a, b = loop(pts)
        lm.append(a)
        lsd.append(b)
    lm, lsd = np.array(lm), np.array(lsd)
    check(means[good], lm, what="predict_marginalised: the rows' means")
    check(sigs[good], lsd, what="predict_marginalised: the rows' sigmas")
    mean = lm.mean(axis=0)
    check(mix_mu, mean, what="predict_marginalised: mean of the good rows")
    check(mix_sig, np.sqrt((lsd**2 + (lm - mean) ** 2).mean(axis=0)), what="predict_marginalised: sigma of the good rows")


# ------------------------------------------------------------------------------------------------ 5. spatial gradients
def _mirror_gradients(gp, q, x, theta_cov, dims, n_mean=1):
    """The reference's algorithms for the predictive gradients (one point at a time) on the mirror's gradient_terms and
    the model's own factor."""
    from scipy.linalg import solve_triangular

    L, alpha = gp.L, gp.alpha
    gmu, gcov, dvar = [], [], []
    for r in q:
        k = ph.cross(r[None, :], x, theta_cov, dims)[0]
        A, R = ph.gradient_terms(r, x, theta_cov, dims)
        Q = solve_triangular(L, (A * k[None, :]).T, lower=True)
        gmu.append(A @ (k * alpha))
        gcov.append(R - Q.T @ Q)
        z = solve_triangular(L.T, solve_triangular(L, k, lower=True), lower=False)
        dvar.append(-2.0 * (A * k[None, :]) @ z)
    return np.array(gmu), np.array(gcov), np.array(dvar)


@pytest.mark.parametrize("d,dims", [(3, [1]), (1, None)])
def test_spatial_gradients(d, dims):
    x, y, e = ph.dataset(130, d)
    parts = [("per", dims)]
    pd = list(range(d)) if dims is None else dims
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    rng = np.random.default_rng(9)
    for m in (1, 130):
        q = rng.uniform(0.0, ph.SPAN, size=(m, d))
        q[0] = x[3]  # a query point on a training point
        omu, ocov, odvar = _mirror_gradients(gp, q, x, theta[1:], pd)
        gmu, gcov = gp.gradient(q)
        gcov = np.reshape(gcov, (m, d, d))
        check(np.reshape(gmu, (m, d)), omu, what=f"gradient mean m={m}")
        check(gcov, ocov, what=f"gradient covariance m={m}")
        # Symmetry: the package keeps the reference's R - Q^T Q with the vector R broadcast over the rows
        # (regression.py:380), for every kernel and for plugin kernels alike, so cov_ij = R_j - (Q^T Q)_ij.  Q^T Q is
        # symmetric bit for bit (one sum serves both elements); cov itself is where the R_k are equal - always for d = 1.
        R = ph.gradient_terms(q[0], x, theta[1:], pd)[1]
        S = R[None, None, :] - gcov
        assert np.abs(S - np.transpose(S, (0, 2, 1))).max() <= 4 * 2.0**-53 * R.max()
        if d == 1 or np.all(R == R[0]):
            assert np.array_equal(gcov, np.transpose(gcov, (0, 2, 1)))
        dmu, dvar = gp.spatial_derivatives(q)
        check(np.reshape(dmu, (m, d)), omu, what=f"d mu / dx m={m}")
        check(np.reshape(dvar, (m, d)), odvar, what=f"d var / dx m={m}")
        bmu, bvar = gp.spatial_derivatives_batch(q)
        assert bmu.shape == bvar.shape == (m, d)
        check(bmu, omu, what=f"batch d mu / dx m={m}")
        check(bvar, odvar, what=f"batch d var / dx m={m}")


# ------------------------------------------------------------------------------------------------ 6. wrap-round
def test_wrap_round():
    x, y, e = ph.dataset(130, 3)
    parts = [("per", [0, 2])]
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    periods = np.exp(theta[1 + 1 + 3:])
    q = np.random.default_rng(4).uniform(0.0, ph.SPAN, size=(50, 3))
    mu, sig = gp(q)
    for k, p in zip([0, 2], periods):
        shifted = q.copy()
        shifted[:, k] += p
        mu2, sig2 = gp(shifted)
        check(mu2, mu, 1e-9, f"mean one period along dimension {k}")
        check(sig2, sig, 1e-9, f"sigma one period along dimension {k}")


def test_an_angle_with_the_period_pinned_at_two_pi():
    from inference_amd.gp import GpRegressor, Periodic

    rng = np.random.default_rng(12)
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, size=60))
    y = np.cos(ang) + 0.4 * np.sin(2 * ang) + 0.05 * rng.standard_normal(60)
    ln_2pi = math.log(2 * math.pi)
    bounds = [(-2.0, 2.0), (-2.3, 2.3), (ln_2pi, ln_2pi)]
    np.random.seed(3)
    gp = GpRegressor(ang, y, y_err=np.full(60, 0.05), kernel=Periodic(hyperpar_bounds=bounds))
    assert gp._generic is False and gp.hyperpars[-1] == ln_2pi
    mu, sig = gp(np.array([[0.0], [2 * np.pi]]))
    check(mu[1], mu[0], 1e-9, "mean at 0 and 2 pi")
    check(sig[1], sig[0], 1e-9, "sigma at 0 and 2 pi")
    assert abs(mu[0] - 1.0) < 0.2  # the seam is interpolated from both sides, not extrapolated


# ------------------------------------------------------------------------------------------------ 7. GpOptimiser
def test_optimiser_proposal():
    from inference_amd.gp import GpOptimiser, Periodic

    rng = np.random.default_rng(21)
    bounds = [(0.0, 4.0)]
    x = rng.uniform(0.0, 4.0, size=(30, 1))
    y = np.sin(2 * np.pi * x[:, 0] / 1.6) + 0.05 * rng.standard_normal(30)
    e = np.full(30, 0.05)
    theta = np.array([0.0, -0.2, np.log(0.9), np.log(1.6)])
    opt = GpOptimiser(x, y, bounds=bounds, y_err=e, hyperpars=theta, kernel=Periodic)
    assert opt.gp._generic is False and opt.gp._kernel_id == 5
    np.random.seed(5)
    prop = float(np.asarray(opt.propose_evaluation()).squeeze())
    assert 0.0 <= prop <= 4.0
    value = opt.acquisition.opt_func(np.array([prop]))
    val_g, grad = opt.acquisition.opt_func_gradient(np.array([prop]))
    with dense_allowed():
        plug = GpOptimiser(x, y, bounds=bounds, y_err=e, hyperpars=theta, kernel=ph.HostKernel())
        assert plug.gp._generic
        p_value = plug.acquisition.opt_func(np.array([prop]))
        p_val_g, p_grad = plug.acquisition.opt_func_gradient(np.array([prop]))
    check(value, p_value, 1e-9, "acquisition value at the proposal")
    check(val_g, p_val_g, 1e-9, "acquisition value (gradient call)")
    assert np.abs(np.asarray(grad) - np.asarray(p_grad)).max() <= 1e-7 * max(1.0, np.abs(p_grad).max())


# ------------------------------------------------------------------------------------------------ 8. add_point
def test_add_point_on_a_reserved_handle():
    parts = [("per", [1]), ("wn",)]
    x, y, e = ph.dataset(131, 3)
    theta = _theta(parts, x[:130])
    gp = _gp(parts, x[:130], y[:130], e[:130], theta, reserve=8)
    cap = gp.engine.capacity()
    gp.add_point(x[130], y[130], e[130])
    assert gp.engine.capacity() == cap and gp.engine.n == 131  # appended in place
    fresh = _gp(parts, x, y, e, theta)
    pts = np.random.default_rng(6).uniform(0.0, ph.SPAN, size=(30, 3))
    check(gp.alpha, fresh.alpha, what="alpha")
    mu, sig = gp(pts)
    fmu, fsig = fresh(pts)
    check(mu, fmu, what="mu")
    check(sig, fsig, what="sigma")
    check(gp.marginal_likelihood(theta), fresh.marginal_likelihood(theta), what="lml")
    check(gp.marginal_likelihood_gradient(theta)[1], fresh.marginal_likelihood_gradient(theta)[1], what="lml gradient")


# ------------------------------------------------------------------------------------------------ 9. C-ABI errors
def test_c_abi_errors_each_followed_by_a_correct_call():
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    x, y, e = ph.dataset(65, 3)
    ip = C.POINTER(C.c_int)
    ERR_ARG = -1  # GPMI_ERR_ARG

    def set_periodic(h, dims, n=None):
        arr = np.ascontiguousarray(dims, dtype=np.int32)
        return h.lib.gpmi_set_periodic(h.ctx, len(arr) if n is None else n, arr.ctypes.data_as(ip))

    bare = _lib.Handle()
    assert set_periodic(bare, [0]) == ERR_ARG  # before any data is set
    assert b"gpmi_set_data" in bare.lib.gpmi_last_error(bare.ctx)
    bare.close()

    eng = GpEngine(x, y, noise_var=e**2)
    h = eng.h
    theta = ph.theta_for(3, [1])
    mu = np.full(65, 0.1)
    with pytest.raises(_lib.GpmiError, match="gpmi_set_periodic first"):
        eng.lml(_lib.KERNEL_PER, theta, 0.0, mu)  # nothing declared yet
    eng.set_periodic([1])
    want, info = eng.lml(_lib.KERNEL_PER, theta, 0.0, mu)
    assert info == 0 and np.isfinite(want)
    for dims, n, text in (([1], 0, b"1 to 8"), (list(range(9)), None, b"1 to 8"), ([1, 1], None, b"ascending"),
                          ([2, 0], None, b"ascending"), ([0, 3], None, b"outside"), ([-1], None, b"outside")):
        assert set_periodic(h, dims, n) == ERR_ARG
        assert text in h.lib.gpmi_last_error(h.ctx), (dims, h.lib.gpmi_last_error(h.ctx))
        got, info = eng.lml(_lib.KERNEL_PER, theta, 0.0, mu)  # the handle is usable, the earlier declaration in force
        assert info == 0 and got == want
    assert h.lib.gpmi_set_periodic(h.ctx, 1, None) == ERR_ARG and b"NULL" in h.lib.gpmi_last_error(h.ctx)
    with pytest.raises(_lib.GpmiError, match="n_theta"):
        eng.lml(_lib.KERNEL_PER, theta[:-1], 0.0, mu)
    assert eng.lml(_lib.KERNEL_PER, theta, 0.0, mu)[0] == want
    # the entry points without the kernel refuse it, alone and inside the declared sum, before anything is launched
    with pytest.raises(_lib.GpmiError, match="GPMI_KERNEL_PER is not supported"):
        eng.lml_hessian(_lib.KERNEL_PER, theta, 0.0, mu)
    eng.mt_set_targets(np.stack([y, 2 * y], axis=1))
    with pytest.raises(_lib.GpmiError, match="GPMI_KERNEL_PER is not supported"):
        eng.mt_lml(_lib.KERNEL_PER, theta, 0.0)
    eng.set_sum([_lib.KERNEL_SE, _lib.KERNEL_PER])
    both = np.concatenate([mh.theta_for("se", 3), theta])
    with pytest.raises(_lib.GpmiError, match="GPMI_KERNEL_PER is not supported"):
        eng.mt_lml(_lib.KERNEL_SUM, both, 0.0)
    value, info = eng.lml(_lib.KERNEL_SUM, both, 0.0, mu)
    assert info == 0 and np.isfinite(value)
    assert eng.lml(_lib.KERNEL_PER, theta, 0.0, mu)[0] == want
    eng.close()


# ------------------------------------------------------------------------------------------------ 10. further checks
def test_under_and_overflowing_periods_and_scales():
    from numpy.linalg import LinAlgError

    parts = [("per", [1])]
    x, y, e = ph.dataset(65, 3)
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    before = gp.marginal_likelihood(theta)
    alpha = gp.alpha.copy()
    for index, value, must_fail in ((5, -800.0, True), (3, -800.0, True), (2, -800.0, True), (5, 800.0, False)):
        bad = theta.copy()
        bad[index] = value  # [mean, ln a, ln l_0, ln l_1, ln l_2, ln p_1]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            v = gp.marginal_likelihood(bad)
            row = gp.marginal_likelihood_batch(np.array([theta, bad]))
        assert not np.isnan(v) and not np.isnan(row).any()
        check(row[0], before, what="the good row beside it")
        if must_fail:
            assert v == -1e50 and row[1] == -1e50
            with pytest.raises(LinAlgError):
                gp.set_hyperparameters(bad)
        else:  # p -> inf: K = a^2 on the periodic dimension, a finite value or the sentinel
            assert np.isfinite(v) and np.isfinite(row[1])
            try:
                gp.set_hyperparameters(bad)
            except LinAlgError:
                pass
        gp.set_hyperparameters(theta)  # the next call is right
        assert gp.marginal_likelihood(theta) == before and np.array_equal(gp.alpha, alpha)


def test_nine_periodic_dimensions_raise():
    from inference_amd.gp import GpRegressor, Periodic

    x, y, e = ph.dataset(20, 9)
    with pytest.raises(ValueError, match="at most 8"):
        GpRegressor(x, y, y_err=e, kernel=Periodic(periodic_dims=list(range(9))), hyperpars=np.zeros(20))
    with pytest.raises(ValueError, match="at most 8"):
        GpRegressor(x, y, y_err=e, kernel=Periodic(), hyperpars=np.zeros(20))


def test_hessian_exact_raises_and_auto_is_fd():
    parts = [("per", [0]), ("wn",)]
    x, y, e = ph.dataset(65, 2)
    theta = _theta(parts, x)
    gp = _gp(parts, x, y, e, theta)
    with pytest.raises(NotImplementedError, match="exact Hessian"):
        gp.marginal_likelihood_hessian(theta, method="exact")
    auto = gp.marginal_likelihood_hessian(theta)
    fd = gp.marginal_likelihood_hessian(theta, method="fd")
    assert auto[0] == fd[0] and np.array_equal(auto[1], fd[1]) and np.array_equal(auto[2], fd[2])
    assert np.array_equal(fd[2], fd[2].T) and not np.isnan(fd[2]).any()


def test_repeats_are_bit_identical_and_other_thetas_leave_the_fit_alone():
    parts = [("per", [1]), ("wn",)]
    x, y, e = ph.dataset(130, 3)
    pts = np.random.default_rng(8).uniform(0.0, ph.SPAN, size=(33, 3))
    theta = _theta(parts, x)
    other = theta + 0.1
    gp = _gp(parts, x, y, e, theta)

    def everything():
        out = [gp.K_xx.copy(), gp.alpha.copy(), gp.L.copy(), *gp(pts), *gp.build_posterior(pts), *gp.spatial_derivatives(pts),
               *gp.gradient(pts[:5])]
        for t in (theta, other):
            out += [np.float64(gp.marginal_likelihood(t)), *gp.marginal_likelihood_gradient(t), np.float64(gp.loo_likelihood(t)),
                    *gp.loo_likelihood_gradient(t)]
        out += [gp.marginal_likelihood_batch(np.array([theta, other])), *gp.marginal_likelihood_gradient_batch(np.array([theta, other])),
                *gp.predict_marginalised(pts, np.array([theta, other]))]
        return out

    first = everything()
    second = everything()
    assert len(first) == len(second)
    for i, (a, b) in enumerate(zip(first, second)):
        assert np.array_equal(np.asarray(a), np.asarray(b)), f"result {i} differs between two identical calls"
    fresh = _gp(parts, x, y, e, theta)
    assert np.array_equal(fresh.alpha, gp.alpha) and np.array_equal(fresh.L, gp.L)
    m1, m2 = fresh(pts), gp(pts)
    assert np.array_equal(m1[0], m2[0]) and np.array_equal(m1[1], m2[1])
