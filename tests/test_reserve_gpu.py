"""
GPU tests of regressors with reserved device capacity and of handles that `add_point` has grown, through every entry point
(the cases, their edges and the builders: tests/reserve_host.py; the yardstick on its own: tests/test_reserve_cpu.py).

Two properties hold on such handles that hold nowhere else in the suite: whole tiles of identity padding (np - n >= 128),
and an n that changed under a live handle - workspaces, lanes, the cached 512-wide inverse blocks and the Python caches
were created at another n.

  (a) entry points that rebuild K in a scratch lane never read the fitted factor: the grown handle and its twin (same n,
      same np, never appended to) return identical doubles - `np.array_equal`, no tolerance;
  (b) everything against the oracle of tests/matern_host.py on the final data (the Hessian: the long-double mirror of
      tests/hessian_host.py), at the project's tolerances for the same quantities (tests/test_dimensions_gpu.py: `check`
      1e-10 of the largest element, `check_each` 1e-7 element-wise above the 1e-6 floor, 1e-13 for elements of K; the
      Hessian file's TOL with its ripple allowance; the draws: ten times the oracle's own spread under 48 ripples of 1e-13,
      as tests/test_draws_gpu.py);
  (c) the device's own failure path of gpmi_append_point (pivot <= 0) leaves the handle as it was, in every bit;
  (d) GpOptimiser(reuse_hyperpars=True) maximises its acquisition on an appended model;
  (e) the rebuild (ChangePoint) and the refusals (HeteroscedasticNoise, dense y_cov) of `add_point`.

Every comparison prints its achieved error.
"""
import copy

import numpy as np
import pytest
from scipy.linalg import solve_triangular
from scipy.special import erfc

import draws_host as dh
import hessian_host as hh
import matern_host as mh
import reserve_host as rh
from test_dimensions_gpu import REFUSAL, check, check_each
from test_hessian_gpu import assert_parity

pytestmark = pytest.mark.gpu

JITTER = 1e-9
_cache = {}


def subject(name):
    """The handle under test of a case, built once: grown by its appends, rebuilt by `add_point` (cp_130), or reserve-only."""
    if ("subject", name) not in _cache:
        c = rh.CASES[name]
        gp = rh.regressor(name, c.n0, c.reserve)
        assert gp.engine.capacity() == rh.capacity(name) and gp.engine.n == c.n0
        if c.appends:
            rh.append(gp, name)
        _cache[("subject", name)] = gp
    return _cache[("subject", name)]


def twin_of(name):
    if ("twin", name) not in _cache:
        _cache[("twin", name)] = rh.twin(name, subject(name).engine.capacity())
    return _cache[("twin", name)]


def oracle(name):
    if ("oracle", name) not in _cache:
        _cache[("oracle", name)] = rh.oracle(name)
    return _cache[("oracle", name)]


def queries(name, m, seed=0):
    x = rh.inputs(name)[0]
    u = np.random.default_rng(seed + m).uniform(0.0, 4.0, size=(m, x.shape[1]))
    u[0] = x[2]  # a query point on a training point
    return u


def thetas_of(name):
    return rh.thetas_around(name)[:1 if name == "m32_2040" else 3]


# ------------------------------------------------------------------------------------------------ (a) grown == twin
def scratch_lane_results(gp, name, thetas, pts):
    """Every entry point that rebuilds K from (x, y, noise, n, np, theta), as {label: array}."""
    out = {}
    for t, th in enumerate(thetas):
        out[f"lml[{t}]"] = gp.marginal_likelihood(th)
        out[f"lml gradient[{t}]"] = np.concatenate([[v] if np.ndim(v) == 0 else v for v in gp.marginal_likelihood_gradient(th)])
        out[f"loo[{t}]"] = gp.loo_likelihood(th)
        out[f"loo gradient[{t}]"] = np.concatenate([[v] if np.ndim(v) == 0 else v for v in gp.loo_likelihood_gradient(th)])
    out["lml batch"] = gp.marginal_likelihood_batch(thetas)
    out["lml gradient batch: values"], out["lml gradient batch: gradients"] = gp.marginal_likelihood_gradient_batch(thetas)
    out["loo gradient batch: values"], out["loo gradient batch: gradients"] = gp.loo_likelihood_gradient_batch(thetas)
    if gp.async_batches():
        gp.marginal_likelihood_batch_submit(thetas, 0)
        gp.marginal_likelihood_batch_submit(thetas[::-1], 1)
        out["submit / wait, slot 0"] = gp.marginal_likelihood_batch_wait(0)
        out["submit / wait, slot 1"] = gp.marginal_likelihood_batch_wait(1)[::-1]
    if gp._lockstep_predict_ok():
        out["predict_samples: means"], out["predict_samples: sigmas"] = gp.predict_samples(pts, thetas)
        out["predict_marginalised: mean"], out["predict_marginalised: sigma"] = gp.predict_marginalised(pts, thetas)
    if rh.hessian_kind(name):
        for t, th in enumerate(thetas):
            lml, grad, H = gp.marginal_likelihood_hessian(th, method="exact")
            out[f"hessian[{t}]"] = np.concatenate([[lml], grad, H.ravel()])
    return {k: np.asarray(v, dtype=float) for k, v in out.items()}


@pytest.mark.parametrize("name", rh.GROWN)
def test_grown_equals_twin_bit_for_bit(name):
    grown, twin = subject(name), twin_of(name)
    assert grown.engine.capacity() == twin.engine.capacity() == rh.capacity(name)
    assert grown.engine.n == twin.engine.n == grown.n_points == twin.n_points
    assert np.array_equal(grown.x, twin.x) and np.array_equal(grown.y, twin.y) and np.array_equal(grown._noise_var, twin._noise_var)
    assert grown.async_batches() and grown._lockstep_predict_ok()
    thetas = rh.thetas_around(name)
    pts = queries(name, 9)
    a, b = scratch_lane_results(grown, name, thetas, pts), scratch_lane_results(twin, name, thetas, pts)
    assert list(a) == list(b) and len(a) >= 23
    bad = []
    for key in a:
        assert a[key].shape == b[key].shape and np.isfinite(a[key]).all(), key
        same = np.array_equal(a[key], b[key])
        print(f"{name} {key}: {'identical' if same else 'DIFFERENT, max |grown - twin| = %.2e' % np.abs(a[key] - b[key]).max()}")
        if not same:
            bad.append(key)
    assert not bad, f"{name}: the grown handle and its twin differ in {bad}"
    # what a slot returns is what the synchronous batch returns
    assert np.array_equal(a["submit / wait, slot 0"], a["lml batch"]) and np.array_equal(a["submit / wait, slot 1"], a["lml batch"])


# ------------------------------------------------------------------------------------------------ (b) against the oracle
def gradient_oracle(name, orc):
    """The oracle as its predictive-gradient methods need it: theta ends with the kernel's own parameters."""
    cut = copy.copy(orc)
    cut.theta = orc.theta[:orc.nm + rh.CASES[name].d + 1]
    return cut


def check_fitted_state(name, gp, orc):
    c = rh.CASES[name]
    w = name
    assert gp._generic is False and gp.n_points == orc.n == gp.engine.n
    check(gp.K_xx, orc.K, 1e-13, f"{w} K_xx")
    L = gp.L
    assert L.shape == (orc.n, orc.n) and np.all(np.triu(L, 1) == 0.0)
    check(L, orc.L, what=f"{w} L")
    check_each(gp.alpha, orc.alpha, what=f"{w} alpha")
    check(gp._logdet, np.log(np.diag(orc.L)).sum(), what=f"{w} log-determinant")
    pts = queries(name, 40)
    mu, sig = gp(pts)
    omu, osig = orc(pts)
    check(mu, omu, what=f"{w} mu")
    check(sig, osig, what=f"{w} sigma")
    pm, pc = gp.build_posterior(pts[:16])
    om, oc = orc.build_posterior(pts[:16])
    check(pm, om, what=f"{w} posterior mean")
    check(pc, oc, what=f"{w} posterior covariance")
    # leave-one-out predictions, R&W eq. 5.12
    iL = solve_triangular(orc.L, np.eye(orc.n), lower=True)
    var = 1.0 / (iL**2).sum(axis=0)
    lm, ls = gp.loo_predictions()
    check(lm, orc.y - orc.alpha * var, what=f"{w} loo means")
    check(ls, np.sqrt(var), what=f"{w} loo sigmas")
    # joint draws with the caller's normals: mean + z chol(cov + jitter I)^T of the oracle's posterior, with the allowance and
    # the two conditions of tests/test_draws_gpu.py: the allowance itself below 1e-9, and the oracle's own rounding (its
    # draws from the Sigma of a long-double solve on the same K; an O(N^3) host loop, left out at N = 2045) inside its
    # ripple spread.  Neither holds at the points above: inside the data the variance is 1e-3 of the prior's, Sigma carries
    # an absolute error of a few ulp of a^2 and the oracle's own draws are off by up to 20 spreads (rq_510: 3.8e-12 against
    # 1.9e-13); 16 points on a line make Sigma + eps I numerically singular (cond 4e9).  Four points across the edge of the
    # data, in [3.5, 5.5]^d, have variances between 1e-3 of the prior's and all of it, and meet both in every case.
    pd_ = 3.5 + 0.5 * pts[:4]
    om, oc = orc.build_posterior(pd_)
    rng = np.random.default_rng(orc.n)
    z = rng.standard_normal((4, 4))
    base = dh.draws_oracle(om, oc, JITTER, z)
    spread = 0.0
    for _ in range(48):
        r = rng.uniform(-1.0, 1.0, oc.shape)
        r = np.triu(r) + np.triu(r, 1).T
        spread = max(spread, float(np.abs(dh.draws_oracle(om, oc * (1.0 + 1e-13 * r), JITTER, z) - base).max()))
    allowance = 10.0 * spread
    assert 0.0 < allowance < 1e-9, allowance
    own = float("nan")
    if orc.n <= 600:
        th = orc.theta[orc.nm:]
        S_ld = dh.posterior_covariance_longdouble(orc.K, orc.m.cross(pd_, orc.x, th), orc.m.cross(pd_, pd_, th))
        own = float(np.abs(dh.draws_oracle(om, S_ld, JITTER, z) - base).max())
        assert own <= spread, f"{w}: the oracle's own rounding moves its draws by {own:.2e}, its ripples by {spread:.2e}"
    err = float(np.abs(gp.sample_posterior(pd_, 4, z=z, jitter=JITTER) - base).max())
    print(f"{w} draws vs oracle: {err:.3e}, allowance {allowance:.3e} (10 x the oracle's spread under 48 ripples of 1e-13); the "
          f"oracle against its long-double Sigma: {own:.3e}")
    assert err <= allowance
    # predictive gradients at one point and at one point more than a chunk of 1024 // d
    kind = rh.gradient_kind(name)
    if kind is None:
        for call in (gp.gradient, gp.spatial_derivatives, gp.spatial_derivatives_batch):
            with pytest.raises(NotImplementedError, match=REFUSAL):
                call(pts[:2])
        return
    cut = gradient_oracle(name, orc)
    for m in (1, 1024 // c.d + 1):
        q = queries(name, m, seed=7)
        omu, ocov = cut.gradient(q, kind)
        odmu, odvar = cut.spatial_derivatives(q, kind)
        gmu, gcov = gp.gradient(q)
        dmu, dvar = gp.spatial_derivatives(q)
        bmu, bvar = gp.spatial_derivatives_batch(q)
        assert bmu.shape == bvar.shape == (m, c.d)
        check(gmu.reshape(m, c.d), omu, what=f"{w} m={m} gradient mean")
        check(gcov.reshape(m, c.d, c.d), ocov, what=f"{w} m={m} gradient covariance")
        check(dmu.reshape(m, c.d), odmu, what=f"{w} m={m} d mu / dx")
        check(dvar.reshape(m, c.d), odvar, what=f"{w} m={m} d var / dx")
        check(bmu, odmu, what=f"{w} m={m} d mu / dx (batch form)")
        check(bvar, odvar, what=f"{w} m={m} d var / dx (batch form)")


def hessian_mirror(name, gp, theta):
    """(mirror in long double, its arguments) of a case at `theta`, in the layout of `hyperpars`."""
    c = rh.CASES[name]
    x, y, e, _ = rh.inputs(name)
    nm = rh.n_mean(name)
    wn = c.parts[-1][0] == "wn"
    phi = np.array(gp.mean.mean_and_gradients(theta[gp.mean_slice])[1])
    args = (rh.hessian_kind(name), x, y, e**2, theta[:nm], phi, theta[nm: len(theta) - (1 if wn else 0)], theta[-1] if wn else None)
    return hh.hessian(*args, dtype=np.longdouble), args


def check_scratch_lanes(name, gp, orc):
    w = name
    thetas = thetas_of(name)
    T, P = thetas.shape
    ref = [(orc.marginal_likelihood_gradient(th), orc.loo_likelihood_gradient(th)) for th in thetas]
    for t, th in enumerate(thetas):
        (ov, og), (olv, olg) = ref[t]
        check(gp.marginal_likelihood(th), ov, what=f"{w} lml [{t}]")
        v, g = gp.marginal_likelihood_gradient(th)
        assert g.shape == (P,)
        check(v, ov, what=f"{w} lml (gradient call) [{t}]")
        check_each(g, og, what=f"{w} lml gradient [{t}]")
        check(gp.loo_likelihood(th), olv, what=f"{w} loo [{t}]")
        v, g = gp.loo_likelihood_gradient(th)
        check(v, olv, what=f"{w} loo (gradient call) [{t}]")
        check_each(g, olg, what=f"{w} loo gradient [{t}]")
    if name == "m32_2040":  # the host oracles are O(N^3): the single evaluations alone at N = 2045
        return
    o_lml, o_g = np.array([r[0][0] for r in ref]), np.array([r[0][1] for r in ref])
    o_loo, o_lg = np.array([r[1][0] for r in ref]), np.array([r[1][1] for r in ref])
    check(gp.marginal_likelihood_batch(thetas), o_lml, what=f"{w} lml batch")
    gv, gg = gp.marginal_likelihood_gradient_batch(thetas)
    lv, lg = gp.loo_likelihood_gradient_batch(thetas)
    assert gv.shape == lv.shape == (T,) and gg.shape == lg.shape == (T, P)
    check(gv, o_lml, what=f"{w} lml gradient batch: values")
    check(lv, o_loo, what=f"{w} loo gradient batch: values")
    for t in range(T):
        check_each(gg[t], o_g[t], what=f"{w} lml gradient batch [{t}]")
        check_each(lg[t], o_lg[t], what=f"{w} loo gradient batch [{t}]")
    if gp.async_batches():
        gp.marginal_likelihood_batch_submit(thetas, 0)
        gp.marginal_likelihood_batch_submit(thetas[::-1], 1)
        check(gp.marginal_likelihood_batch_wait(0), o_lml, what=f"{w} submit / wait, slot 0")
        check(gp.marginal_likelihood_batch_wait(1), o_lml[::-1], what=f"{w} submit / wait, slot 1")
    if gp._lockstep_predict_ok():
        c = rh.CASES[name]
        x, y, e, _ = rh.inputs(name)
        q = queries(name, 9)
        each = [mh.OracleGp(x, y, e, orc.m, th, mean=orc.mean)(q) for th in thetas]
        om, os_ = np.array([r[0] for r in each]), np.array([r[1] for r in each])
        means, sigs = gp.predict_samples(q, thetas)
        mix_mu, mix_sig = gp.predict_marginalised(q, thetas)
        check(means, om, what=f"{w} predict_samples: means")
        check(sigs, os_, what=f"{w} predict_samples: sigmas")
        mean = om.mean(axis=0)
        check(mix_mu, mean, what=f"{w} predict_marginalised: mean")
        check(mix_sig, np.sqrt((os_**2 + (om - mean) ** 2).mean(axis=0)), what=f"{w} predict_marginalised: sigma")
    if rh.hessian_kind(name):
        th = thetas[0]
        lml, grad, H = gp.marginal_likelihood_hessian(th, method="exact")
        mirror, args = hessian_mirror(name, gp, th)
        assert H.shape == (P, P) and np.array_equal(H, H.T) and np.isfinite(H).all()
        check(lml, mirror["lml"], what=f"{w} hessian call: lml")
        g_ref = np.asarray(mirror["grad"], dtype=float)
        assert np.abs(grad - g_ref).max() <= 1e-10 * max(np.abs(g_ref).max(), 1.0)
        assert_parity(f"{w} hessian", H, mirror, args)
    else:
        with pytest.raises(NotImplementedError, match="fd"):
            gp.marginal_likelihood_hessian(thetas[0], method="exact")


@pytest.mark.parametrize("name", list(rh.CASES))
def test_fitted_state_against_the_oracle(name):
    check_fitted_state(name, subject(name), oracle(name))


@pytest.mark.parametrize("name", list(rh.CASES))
def test_scratch_lane_entry_points_against_the_oracle(name):
    gp = subject(name)
    hyper = np.array(gp.hyperpars)
    check_scratch_lanes(name, gp, oracle(name))
    assert np.array_equal(gp.hyperpars, hyper)
    check_each(gp.alpha, oracle(name).alpha, what=f"{name} alpha after the likelihood evaluations")
    mu, _ = gp(queries(name, 40))
    check(mu, oracle(name)(queries(name, 40))[0], what=f"{name} mu after the likelihood evaluations")


@pytest.mark.parametrize("name", rh.GROWN)
def test_grown_against_the_tight_handle(name):
    """The same data without any padding beyond the tile: a third handle, the usual one of every other test file."""
    grown, tight = subject(name), rh.tight(name)
    assert tight.engine.capacity() == rh.round_up(grown.n_points) <= grown.engine.capacity()
    check_each(grown.alpha, tight.alpha, what=f"{name} alpha: grown vs tight")
    check(grown._logdet, tight._logdet, what=f"{name} log-determinant: grown vs tight")
    pts = queries(name, 40)
    for a, b, what in zip(grown(pts), tight(pts), ("mu", "sigma")):
        check(a, b, what=f"{name} {what}: grown vs tight")
    tight.engine.close()


# ------------------------------------------------------------------------------------------------ (c) the failure path
def test_failed_append_on_the_device_leaves_every_bit():
    """A new point whose data variance is -(prior variance + 1): K_nn = a^2 (1 + 1e-12) + noise < 0 whatever l . l is, so
    the pivot K_nn - l . l is <= 0.  gpmi_append_point reports info = n + 1 with GPMI_OK and must have changed nothing;
    the valid appends after it give the bits of a handle that never saw the failure."""
    name = "se_62"
    c = rh.CASES[name]
    x, y, e, theta = rh.inputs(name)
    gp, clean = rh.regressor(name, c.n0, c.reserve), rh.regressor(name, c.n0, c.reserve)
    pts = queries(name, 40)
    th = rh.thetas_around(name)[0]

    def state(g):
        return (g.engine.get_L(), *g(pts), *g.marginal_likelihood_gradient(th), np.array(g.alpha))

    before = state(gp)
    prior_var = float(np.exp(2.0 * theta[1]))
    _, _, info = gp.engine.append_point(x[c.n0], y[c.n0], -(prior_var + 1.0), np.full(c.n0 + 1, theta[0]))
    assert info == c.n0 + 1
    assert gp.engine.n == c.n0 and gp.engine.capacity() == rh.capacity(name) and gp.engine.x.shape == (c.n0, c.d)
    after = state(gp)
    for a, b, what in zip(before, after, ("L", "mu", "sigma", "lml", "lml gradient", "alpha")):
        assert np.array_equal(a, b), f"{what} changed after a failed append (max {np.abs(np.asarray(a) - np.asarray(b)).max():.2e})"
    rh.append(gp, name)
    rh.append(clean, name)
    assert gp.engine.n == clean.engine.n == c.n0 + c.appends
    for a, b, what in zip(state(gp), state(clean), ("L", "mu", "sigma", "lml", "lml gradient", "alpha")):
        assert np.array_equal(a, b), f"{what} after a failed and {c.appends} valid appends differs from {c.appends} valid appends"
    check_each(gp.alpha, oracle(name).alpha, what="alpha after a failed and the valid appends")
    for a, b, what in zip(gp(pts), oracle(name)(pts), ("mu", "sigma")):  # (the two handles share their history of predictions)
        check(a, b, what=f"{what} after a failed and the valid appends")
    gp.engine.close()
    clean.engine.close()


# ------------------------------------------------------------------------------------------------ (d) GpOptimiser
def _acquisition_on_host(tag, mu, sig, dmu, dvar, y_max, kappa=2.0):
    """(-acquisition objective, its gradient) from the formulas: UCB = mu + kappa sigma; EI = sigma (Z Phi(Z) + phi(Z)),
    Z = (mu - y_max) / sigma, the objective its logarithm."""
    dsig = 0.5 * dvar / sig[:, None]
    if tag == "ucb":
        return -(mu + kappa * sig), -(dmu + kappa * dsig)
    Z = (mu - y_max) / sig
    pdf, cdf = np.exp(-0.5 * Z**2) / np.sqrt(2.0 * np.pi), 0.5 * erfc(-Z / np.sqrt(2.0))  # (erfc: Phi(-13) = 6e-39 is below the
    # rounding of 1 + erf; Z Phi + phi ~ phi / Z^2 then loses Z^2 ulp to cancellation, 2e-14 at Z = -13)
    EI = sig * (Z * cdf + pdf)
    return -np.log(EI), -(pdf[:, None] * dsig + cdf[:, None] * dmu) / EI[:, None]  # dEI = Phi dmu + phi dsigma


@pytest.mark.parametrize("tag", ["ei", "ucb"])
def test_gp_optimiser_acquisition_on_an_appended_model(tag):
    import inference_amd.gp as gp_mod
    from test_gpu_parity import _bo_problem

    bx, by, bounds = _bo_problem()
    e = np.full(by.size, 0.1)
    th = np.array([by.mean(), np.log(by.std()), np.log(2.0), np.log(2.0)])
    acq = {"ei": gp_mod.ExpectedImprovement, "ucb": gp_mod.UpperConfidenceBound}[tag]
    opt = gp_mod.GpOptimiser(bx, by, bounds=bounds, y_err=e, hyperpars=th, acquisition=acq, reuse_hyperpars=True)
    assert opt.gp.engine.capacity() == rh.round_up(by.size + 256) == 384
    handle = opt.gp.engine
    new = np.array([[-2.0, 3.0], [4.5, -1.5], [1.0, 4.0]])
    for p in new:
        opt.add_evaluation(p, float(np.sin(p[0]) + 0.1 * p[1]), 0.1)
    n = by.size + 3
    assert opt.gp.engine is handle and handle.n == n == opt.y.size and np.array_equal(opt.gp.hyperpars, th), "appended, not re-fitted"
    assert opt.acquisition.gp is opt.gp and opt.acquisition.mu_max == opt.y.max()
    orc = mh.OracleGp(opt.x, opt.y, opt.y_err, mh.HostModel([("se",)], opt.x), th)
    cond = float(np.linalg.cond(orc.K))
    print(f"{tag}: cond(K + sig) = {cond:.2e}")
    assert cond <= rh.COND_MAX
    lo, hi = np.array(bounds).T
    pts = np.random.default_rng(20).uniform(lo, hi, size=(20, 2))
    val, grad = opt.acquisition.opt_func_gradient_batch(pts)
    assert val.shape == (20,) and grad.shape == (20, 2)
    fresh = gp_mod.GpRegressor(opt.x, opt.y, y_err=opt.y_err, hyperpars=th)
    assert fresh.engine.capacity() == 128
    other = acq()
    other.update_gp(fresh)
    fval, fgrad = other.opt_func_gradient_batch(pts)
    check(val, fval, what=f"{tag} objective: appended vs fresh model")
    check(grad, fgrad, what=f"{tag} gradient: appended vs fresh model")
    mu, sig = orc(pts)
    dmu, dvar = orc.spatial_derivatives(pts, "se")
    oval, ograd = _acquisition_on_host(tag, mu, sig, dmu, dvar, opt.y.max())
    check(val, oval, what=f"{tag} objective: appended model vs oracle")
    check(grad, ograd, what=f"{tag} gradient: appended model vs oracle")
    check(opt.acquisition.opt_func_batch(pts), oval, what=f"{tag} objective (value call) vs oracle")
    fresh.engine.close()
    handle.close()


# ------------------------------------------------------------------------------------------------ (e) rebuild and refusals
def test_change_point_add_point_rebuilds_with_the_reserve():
    """cp_130: `add_point` closes the handle and re-fits on 131 points with the reserve it had (>= 128); the rebuilt model is
    the subject of the oracle comparisons above."""
    name = "cp_130"
    c = rh.CASES[name]
    gp = rh.regressor(name, c.n0, c.reserve)
    first = gp.engine
    assert first.capacity() == rh.round_up(c.n0 + c.reserve) == 512
    rh.append(gp, name)
    assert gp.engine is not first and gp._reserve == 256
    assert gp.engine.n == 131 and gp.engine.capacity() == rh.round_up(131 + 256) == 512
    sub = subject(name)
    assert sub.engine.capacity() == 512 and sub.engine.n == 131
    assert np.array_equal(gp.alpha, sub.alpha), "two rebuilds on the same data"
    check_each(gp.alpha, oracle(name).alpha, what=f"{name} alpha after the rebuild")
    gp.engine.close()


@pytest.mark.parametrize("name,match", [("het_96", "HeteroscedasticNoise"), ("ycov_100", "dense y_cov")])
def test_refused_add_point_leaves_the_model_unchanged(name, match):
    c = rh.CASES[name]
    gp = subject(name)
    handle = gp.engine
    pts = queries(name, 40)
    before = (*gp(pts), np.array(gp.alpha), gp.engine.get_L())
    new = (np.full(c.d, 1.5), 0.3) + (() if name == "ycov_100" else (0.1,))
    with pytest.raises(NotImplementedError, match=match):
        gp.add_point(*new)
    assert gp.engine is handle and handle.n == c.n0 == gp.n_points and handle.capacity() == rh.capacity(name)
    after = (*gp(pts), np.array(gp.alpha), gp.engine.get_L())
    for a, b, what in zip(before, after, ("mu", "sigma", "alpha", "L")):
        assert np.array_equal(a, b), f"{name}: {what} changed after a refused add_point"
