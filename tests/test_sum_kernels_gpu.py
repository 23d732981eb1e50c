"""
GPU tests of sums of stationary covariance kernels (GPMI_KERNEL_SUM: the fused sum K-build of csrc/kbuild.hip and the
fused sum gradient contraction of csrc/grad.hip) through the whole GpRegressor surface: against the reference's values
(tests/golden/sum.npz), against independent routes to the same model (a NumPy computation, the mixture kernels with all
window weights 1), batched against single evaluations, and run against run.  Every test runs with the engine's dense
host-composition entry points (`*_dense`) made to raise, so that a fallback off the fused device path fails.
"""
import os

import numpy as np
import pytest

import workloads as wl

pytestmark = pytest.mark.gpu

RTOL = 1e-10
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, tol=RTOL, what=""):
    r = rel(a, b)
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"
    return r


@pytest.fixture(autouse=True)
def no_dense_path(monkeypatch):
    from inference_amd._engine import GpEngine

    def tripwire(name):
        def fail(*args, **kwargs):
            raise AssertionError(f"GpEngine.{name} called: a sum of kernels left the fused device path")

        return fail

    for name in dir(GpEngine):
        if name.endswith("_dense"):
            monkeypatch.setattr(GpEngine, name, tripwire(name))


@pytest.fixture(scope="module")
def gsum():
    return np.load(os.path.join(ROOT, "tests", "golden", "sum.npz"))


def _cov(kinds):
    from inference_amd.gp import RationalQuadratic, SquaredExponential, WhiteNoise

    parts = [{"se": SquaredExponential, "rq": RationalQuadratic, "wn": WhiteNoise}[k]() for k in kinds]
    cov = parts[0]
    for p in parts[1:]:
        cov = cov + p
    return cov


CASES = {
    "serq": ("se", "rq"),
    "sese": ("se", "se"),
    "serqwn": ("se", "rq", "wn"),
    "rqsesewn": ("rq", "se", "se", "wn"),
}


def _model(g, tag, hyperpars=None, **kw):
    from inference_amd.gp import GpRegressor

    th = g[f"{tag}_thetas"][0] if hyperpars is None else hyperpars
    return GpRegressor(g[f"{tag}_x"], g[f"{tag}_y"], y_err=g[f"{tag}_y_err"], kernel=_cov(CASES[tag]), hyperpars=th, **kw)


@pytest.mark.parametrize("tag", list(CASES))
def test_sum_matches_reference(gsum, tag):
    from inference_amd import _lib

    g = gsum
    gp = _model(g, tag)
    assert gp._kernel_id == _lib.KERNEL_SUM and not gp._generic
    assert gp.hyperpar_labels == list(g[f"{tag}_labels"])
    check(np.array(gp.hp_bounds, dtype=float), g[f"{tag}_bounds"], 1e-12, "bounds")
    if f"{tag}_K_xx" in g.files:
        check(gp.K_xx, g[f"{tag}_K_xx"], 1e-13, "K_xx")
    check(gp.alpha, g[f"{tag}_alpha"], what="alpha")
    pts = g[f"{tag}_pts"]
    mu, sig = gp(pts)
    check(mu, g[f"{tag}_mu"], what="mu")
    check(sig, g[f"{tag}_sig"], what="sigma")
    pm, pc = gp.build_posterior(pts[:16])
    check(pm, g[f"{tag}_post_mu"], what="posterior mean")
    check(pc, g[f"{tag}_post_cov"], what="posterior covariance")
    lm, ls = gp.loo_predictions()
    check(lm, g[f"{tag}_loo_mu"], what="loo mu")
    check(ls, g[f"{tag}_loo_sig"], what="loo sigma")
    thetas = g[f"{tag}_thetas"]
    check([gp.marginal_likelihood(t) for t in thetas], g[f"{tag}_lml"], what="lml")
    check(np.array([gp.marginal_likelihood_gradient(t)[1] for t in thetas]), g[f"{tag}_lml_grad"], what="lml gradient")
    check([gp.loo_likelihood(t) for t in thetas], g[f"{tag}_loo"], what="loo")
    check(np.array([gp.loo_likelihood_gradient(t)[1] for t in thetas]), g[f"{tag}_loo_grad"], what="loo gradient")
    # batched forms (lockstep at these sizes) against the reference as well
    check(gp.marginal_likelihood_batch(thetas), g[f"{tag}_lml"], what="lml batch")
    check(gp.marginal_likelihood_gradient_batch(thetas)[1], g[f"{tag}_lml_grad"], what="lml gradient batch")
    check(gp.loo_likelihood_gradient_batch(thetas)[1], g[f"{tag}_loo_grad"], what="loo gradient batch")


@pytest.mark.parametrize("tag", list(CASES))
def test_seeded_search_reaches_reference(gsum, tag):
    from inference_amd.gp import GpRegressor

    g = gsum
    np.random.seed(7)
    gp = GpRegressor(g[f"{tag}_x"], g[f"{tag}_y"], y_err=g[f"{tag}_y_err"], kernel=_cov(CASES[tag]), n_starts=3)
    check(gp.marginal_likelihood(gp.hyperpars), g[f"{tag}_search_lml"], 1e-10, "search lml")
    # the reference's theta* scores the same on the device: both searches ended at the same optimum
    check(gp.marginal_likelihood(g[f"{tag}_search_theta"]), g[f"{tag}_search_lml"], 1e-10, "lml at the reference's theta*")
    # L-BFGS-B stops within its own convergence test (factr 1e7: ~2e-9 relative in the objective), so theta* agrees to
    # the flatness of the optimum, not to the last digits: measured 7e-6 normwise for serqwn (mean and WhiteNoise
    # parameters; the RQ shape and the WhiteNoise at their bounds), <= 1e-6 for the others
    check(np.asarray(gp.hyperpars, float), g[f"{tag}_search_theta"], 1e-4, "search theta")


def test_batches_equal_single_evaluations(gsum):
    g = gsum
    gp = _model(g, "rqsesewn")
    base = g["rqsesewn_thetas"]
    rng = np.random.default_rng(5)
    for T in (3, 7, 18):
        thetas = base[rng.integers(0, 3, T)] + 0.02 * rng.standard_normal((T, base.shape[1]))
        vals = gp.marginal_likelihood_batch(thetas)
        single = np.array([gp.marginal_likelihood(t) for t in thetas])
        check(vals, single, 1e-12, f"lml batch T={T}")
        lml, grads = gp.marginal_likelihood_gradient_batch(thetas)
        sg = [gp.marginal_likelihood_gradient(t) for t in thetas]
        check(lml, [s[0] for s in sg], 1e-12, f"lml (gradient batch) T={T}")
        check(grads, np.array([s[1] for s in sg]), 1e-12, f"lml gradient batch T={T}")
        lv, lg = gp.loo_likelihood_gradient_batch(thetas)
        sl = [gp.loo_likelihood_gradient(t) for t in thetas]
        check(lv, [s[0] for s in sl], 1e-12, f"loo (gradient batch) T={T}")
        check(lg, np.array([s[1] for s in sl]), 1e-12, f"loo gradient batch T={T}")


def test_failing_member_does_not_disturb_neighbours(gsum):
    g = gsum
    gp = _model(g, "serq")
    thetas = np.array(g["serq_thetas"])
    bad = thetas[1].copy()
    bad[1] = np.nan  # the first component's amplitude: no factorisation
    batch = np.array([thetas[0], bad, thetas[2], thetas[1]])
    with pytest.warns(UserWarning):
        vals = gp.marginal_likelihood_batch(batch)
    assert vals[1] == -1e50
    good = [0, 2, 3]
    check(vals[good], [gp.marginal_likelihood(batch[i]) for i in good], 1e-12, "neighbours of a failure")


def test_runs_are_bit_identical(gsum):
    g = gsum
    thetas = g["rqsesewn_thetas"]
    res = []
    for _ in range(2):
        gp = _model(g, "rqsesewn")
        mu, sig = gp(g["rqsesewn_pts"])
        res.append((gp.alpha.copy(), mu, sig, gp.marginal_likelihood_gradient(thetas[1])[1],
                    gp.marginal_likelihood_gradient_batch(thetas)[1], gp.loo_likelihood_gradient(thetas[2])[1]))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_spatial_gradients_raise(gsum):
    g = gsum
    gp = _model(g, "serqwn")
    with pytest.raises(NotImplementedError):
        gp.gradient(g["serqwn_pts"][:2])
    with pytest.raises(NotImplementedError):
        gp.spatial_derivatives(g["serqwn_pts"][:2])


def test_add_point_equals_fit_from_scratch(gsum):
    from inference_amd.gp import GpRegressor

    g = gsum
    tag = "serqwn"
    x, y, e = g[f"{tag}_x"], g[f"{tag}_y"], g[f"{tag}_y_err"]
    th = g[f"{tag}_thetas"][1]
    pts = g[f"{tag}_pts"]
    for reserve in (0, 64):  # a rebuild, and the device append
        gp = GpRegressor(x[:-1], y[:-1], y_err=e[:-1], kernel=_cov(CASES[tag]), hyperpars=th, reserve=reserve)
        gp.add_point(x[-1], y[-1], e[-1])
        ref = GpRegressor(x, y, y_err=e, kernel=_cov(CASES[tag]), hyperpars=th)
        check(gp.alpha, ref.alpha, 1e-10, f"alpha after add_point (reserve {reserve})")
        mu, sig = gp(pts)
        rmu, rsig = ref(pts)
        check(mu, rmu, 1e-10, "mu after add_point")
        check(sig, rsig, 1e-10, "sigma after add_point")


def test_async_batches_take_the_sum_path(gsum, monkeypatch):
    g = gsum
    gp = _model(g, "rqsesewn")
    assert gp.async_batches()
    thetas = np.array(g["rqsesewn_thetas"])
    want = gp.marginal_likelihood_batch(thetas)
    calls = []
    submit = type(gp.engine).lml_batch_submit

    def counting(self, slot, kernel, *a, **kw):
        calls.append(kernel)
        return submit(self, slot, kernel, *a, **kw)

    monkeypatch.setattr(type(gp.engine), "lml_batch_submit", counting)
    gp.marginal_likelihood_batch_submit(thetas[:2], 0)
    gp.marginal_likelihood_batch_submit(thetas[2:], 1)
    got = np.concatenate([gp.marginal_likelihood_batch_wait(0), gp.marginal_likelihood_batch_wait(1)])
    from inference_amd import _lib

    assert calls == [_lib.KERNEL_SUM, _lib.KERNEL_SUM]
    check(got, want, 1e-12, "asynchronous slots")


def test_parallel_tempering_over_a_sum_takes_the_async_slots(gsum, monkeypatch):
    """ParallelTempering ladders over the LML of a sum model (N = 520: lockstep size, async_batches() holds), advanced
    together by advance_ladders: every likelihood round goes through gpmi_lml_batch_submit with GPMI_KERNEL_SUM, and the
    trajectories equal those of the same ladders advanced one at a time (ParallelTempering.advance)."""
    from inference_amd import _lib
    from inference_amd._engine import GpEngine
    from inference_amd.mcmc import advance_ladders

    g = gsum
    gp = _model(g, "rqsesewn")
    assert gp.async_batches()
    calls = []
    submit = GpEngine.lml_batch_submit

    def counting(self, slot, kernel, thetas_cov, *a, **kw):
        calls.append((kernel, len(thetas_cov)))
        return submit(self, slot, kernel, thetas_cov, *a, **kw)

    monkeypatch.setattr(GpEngine, "lml_batch_submit", counting)
    steps, interval = 2, 1
    together = [wl.cfg5_ladder(gp, k, n_temps=4) for k in range(4)]
    assert all(lad.batch_posterior is not None for lad in together)
    evals = advance_ladders(together, steps, swap_interval=interval)
    assert evals >= 16 * steps * gp.n_hyperpars
    assert calls and all(k == _lib.KERNEL_SUM for k, _ in calls)
    alone = [wl.cfg5_ladder(gp, k, n_temps=4) for k in range(4)]
    for lad in alone:
        lad.advance(steps, swap_interval=interval)
    for a, b in zip(together, alone):
        for ca, cb in zip(a.chains, b.chains):
            assert np.array_equal(ca.get_sample(burn=0), cb.get_sample(burn=0))
            assert np.array_equal(np.array(ca.probs), np.array(cb.probs))
        assert np.array_equal(a.successful_swaps, b.successful_swaps)


def _numpy_lml_and_gradient(x, y, e2, kinds, theta_cov, mu):
    """LML and its gradient with respect to the stationary components' parameters of an SE / RQ sum (no WhiteNoise),
    by dense NumPy: K = sum_m a_m^2 (C_m + 1e-12 I) + diag(e2)."""
    n, d = x.shape
    D = [0.5 * (x[:, k][:, None] - x[:, k][None, :]) ** 2 for k in range(d)]
    K = np.diag(e2).astype(float)
    dKs = []
    off = 0
    for kind in kinds:
        a2 = np.exp(2 * theta_cov[off])
        if kind == "rq":
            kap = np.exp(theta_cov[off + 1])
            ls = np.exp(theta_cov[off + 2: off + 2 + d])
            s = sum(D[k] / ls[k] ** 2 for k in range(d))
            F = 1 + s / kap
            C = F ** (-kap)
            Km = a2 * (C + 1e-12 * np.eye(n))
            dKs.append(2 * Km)
            dKs.append(-a2 * C * (kap * np.log(F) - s / F))
            dKs += [a2 * C / F * (2 * D[k] / ls[k] ** 2) for k in range(d)]
            off += 2 + d
        else:
            ls = np.exp(theta_cov[off + 1: off + 1 + d])
            s = sum(D[k] / ls[k] ** 2 for k in range(d))
            C = np.exp(-s)
            Km = a2 * (C + 1e-12 * np.eye(n))
            dKs.append(2 * Km)
            dKs += [a2 * C * (2 * D[k] / ls[k] ** 2) for k in range(d)]
            off += 1 + d
        K = K + Km
    L = np.linalg.cholesky(K)
    r = y - mu
    v = np.linalg.solve(L, r)
    alpha = np.linalg.solve(L.T, v)
    lml = -0.5 * v @ v - np.log(np.diagonal(L)).sum()
    iK = np.linalg.inv(K)
    Q = np.outer(alpha, alpha) - iK
    grad = np.array([0.5 * (Q * dK).sum() for dK in dKs])
    return lml, grad


def test_sum_against_numpy_at_2500():
    from inference_amd.gp import GpRegressor

    n, d = 2500, 3
    x, y, e = wl.synthetic_dataset(21, n, d)
    kinds = ("se", "rq")
    theta = np.array([float(np.mean(y)), 0.1, np.log(0.6), np.log(0.5), np.log(0.7), -0.4, 0.2, np.log(0.15),
                      np.log(0.1), np.log(0.2)])
    gp = GpRegressor(x, y, y_err=e, kernel=_cov(kinds), hyperpars=theta)
    lml, grad = gp.marginal_likelihood_gradient(theta)
    rl, rg = _numpy_lml_and_gradient(x, y, e ** 2, kinds, theta[1:], np.full(n, theta[0]))
    check(lml, rl, 1e-10, "lml vs numpy")
    check(grad[1:], rg, 1e-10, "lml gradient vs numpy")
    check(gp.marginal_likelihood(theta), rl, 1e-10, "lml (no gradient) vs numpy")


@pytest.mark.parametrize("n", [4100, 8192])
def test_sum_against_mixture_with_unit_weights(n):
    """The same model through independent kernels: gpmi_lml_mix / gpmi_lml_grad_mix with every window weight 1 build
    K = sum_m K_m by separate single-kernel builds and contract the gradient component by component."""
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    d = 8
    x, y, e = wl.synthetic_dataset(3, n, d)
    kinds = [_lib.KERNEL_SE, _lib.KERNEL_RQ]
    th_se = np.concatenate([[0.2], np.log(np.linspace(0.8, 1.6, d))])
    th_rq = np.concatenate([[-0.5, 0.3], np.log(np.linspace(0.3, 0.6, d))])
    mu = np.full(n, float(np.mean(y)))
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        eng.set_sum(kinds)
        theta = np.concatenate([th_se, th_rq])
        lml, info = eng.lml(_lib.KERNEL_SUM, theta, 0.0, mu)
        assert info == 0
        glml, grad, trace_q, alpha, ginfo = eng.lml_grad(_lib.KERNEL_SUM, theta, 0.0, mu)
        assert ginfo == 0
        ones = np.ones((2, n))
        mlml, minfo = eng.lml_mix(kinds, [th_se, th_rq], ones, 0.0, mu)
        assert minfo == 0
        mglml, mgrad, _, malpha, mginfo = eng.lml_grad_mix(kinds, [th_se, th_rq], ones, 0.0, mu)
        assert mginfo == 0
    finally:
        eng.close()
    check(lml, mlml, 1e-11, "lml vs mixture")
    check(glml, mglml, 1e-11, "lml (gradient path) vs mixture")
    check(grad, mgrad, 1e-11, "gradient vs mixture")
    check(alpha, malpha, 1e-11, "alpha vs mixture")


def _numpy_sum_cross(u, v, kinds, theta_cov):
    """sum_m a_m^2 C_m(u, v) of SE / RQ components by dense NumPy (no jitter: a cross-covariance)."""
    d = u.shape[1]
    out = np.zeros((u.shape[0], v.shape[0]))
    off = 0
    for kind in kinds:
        a2 = np.exp(2 * theta_cov[off])
        if kind == "rq":
            kap = np.exp(theta_cov[off + 1])
            ls = np.exp(theta_cov[off + 2: off + 2 + d])
            off += 2 + d
        else:
            ls = np.exp(theta_cov[off + 1: off + 1 + d])
            off += 1 + d
        s = sum(0.5 * (u[:, k][:, None] - v[:, k][None, :]) ** 2 / ls[k] ** 2 for k in range(d))
        out += a2 * ((1 + s / kap) ** (-kap) if kind == "rq" else np.exp(-s))
    return out


@pytest.mark.parametrize("m", [1, 200, 2500])
def test_cross_and_square_covariance_entry_points(m):
    """gpmi_cross_covariance / gpmi_covariance with GPMI_KERNEL_SUM directly: ragged query counts over one, several and
    more than a 2048-point chunk of 64-row tiles (N = 700, d = 3, RQ + SE + SE), against the NumPy sum."""
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    n, d = 700, 3
    x, y, e = wl.synthetic_dataset(17, n, d)
    pts = np.random.default_rng(m).uniform(x.min(), x.max(), (m, d))
    kinds = ("rq", "se", "se")
    theta = np.array([-0.2, 0.4, np.log(0.9), np.log(0.7), np.log(1.1),
                      0.3, np.log(0.5), np.log(0.4), np.log(0.6),
                      -0.8, np.log(0.12), np.log(0.2), np.log(0.15)])
    eng = GpEngine(x, y, noise_var=e ** 2)
    try:
        eng.set_sum([_lib.KERNEL_RQ, _lib.KERNEL_SE, _lib.KERNEL_SE])
        kx = eng.cross_covariance(_lib.KERNEL_SUM, theta, pts)
        K = eng.covariance(_lib.KERNEL_SUM, theta, 0.01)
        Kn = eng.covariance(_lib.KERNEL_SUM, theta, 0.01, with_noise=True)
    finally:
        eng.close()
    check(kx, _numpy_sum_cross(pts, x, kinds, theta), 1e-13, f"cross covariance, m = {m}")
    jitter = sum(np.exp(2 * theta[o]) * 1e-12 for o in (0, 5, 9))
    ref = _numpy_sum_cross(x, x, kinds, theta) + (jitter + 0.01) * np.eye(n)
    check(K, ref, 1e-13, "square covariance")
    check(Kn, ref + np.diag(e ** 2), 1e-13, "square covariance with data variances")
