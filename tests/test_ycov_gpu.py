"""
GPU tests of a dense data-error covariance (`GpRegressor(..., y_cov=Y)`: K = cov(theta) + Y in every method, regression.py:
133, 239, 475, 498, 534, 552 of the reference).  With Y present the device adds the N x N matrix into every factorisation
(launch_add_full), builds K unsplit at look-ahead sizes, and runs every batch through the per-lane fallback instead of the
lockstep kernels - paths no diagonal-noise model reaches.  Compared here: every public method against the reference's values
(tests/golden/ycov.npz), batches against single evaluations, the routing such a model relies on, N = 6500 against the CPU
oracle, and a seeded random sweep (tools/fuzz_parity.py, dense_noise=True).  The comparisons go through test_gpu_parity's
helpers, so the achieved errors appear in the run's table.

Every test runs with the engine's dense host-composition entry points (`*_dense`) made to raise; where a model legitimately
takes one of them, the test says so and lets that one through.
"""
import os
import sys
import warnings

import numpy as np
import pytest

import workloads as wl
import ycov_builders as yb
from test_gpu_parity import RTOL, _record, check, check_each

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TAGS = ["se", "rqwn", "serq", "cp", "het", "se1500"]


@pytest.fixture(autouse=True)
def allow_dense(monkeypatch):
    """Every GpEngine.*_dense raises; the returned function lets one of them through again."""
    from inference_amd._engine import GpEngine

    originals = {}

    def tripwire(name):
        def fail(*args, **kwargs):
            raise AssertionError(f"GpEngine.{name} called: a y_cov model left the device kernels")

        return fail

    for name in dir(GpEngine):
        if name.endswith("_dense"):
            originals[name] = getattr(GpEngine, name)
            monkeypatch.setattr(GpEngine, name, tripwire(name))

    def allow(name):
        monkeypatch.setattr(GpEngine, name, originals[name])

    return allow


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "ycov.npz"), allow_pickle=False)


def y_cov_of(g, tag):
    if f"{tag}_Y" in g.files:
        return g[f"{tag}_Y"]
    p = g[f"{tag}_perm"]
    Y = yb.kms_cov(p)
    ij = g[f"{tag}_probe_ij"]
    # the rebuilt matrix is the reference's bit for bit before anything is compared with it
    assert np.array_equal(Y[ij[:, 0], ij[:, 1]], g[f"{tag}_probe_val"])
    return Y


def _cov(tag):
    from inference_amd.gp import ChangePoint, HeteroscedasticNoise, RationalQuadratic, SquaredExponential, WhiteNoise

    if tag in ("se", "se1500"):
        return SquaredExponential()
    if tag == "rqwn":
        return RationalQuadratic() + WhiteNoise()
    if tag == "serq":
        return SquaredExponential() + RationalQuadratic()
    if tag == "cp":
        return ChangePoint(kernels=[SquaredExponential, RationalQuadratic], axis=0)
    return SquaredExponential() + HeteroscedasticNoise()


def _model(g, tag, **kw):
    from inference_amd.gp import GpRegressor

    if "n_starts" not in kw:
        kw["hyperpars"] = g[f"{tag}_thetas"][0]
    return GpRegressor(g[f"{tag}_x"], g[f"{tag}_y"], y_cov=y_cov_of(g, tag), kernel=_cov(tag), **kw)


# the leave-one-out gradient of a ChangePoint or HeteroscedasticNoise model has lockstep kernels for diagonal data errors
# only (GpRegressor._loo_batch_ok); with a dense y_cov it is gpmi_loo_dense plus per-component host contractions
LOO_GRAD_DENSE = ("cp", "het")


@pytest.mark.parametrize("tag", TAGS)
def test_y_cov_case_matches_reference(g, allow_dense, tag):
    gp = _model(g, tag)
    assert gp._y_cov is not None and not gp._generic
    assert gp.hyperpar_labels == list(g[f"{tag}_labels"])
    check(np.array(gp.hp_bounds, dtype=float), g[f"{tag}_bounds"], 1e-12, f"{tag}: bounds")
    if tag == "se":
        ii = g["se_K_idx"]
        check(gp.K_xx[np.ix_(ii, ii)], g["se_K_sub"], 1e-13, f"{tag}: K_xx at 64 rows / columns")
    check_each(gp.alpha, g[f"{tag}_alpha"], what=f"{tag}: alpha")
    pts = g[f"{tag}_pts"]
    mu, sig = gp(pts)
    check(mu, g[f"{tag}_mu"], what=f"{tag}: mu")
    check(sig, g[f"{tag}_sig"], what=f"{tag}: sigma")
    pm, pc = gp.build_posterior(pts[:16])
    check(pm, g[f"{tag}_post_mu"], what=f"{tag}: posterior mean")
    check(pc, g[f"{tag}_post_cov"], what=f"{tag}: posterior covariance")
    lm, ls = gp.loo_predictions()
    check(lm, g[f"{tag}_loo_mu"], what=f"{tag}: loo mu")
    check(ls, g[f"{tag}_loo_sig"], what=f"{tag}: loo sigma")
    if tag in ("se", "se1500"):
        g_mu, g_cov = gp.gradient(pts)
        check(g_mu, g[f"{tag}_grad_mu"], what=f"{tag}: gradient mean")
        check(g_cov, g[f"{tag}_grad_cov"], what=f"{tag}: gradient covariance")
        s_mu, s_var = gp.spatial_derivatives(pts)
        check(s_mu, g[f"{tag}_sd_mu"], what=f"{tag}: spatial derivative of mu")
        check(s_var, g[f"{tag}_sd_var"], what=f"{tag}: spatial derivative of the variance")
    thetas = g[f"{tag}_thetas"]
    check([gp.marginal_likelihood(t) for t in thetas], g[f"{tag}_lml"], what=f"{tag}: lml")
    for t, ref_l, ref_g in zip(thetas, g[f"{tag}_lml"], g[f"{tag}_lml_grad"]):
        lml, grad = gp.marginal_likelihood_gradient(t)
        check(lml, ref_l, what=f"{tag}: lml (gradient call)")
        check_each(grad, ref_g, what=f"{tag}: lml gradient")
    check([gp.loo_likelihood(t) for t in thetas], g[f"{tag}_loo"], what=f"{tag}: loo")
    if tag in LOO_GRAD_DENSE:
        allow_dense("loo_dense")
    for t, ref_l, ref_g in zip(thetas, g[f"{tag}_loo"], g[f"{tag}_loo_grad"]):
        loo, grad = gp.loo_likelihood_gradient(t)
        check(loo, ref_l, what=f"{tag}: loo (gradient call)")
        check_each(grad, ref_g, what=f"{tag}: loo gradient")


@pytest.mark.parametrize("tag", ["se", "rqwn", "serq"])
def test_y_cov_seeded_search_reaches_reference(g, tag):
    """As test_seeded_search_reaches_reference (tests/test_sum_kernels_gpu.py): with y_cov the starts run one after
    another (no lockstep search), from the same numpy.random.seed(7) positions as the reference's."""
    np.random.seed(7)
    gp = _model(g, tag, n_starts=3)
    check(gp.marginal_likelihood(gp.hyperpars), g[f"{tag}_search_lml"], 1e-10, f"{tag}: search lml")
    # the reference's theta* scores the same on the device: both searches ended at the same optimum
    check(gp.marginal_likelihood(g[f"{tag}_search_theta"]), g[f"{tag}_search_lml"], 1e-10,
          f"{tag}: lml at the reference's theta*")
    # L-BFGS-B stops within its own convergence test (factr 1e7: ~2e-9 relative in the objective), so theta* agrees to
    # the flatness of the optimum, not to the last digits
    check(np.asarray(gp.hyperpars, float), g[f"{tag}_search_theta"], 1e-4, f"{tag}: search theta")


@pytest.mark.parametrize("tag", ["se1500", "serq", "cp"])
def test_y_cov_batches_equal_single_evaluations(g, allow_dense, tag):
    """With y_cov no batch runs in lockstep: gpmi_lml_batch / gpmi_lml_grad_batch(_mix) / gpmi_loo_grad_batch take the
    per-lane fallback, T evaluations spread over fewer lanes.  (cp: its LOO gradient is the dense path, LOO_GRAD_DENSE.)"""
    if tag in LOO_GRAD_DENSE:
        allow_dense("loo_dense")
    gp = _model(g, tag)
    base = g[f"{tag}_thetas"]
    # against the reference first
    check(gp.marginal_likelihood_batch(base), g[f"{tag}_lml"], what=f"{tag}: lml batch")
    check_each(gp.marginal_likelihood_gradient_batch(base)[1], g[f"{tag}_lml_grad"], what=f"{tag}: lml gradient batch")
    check_each(gp.loo_likelihood_gradient_batch(base)[1], g[f"{tag}_loo_grad"], what=f"{tag}: loo gradient batch")
    rng = np.random.default_rng(5)
    for T in (2, 5, 9, 17):
        thetas = base[rng.integers(0, 3, T)] + 0.02 * rng.standard_normal((T, base.shape[1]))
        check(gp.marginal_likelihood_batch(thetas), [gp.marginal_likelihood(t) for t in thetas], 1e-12,
              f"{tag}: lml batch of {T}")
        lml, grads = gp.marginal_likelihood_gradient_batch(thetas)
        single = [gp.marginal_likelihood_gradient(t) for t in thetas]
        check(lml, [s[0] for s in single], 1e-12, f"{tag}: lml (gradient batch of {T})")
        for k in range(T):
            check_each(grads[k], single[k][1], 1e-12, what=f"{tag}: lml gradient, batch of {T}")
        loo, grads = gp.loo_likelihood_gradient_batch(thetas)
        single = [gp.loo_likelihood_gradient(t) for t in thetas]
        check(loo, [s[0] for s in single], 1e-12, f"{tag}: loo (gradient batch of {T})")
        for k in range(T):
            check_each(grads[k], single[k][1], 1e-12, what=f"{tag}: loo gradient, batch of {T}")
    # a failing member: the sentinel, and its neighbours exactly as without it
    thetas = base[rng.integers(0, 3, 9)] + 0.02 * rng.standard_normal((9, base.shape[1]))
    clean = gp.marginal_likelihood_batch(thetas)
    bad = thetas.copy()
    bad[4, 1] = np.nan  # the (first) amplitude
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        vals = gp.marginal_likelihood_batch(bad)
    assert vals[4] == -1e50
    keep = np.arange(9) != 4
    assert np.array_equal(vals[keep], clean[keep]), np.abs(vals[keep] - clean[keep]).max()


def test_y_cov_routing_and_reproducibility(g):
    """What a y_cov model relies on: no asynchronous or lockstep batches, no O(N^2) point append; and two fresh
    regressors on the same data give the same bits."""
    gp = _model(g, "se1500")
    assert not gp.async_batches()
    assert not gp._lockstep_search()
    assert not gp._loo_batch_ok()
    gp2 = _model(g, "se1500")
    th = g["se1500_thetas"][1]
    assert np.array_equal(gp.alpha, gp2.alpha)
    assert gp.marginal_likelihood(th) == gp2.marginal_likelihood(th)
    with pytest.raises(NotImplementedError):
        gp.add_point(np.full(3, 0.5), 0.1)
    assert gp.n_points == 1500


def test_y_cov_large_size_vs_oracle():
    """N = 6500 (padded to 6528 = 51 tile rows): the look-ahead regime, the 512-wide inverse blocks with a partial last
    block, and the K-build unsplit because Y is added after it (api.hip); shape as test_ragged_large_size_vs_oracle."""
    from inference_amd.gp import GpRegressor
    from oracle import gp_oracle as orc

    n, d = 6500, 3
    x, y, _ = wl.synthetic_dataset(67, n, d)
    Y = yb.kms_cov(np.random.default_rng(67).permutation(n))
    th = wl.timing_theta(wl.SE, y, d)
    gp = GpRegressor(x, y, y_cov=Y, hyperpars=th)
    ref = orc.OracleGp(x, y, y_cov=Y, kernel=orc.SE, hyperpars=th)
    check_each(gp.alpha, ref.alpha, what="alpha, N = 6500")
    check(gp.marginal_likelihood(th), ref.marginal_likelihood(th), what="lml, N = 6500")
    pts = wl.query_points(67, 300, d)
    mu, sig = gp(pts)
    rmu, rsig = ref(pts)
    check(mu, rmu, what="mu, N = 6500")
    check(sig, rsig, what="sig, N = 6500")
    lml, grad = gp.marginal_likelihood_gradient(th)
    rl, rg = ref.marginal_likelihood_gradient(th)
    check(lml, rl, what="lml (gradient call), N = 6500")
    check_each(grad, rg, what="lml gradient, N = 6500")
    loo, grad = gp.loo_likelihood_gradient(th)
    rl, rg = ref.loo_likelihood_gradient_lean(th)
    check(loo, rl, what="loo (gradient call), N = 6500")
    check_each(grad, rg, what="loo gradient, N = 6500")


def test_y_cov_random_problems_vs_oracle():
    """tools/fuzz_parity.py with dense data errors: sizes 2 .. 2600 across the tile-count boundaries, SE / RQ, with and
    without WhiteNoise, every quantity of the sweep against the oracle to 1e-10."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_parity

    res = fuzz_parity.sweep(seed=11, cases=8, nmax=2600, verbose=False, dense_noise=True)
    assert len(res) == 8
    worst = {}
    for desc, errs in res:
        for q, r in errs.items():
            assert r <= RTOL, f"{desc}: {q} relative error {r:.3e}"
            worst[q] = max(worst.get(q, 0.0), r)
    for q, r in worst.items():
        _record(f"worst {q} over 8 random problems with dense y_cov", r, RTOL)
