"""
CPU tests of a dense data-error covariance (`y_cov`): the oracle's dense-noise path (oracle/gp_oracle.py, `sig_full`)
against the reference's values (tests/golden/ycov.npz), the bit-exact rebuild of the stored Kac-Murdock-Szego matrices
(tests/ycov_builders.py), and the constructor's checks of `y_cov` that run before any device work (regression.py:366-388,
as the reference's :246-293).
"""
import os
import warnings

import numpy as np
import pytest

import ycov_builders as yb
from oracle import gp_oracle as orc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL = 1e-11


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, what, tol=TOL):
    r = rel(a, b)
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "ycov.npz"), allow_pickle=False)


def y_cov_of(g, tag):
    """The case's Y: stored (kind a) or rebuilt from its permutation (kind b)."""
    if f"{tag}_Y" in g.files:
        return g[f"{tag}_Y"]
    return yb.kms_cov(g[f"{tag}_perm"])


@pytest.mark.parametrize("tag", ["serq", "cp", "het", "se1500"])
def test_rebuilt_y_cov_matches_the_stored_probes_bit_for_bit(g, tag):
    Y = y_cov_of(g, tag)
    ij = g[f"{tag}_probe_ij"]
    assert np.array_equal(Y[ij[:, 0], ij[:, 1]], g[f"{tag}_probe_val"])
    assert np.array_equal(Y, Y.T)
    # the probes reach both the large entries and the tiny far ones
    assert (g[f"{tag}_probe_val"] > 1e-3 * Y.max()).sum() >= 16


def test_stored_y_cov_is_symmetric_and_dense(g):
    for tag in ("se", "rqwn"):
        Y = g[f"{tag}_Y"]
        assert np.array_equal(Y, Y.T)
        off = np.abs(Y).sum() - np.trace(Y)
        assert off > 2 * np.trace(Y), "the off-diagonal mass is what this fixture is about"


def test_kms_y_cov_is_far_from_banded():
    """Most large entries of kind (b) lie more than 64 rows off the diagonal: a K-build that adds Y only within a band
    drops them."""
    p = np.random.default_rng(0).permutation(1500)
    Y = yb.kms_cov(p)
    i, j = np.nonzero(Y > 1e-3 * Y.max())
    assert (np.abs(i - j) > 64).mean() > 0.8
    assert np.linalg.cond(Y) < 100


ORACLE = {"se": (orc.SE, False), "rqwn": (orc.RQ, True), "se1500": (orc.SE, False)}


@pytest.mark.parametrize("tag", list(ORACLE))
def test_oracle_dense_noise_matches_reference(g, tag):
    kernel, wn = ORACLE[tag]
    thetas = g[f"{tag}_thetas"]
    ref = orc.OracleGp(g[f"{tag}_x"], g[f"{tag}_y"], y_cov=y_cov_of(g, tag), kernel=kernel, white_noise=wn,
                       hyperpars=thetas[0])
    check(np.array(ref.hp_bounds, dtype=float), g[f"{tag}_bounds"], "bounds", 1e-12)
    check(ref.alpha, g[f"{tag}_alpha"], "alpha")
    if tag == "se":
        ii = g["se_K_idx"]
        check(ref.K_xx[np.ix_(ii, ii)], g["se_K_sub"], "K_xx", 1e-15)
    pts = g[f"{tag}_pts"]
    mu, sig = ref(pts)
    check(mu, g[f"{tag}_mu"], "mu")
    check(sig, g[f"{tag}_sig"], "sigma")
    pm, pc = ref.build_posterior(pts[:16])
    check(pm, g[f"{tag}_post_mu"], "posterior mean")
    check(pc, g[f"{tag}_post_cov"], "posterior covariance")
    lm, ls = ref.loo_predictions()
    check(lm, g[f"{tag}_loo_mu"], "loo mu")
    check(ls, g[f"{tag}_loo_sig"], "loo sigma")
    check([ref.marginal_likelihood(t) for t in thetas], g[f"{tag}_lml"], "lml")
    res = [ref.marginal_likelihood_gradient(t) for t in thetas]
    check([r[0] for r in res], g[f"{tag}_lml"], "lml (gradient call)")
    check(np.array([r[1] for r in res]), g[f"{tag}_lml_grad"], "lml gradient")
    check([ref.loo_likelihood(t) for t in thetas], g[f"{tag}_loo"], "loo")
    check(np.array([ref.loo_likelihood_gradient(t)[1] for t in thetas]), g[f"{tag}_loo_grad"], "loo gradient")
    if kernel == orc.SE:
        ref.set_hyperparameters(thetas[0])
        s_mu, s_var = ref.spatial_derivatives(pts)
        check(s_mu, g[f"{tag}_sd_mu"], "spatial derivative of mu")
        check(s_var, g[f"{tag}_sd_var"], "spatial derivative of the variance")
        g_mu, g_cov = ref.gradient(pts)
        check(g_mu, g[f"{tag}_grad_mu"], "gradient mean")
        check(g_cov, g[f"{tag}_grad_cov"], "gradient covariance")


# ---------------------------------------------------------------------------------------
# constructor checks of y_cov: all of them run before the device is touched
# ---------------------------------------------------------------------------------------
def _data(n=12, d=2):
    rng = np.random.default_rng(3)
    return rng.uniform(0, 1, (n, d)), rng.normal(size=n)


def test_y_cov_of_the_wrong_shape_is_refused():
    from inference_amd.gp import GpRegressor

    x, y = _data()
    Y = yb.kms_cov(np.arange(12))
    for bad in (Y[:-1, :-1], Y[:, :-1], np.diag(Y)):
        with pytest.raises(ValueError):
            GpRegressor(x, y, y_cov=bad, hyperpars=np.zeros(4))


def test_y_cov_one_ulp_off_symmetric_is_refused():
    from inference_amd.gp import GpRegressor

    x, y = _data()
    Y = yb.kms_cov(np.random.default_rng(1).permutation(12))
    Y[7, 2] = np.nextafter(Y[7, 2], np.inf)
    with pytest.raises(ValueError):
        GpRegressor(x, y, y_cov=Y, hyperpars=np.zeros(4))


def test_y_err_beside_y_cov_warns_and_y_cov_wins():
    from inference_amd.gp import GpRegressor

    x, y = _data()
    Y = yb.kms_cov(np.random.default_rng(2).permutation(12))
    gp = GpRegressor.__new__(GpRegressor)  # the checks alone: no device behind this object
    gp.n_points = y.size
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        noise_var, y_cov = gp.check_error_data(np.full(12, 0.3), Y)
    assert len(w) == 1 and "y_cov" in str(w[0].message)
    assert noise_var is None and np.array_equal(y_cov, Y)
    gp._noise_var, gp._y_cov = noise_var, y_cov
    assert np.array_equal(gp.sig, Y)
