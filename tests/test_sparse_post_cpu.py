"""CPU checks of the sparse model's joint posterior and derivatives by the query point: the mirror's formulas
(tests/sparse_post_host.py) against finite differences of `SparseMirror.predict`, against the mirror's own variance and
against the exact GP posterior, and the surface the feature adds (header, prototypes, SparseGpRegressor).

The tolerance of the finite-difference checks is taken from the finite differences themselves: ten times the largest
difference between fourth-order differences at h = 1e-3 and at h = 2e-3, per kernel and quantity.  Measured (error /
tolerance), 9 query points of which one is a row of x and one a row of Z:
  se   N = 120  d = 3  m = 9     d mean 3.0e-11 / 4.5e-09    d var 2.1e-10 / 3.2e-08
  m52  N = 150  d = 2  m = 11    d mean 6.2e-10 / 9.2e-08    d var 5.4e-09 / 8.1e-07
  rq   N = 90   d = 4  m = 7     d mean 2.4e-11 / 3.6e-09    d var 6.7e-11 / 1.0e-08
  m32  N = 80   d = 5  m = 6     d mean 2.6e-11 / 3.8e-09    d var 5.5e-11 / 8.2e-09
(Matern32 is only C^1 at zero distance: its query points keep off the inducing inputs.)
"""
import inspect
import os
import re

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import matern_host as mh
import sparse_host as sh
import sparse_post_host as sph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("gpmi_sgp_posterior", "gpmi_sgp_posterior_draws", "gpmi_sgp_spatial_derivatives")
SHAPES = [("se", 120, 3, 9), ("m52", 150, 2, 11), ("rq", 90, 4, 7), ("m32", 80, 5, 6)]


def _model(kind, n, d, m):
    x, y, e = sh.dataset(n, d, seed=3)
    z = x[sh.spread_rows(x, m)] + 0.01
    scales = 0.35 * np.sqrt(d / 3.0) * (1.0 + 0.1 * np.arange(d) / max(d - 1, 1))
    theta = np.array([0.1] + ([0.3] if kind == "rq" else []) + list(np.log(scales)))
    q = np.random.default_rng(7).uniform(0.05, 0.95, size=(9, d))
    q[1] = x[5]
    if kind != "m32":
        q[2] = z[3]
    mir = sh.SparseMirror(kind, x, z)
    r, nv, white = y - 0.2, e**2, 0.02
    return mir, theta, white, r, nv, q, mir.state(theta, white, r, nv)


@pytest.mark.parametrize("kind,n,d,m", SHAPES)
def test_mirror_derivatives_against_finite_differences(kind, n, d, m):
    mir, theta, white, r, nv, q, st = _model(kind, n, d, m)
    dmean, dvar = sph.derivatives(mir, st, theta, q)
    assert dmean.shape == q.shape and dvar.shape == q.shape
    for which, got in ((0, dmean), (1, dvar)):
        f = lambda pts: mir.predict(theta, white, r, nv, pts, st=st)[which]
        fd1, fd2 = sph.fd4_rows(f, q, 1e-3), sph.fd4_rows(f, q, 2e-3)
        tol = 10.0 * float(np.abs(fd1 - fd2).max())
        err = float(np.abs(got - fd1).max())
        print(f"{kind} N = {n} d = {d} m = {m} {'d var' if which else 'd mean'}: max {np.abs(got).max():.3g}, "
              f"error {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (kind, which, err, tol)


@pytest.mark.parametrize("kind,n,d,m", SHAPES)
def test_diagonal_of_sigma_is_the_predictive_variance(kind, n, d, m):
    mir, theta, white, r, nv, q, st = _model(kind, n, d, m)
    mu, sigma = sph.posterior(mir, st, theta, q)
    mean, var = mir.predict(theta, white, r, nv, q, st=st)
    assert np.array_equal(sigma, sigma.T)
    assert np.abs(mu - mean).max() <= 1e-13 * max(1.0, np.abs(mean).max())
    assert np.abs(np.diag(sigma) - var).max() <= 1e-13 * st["a2"]


def test_a_query_point_on_an_inducing_input_gets_an_exact_zero():
    """One inducing input, the query on it: both derivatives are exactly zero - nothing is divided by a distance."""
    x, y, e = sh.dataset(40, 2, seed=2)
    z = x[[11]].copy()
    for kind in ("se", "m52", "rq", "m32"):
        theta = np.array([0.1] + ([0.3] if kind == "rq" else []) + [np.log(0.4)] * 2)
        mir = sh.SparseMirror(kind, x, z)
        st = mir.state(theta, 0.02, y - 0.2, e**2)
        dmean, dvar = sph.derivatives(mir, st, theta, z)
        assert np.array_equal(dmean, np.zeros((1, 2))) and np.array_equal(dvar, np.zeros((1, 2))), kind


def test_inducing_points_at_the_data_give_the_exact_posterior():
    """Z = x, eps = 0: mu and Sigma are the exact GP's, computed densely.  Allowance: the two routes differ by rounding
    errors amplified by cond(K_mm) = 2.8e5, about 2.8e5 x 2.2e-16 = 6e-11 per operation: 1e-9 of the scale (measured:
    mu 4.6e-11, Sigma 1.4e-11)."""
    n, d = 60, 2
    x, y, e = sh.dataset(n, d, seed=4)
    theta = np.array([0.1, np.log(0.3), np.log(0.35)])
    q = np.random.default_rng(2).uniform(0.0, 1.0, size=(13, d))
    r, nv = y - 0.2, e**2
    mir = sh.SparseMirror("m52", x, x, jitter=0.0)
    st = mir.state(theta, 0.0, r, nv)
    mu, sigma = sph.posterior(mir, st, theta, q)
    K = mh.cross("m52", x, x, theta) + np.diag(nv)
    Lk = cholesky(K, lower=True)
    Kq = mh.cross("m52", x, q, theta)
    A = solve_triangular(Lk, Kq, lower=True)
    mu_exact = A.T @ solve_triangular(Lk, r, lower=True)
    sigma_exact = mh.cross("m52", q, q, theta) - A.T @ A
    a2 = float(np.exp(2.0 * theta[0]))
    e_mu, e_sig = float(np.abs(mu - mu_exact).max()), float(np.abs(sigma - sigma_exact).max())
    print(f"Z = x: mu {e_mu:.3e}, Sigma {e_sig:.3e}, cond {np.linalg.cond(mh.cross('m52', x, x, theta)):.3g}")
    assert e_mu <= 1e-9 * np.abs(mu_exact).max() and e_sig <= 1e-9 * a2


def test_header_and_prototypes_name_the_entry_points():
    from inference_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(\s*gpmi_sgp\s*\*", header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["gpmi_sgp_posterior_draws"][1]) == len(_lib.SIGNATURES["gpmi_posterior_draws"][1])
    assert re.search(r"#define\s+GPMI_VERSION\s+100\b", header)


def test_regressor_and_engine_have_the_new_methods():
    from inference_amd._engine import SparseEngine
    from inference_amd.gp import GpRegressor, SparseGpRegressor

    for name in ("process_points", "build_posterior", "sample_posterior", "spatial_derivatives", "spatial_derivatives_batch"):
        assert callable(getattr(SparseGpRegressor, name, None)), name
    assert not hasattr(SparseGpRegressor, "gradient")
    a = inspect.signature(SparseGpRegressor.sample_posterior).parameters
    b = inspect.signature(GpRegressor.sample_posterior).parameters
    assert list(a) == list(b) and all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    assert inspect.signature(SparseGpRegressor.build_posterior).parameters["mean_only"].default is False
    for name in ("posterior", "posterior_draws", "spatial_derivatives"):
        assert callable(getattr(SparseEngine, name, None)), name
    assert inspect.signature(SparseEngine.spatial_derivatives).parameters["want_var"].default is True
