"""CPU checks of the gradient by the inducing inputs: the mirror's formula (tests/sparse_z_host.py) against finite
differences of the mirror's own bound, and the surface the feature adds (header, export map, SparseGpRegressor).

The tolerance of the finite-difference check is taken from the finite difference itself: ten times the largest difference
between `fd4` at h = 1e-3 and at h = 2e-3, per kernel.  Measured (error / tolerance, gradients of order 10^2):
  se   N = 120  d = 3  m = 9     1.8e-08 / 2.6e-06    (max |dF/dZ| 485)
  m52  N = 150  d = 2  m = 11    3.3e-07 / 4.9e-05    (367)
  rq   N = 90   d = 4  m = 7     9.8e-09 / 1.4e-06    (191)
  m32  N = 80   d = 5  m = 6     7.6e-07 / 1.1e-04    (176; the kernel is only C^1 at zero distance)
"""
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest

import sparse_host as sh
import sparse_z_host as szh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("gpmi_sgp_set_inducing", "gpmi_sgp_bound_zgrad")


@pytest.mark.parametrize("kind,n,d,m", [("se", 120, 3, 9), ("m52", 150, 2, 11), ("rq", 90, 4, 7), ("m32", 80, 5, 6)])
def test_mirror_gradient_against_finite_differences(kind, n, d, m):
    x, y, e = sh.dataset(n, d, seed=3)
    z = x[sh.spread_rows(x, m)] + 0.01  # (off the data: Matern32 has no second derivative at zero distance)
    scales = 0.35 * np.sqrt(d / 3.0) * (1.0 + 0.1 * np.arange(d) / max(d - 1, 1))
    theta = np.array([0.1] + ([0.3] if kind == "rq" else []) + list(np.log(scales)))
    r, nv, white = y - 0.2, e**2, 0.02
    got = szh.inducing_gradient(sh.SparseMirror(kind, x, z), theta, white, r, nv)
    assert got.shape == (m, d)
    f = szh.bound_of_z(kind, x, theta, white, r, nv)
    fd1, fd2 = sh.fd4(f, z.ravel(), h=1e-3), sh.fd4(f, z.ravel(), h=2e-3)
    tol = 10.0 * float(np.abs(fd1 - fd2).max())
    err = float(np.abs(got.ravel() - fd1).max())
    print(f"{kind} N = {n} d = {d} m = {m}: max |dF/dZ| {np.abs(got).max():.3g}, error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (kind, err, tol)


def test_coincident_points_contribute_exact_zeros():
    """Z rows that are rows of x, two of them equal: nothing is divided by a distance, the gradient is finite for all
    four kernels."""
    x, y, e = sh.dataset(60, 2, seed=1)
    z = x[[0, 7, 7, 30]].copy()
    for kind in ("se", "m52", "rq", "m32"):
        theta = np.array([0.1] + ([0.3] if kind == "rq" else []) + [np.log(0.4)] * 2)
        g = szh.inducing_gradient(sh.SparseMirror(kind, x, z, jitter=1e-6), theta, 0.02, y - 0.2, e**2)
        assert np.isfinite(g).all(), kind


def test_header_declares_and_map_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    text = open(os.path.join(ROOT, "inference-tools_amd", "csrc", "gpmi.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = re.findall(r"[\w*]+(?=;)", text.split("global:")[1].split("local:")[0])
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(\s*gpmi_sgp\s*\*", header), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), (name, exported)


def test_library_prototypes_name_the_entry_points():
    from inference_amd import _lib

    src = inspect.getsource(_lib)
    for name in NEW_ENTRY_POINTS:
        assert f'"{name}"' in src, name


def test_regressor_has_the_new_methods():
    from inference_amd.gp import SparseGpRegressor

    for name in ("set_inducing_points", "optimise_inducing_points", "marginal_likelihood_gradient"):
        assert callable(getattr(SparseGpRegressor, name, None)), name
    assert "optimise_inducing" in inspect.signature(SparseGpRegressor.__init__).parameters
    sig = inspect.signature(SparseGpRegressor.optimise_inducing_points)
    assert sig.parameters["hyperpars"].default is True and sig.parameters["maxiter"].default == 200


def test_gradient_call_accepts_inducing_points():
    from inference_amd.gp import SparseGpRegressor

    par = inspect.signature(SparseGpRegressor.marginal_likelihood_gradient).parameters
    assert "inducing_points" in par and par["inducing_points"].default is False
