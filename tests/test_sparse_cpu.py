"""CPU checks of the inducing-point model: the NumPy mirror (tests/sparse_host.py) against the dense definition, its
analytic gradient against finite differences, the limit Z = X against the exact regression of the two host references,
the constructor's argument errors, and the names of the C entry points.  No device call is made.

Every tolerance is 10 x the difference measured on the CPU between the two float64 routes (printed by each test)."""
import os
import re

import numpy as np
import pytest

import matern_host as mh
import sparse_host as sh

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = [(300, 3, 33), (257, 5, 64)]


def setup(kind, n, d, m):
    x, y, e = sh.dataset(n, d)
    z = x[sh.spread_rows(x, m)]
    theta = np.array([0.1] + [np.log(0.35)] * d)
    return sh.SparseMirror(kind, x, z), theta, y - 0.2, e**2


@pytest.mark.parametrize("kind", ["se", "m52"])
@pytest.mark.parametrize("n,d,m", CASES)
def test_mirror_equals_the_dense_definition(kind, n, d, m):
    """ln N(r | 0, Q + Sigma) - 1/2 tr(W (a^2 I - Q)) through the N x N matrix.  Measured |difference|: se 1.2e-11,
    3.9e-12; m52 1.6e-12, 1.8e-12 (F of order 10^3) -> 1.3e-10."""
    mir, theta, r, nv = setup(kind, n, d, m)
    cond = mir.cond_kmm(theta)
    assert cond <= 1e3, cond  # (measured: 262, 26, 49, 16)
    F, dense = mir.bound(theta, 0.01, r, nv), mir.dense_bound(theta, 0.01, r, nv)
    print(f"{kind} {n} {d} {m}: cond {cond:.3g}  F {F:.6f}  |F - dense| {abs(F - dense):.3g}")
    assert abs(F - dense) <= 1.3e-10


# measured |analytic - finite difference|, largest component: (kind, n): value
FD_MEASURED = {("se", 300): 1.91e-8, ("se", 257): 5.19e-9, ("m52", 300): 3.86e-9, ("m52", 257): 3.61e-9, ("rq", 300): 1.58e-8,
               ("rq", 257): 1.71e-8}  # on gradients of order 10^3


@pytest.mark.parametrize("kind", ["se", "m52", "rq"])
@pytest.mark.parametrize("n,d,m", CASES)
def test_mirror_gradient_against_finite_differences(kind, n, d, m):
    """Fourth-order central differences at h = 1e-3 of F by every kernel parameter, ln s and the constant mean."""
    mir, theta, r, nv = setup(kind, n, d, m)
    if kind == "rq":
        theta = np.concatenate([theta[:1], [0.3], theta[1:]])
    s2 = 0.01
    F, grad, alpha = mir.bound_and_gradient(theta, s2, r, nv)
    fd = sh.fd4(lambda t: mir.bound(t, s2, r, nv), theta)
    fd_s = sh.fd4(lambda t: mir.bound(theta, float(np.exp(2.0 * t[0])), r, nv), [0.5 * np.log(s2)])[0]
    fd_mu = sh.fd4(lambda t: mir.bound(theta, s2, r - t[0], nv), [0.0])[0]
    err = max(np.abs(fd - grad[:-1]).max(), abs(fd_s - grad[-1]), abs(fd_mu - alpha.sum()))
    print(f"{kind} {n}: |grad| {np.abs(grad).max():.4g}  |analytic - fd| {err:.3g}")
    assert err <= 10.0 * FD_MEASURED[(kind, n)]


def test_inducing_points_at_the_data_give_the_exact_regression():
    """Z = X, eps = 0, N = m = 130, d = 3: Q = K_nn, so the bound is the exact log marginal likelihood and the prediction
    the exact one - Matern52 against tests/matern_host.py's regression, SquaredExponential against oracle/gp_oracle.py's
    (which has no Matern kernel).  Both add a^2 1e-12 to the diagonal of K, which the sparse model does not: part of the
    measured differences.  Measured: m52 |dF| 1.2e-9, mean 3.6e-10, std 3.3e-10; se (cond(K) 5e8) 6.2e-9, 3.2e-9, 9.2e-9."""
    from oracle import gp_oracle as orc

    n, d = 130, 3
    x, y, e = sh.dataset(n, d)
    theta = np.array([0.1] + [np.log(0.35)] * d)
    full = np.concatenate([[0.2], theta])
    q = np.random.default_rng(3).uniform(0.0, 1.0, size=(17, d))
    refs = {"m52": mh.OracleGp(x, y, e, mh.HostModel([("m52",)], x), full),
            "se": orc.OracleGp(x, y, e, kernel=orc.SE, hyperpars=full)}
    allow = {"m52": (1.2e-8, 3.6e-9, 3.3e-9), "se": (6.2e-8, 3.2e-8, 9.2e-8)}
    for kind, ref in refs.items():
        mir = sh.SparseMirror(kind, x, x, jitter=0.0)
        st = mir.state(theta, 0.0, y - 0.2, e**2)
        mean, var = mir.predict(theta, 0.0, y - 0.2, e**2, q, st)
        exact = ref.marginal_likelihood(full) - 0.5 * n * sh.LN_2PI  # (both references leave the 2 pi constant out)
        mu, sig = ref(q)
        got = (abs(st["F"] - exact), np.abs(mean + 0.2 - mu).max(), np.abs(np.sqrt(np.abs(var)) - sig).max())
        print(kind, "F", st["F"], "differences", got)
        assert all(g <= a for g, a in zip(got, allow[kind])), (kind, got)


def test_constructor_argument_errors():
    """Raised on the host, before any device call (none of these creates a device object)."""
    from inference_amd.gp import (ChangePoint, ConstantMean, HeteroscedasticNoise, Matern52, RationalQuadratic, SparseGpRegressor,
                                  SquaredExponential, WhiteNoise)

    x, y, e = sh.dataset(40, 2)
    th = np.zeros(4)
    ok = dict(y_err=e, inducing_points=8, hyperpars=th)
    for bad in (SquaredExponential() + RationalQuadratic(), ChangePoint(kernels=[SquaredExponential, SquaredExponential]),
                SquaredExponential() + HeteroscedasticNoise(), SquaredExponential() + WhiteNoise() + WhiteNoise(),
                mh.HostKernel("m52")):
        with pytest.raises(NotImplementedError, match="SquaredExponential, RationalQuadratic, Matern32, Matern52"):
            SparseGpRegressor(x, y, kernel=bad, **ok)
    with pytest.raises(NotImplementedError, match="y_cov"):
        SparseGpRegressor(x, y, y_cov=np.diag(e**2), inducing_points=8, hyperpars=th)
    with pytest.raises(ValueError, match="needs noise"):
        SparseGpRegressor(x, y, inducing_points=8, hyperpars=th, kernel=Matern52)
    with pytest.raises(ValueError, match="inducing_points"):
        SparseGpRegressor(x, y, y_err=e, inducing_points=41, hyperpars=th)
    with pytest.raises(ValueError, match="inducing_points"):
        SparseGpRegressor(x, y, y_err=e, inducing_points=0, hyperpars=th)
    with pytest.raises(ValueError, match="inducing_points"):
        SparseGpRegressor(x, y, y_err=e, inducing_points=np.zeros((5, 3)), hyperpars=th)
    with pytest.raises(ValueError, match="jitter"):
        SparseGpRegressor(x, y, y_err=e, inducing_points=8, hyperpars=th, jitter=-1.0)
    with pytest.raises(ValueError):
        SparseGpRegressor(x, y[:-1], **ok)
    with pytest.raises(ValueError):
        SparseGpRegressor(x, y, y_err=e[:-1], inducing_points=8, hyperpars=th)
    with pytest.raises(ValueError):
        SparseGpRegressor(np.zeros((40, 65)), y, **ok)
    assert ConstantMean is not None


def test_header_map_and_ctypes_name_the_entry_points():
    from inference_amd import _lib

    names = ["gpmi_sgp_create", "gpmi_sgp_destroy", "gpmi_sgp_set_targets", "gpmi_sgp_bound", "gpmi_sgp_fit", "gpmi_sgp_predict"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmi.h")).read(), flags=re.S)
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "inference-tools_amd", "csrc", "gpmi.map")).read())
    import fnmatch

    for name in names:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported), name
        assert name in _lib.SIGNATURES
    for k, klass in enumerate(("BUILD", "GRAM", "FACTOR", "GRAD")):
        assert re.search(rf"#define GPMI_PROF_SGP_{klass} {13 + k}\b", header)
        assert getattr(_lib, f"PROF_SGP_{klass}") == 13 + k
    assert re.search(r"#define GPMI_PROF_NCLASS 17\b", header)
