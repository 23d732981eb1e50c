"""GPU tests of the sparse model's joint posterior, joint draws and derivatives by the query point (gpmi_sgp_posterior,
gpmi_sgp_posterior_draws, gpmi_sgp_spatial_derivatives and the SparseGpRegressor methods on them) against the NumPy mirror
tests/sparse_post_host.py.

Tolerances are not fixed numbers (the rule of tests/test_sparse_gpu.py): the mirror's K_mm, K_mn and K_mq entries are
rippled by 1e-13 relative 48 times; a quantity's allowance is 10 x its largest movement under those ripples, floored at
1e-10 x its scale (max |mu|, max diag Sigma, max |d mean|, max |d var|).  Each test prints the device's error next to the
allowance.

Cases: the five of tests/test_sparse_gpu.py (same construction).  Query sets: M points uniform in the data's box, q[1] a row
of x, q[2] a row of Z (M >= 3); M = 1, 65 (two 64-tiles of the derivative kernel, the second ragged), 130 (two 128-tiles of
Sigma, ragged), and 1025 (crosses the query panel) in case 1.

Measured on one MI355X, device error / allowance (also in the README, "Large data: inducing points"; printed by
`pytest -m gpu -s tests/test_sparse_post_gpu.py`):
  case  M     mu                   Sigma                d mean               d var
  1     1     1.4e-13 / 6.1e-11    1.7e-15 / 4.4e-12    2.1e-12 / 4.9e-11    3.0e-14 / 3.2e-11
  1     65    5.6e-13 / 1.1e-10    9.2e-15 / 3.4e-11    3.1e-12 / 3.0e-10    8.8e-14 / 1.8e-10
  1     130   5.3e-13 / 1.2e-10    8.3e-15 / 3.5e-11    3.6e-12 / 2.7e-10    9.1e-14 / 1.9e-10
  1     1025  6.4e-13 / 1.2e-10    1.6e-14 / 4.9e-11    4.0e-12 / 3.1e-10    1.6e-13 / 1.7e-10
  2     1     2.0e-11 / 1.9e-10    1.8e-13 / 2.7e-12    4.5e-10 / 8.2e-09    4.1e-12 / 6.8e-11
  2     65    1.3e-10 / 7.2e-10    6.0e-13 / 1.0e-11    3.7e-09 / 2.7e-08    2.6e-11 / 2.6e-10
  2     130   1.8e-10 / 9.3e-10    3.1e-12 / 1.5e-11    3.7e-09 / 2.7e-08    6.5e-11 / 5.1e-10
  3     1     2.5e-13 / 6.5e-11    3.6e-16 / 2.0e-11    1.7e-12 / 1.1e-10    1.8e-15 / 1.6e-11
  3     65    3.0e-12 / 1.5e-10    6.1e-15 / 2.4e-11    3.4e-12 / 1.2e-10    7.9e-15 / 2.1e-11
  3     130   3.0e-12 / 1.5e-10    5.2e-15 / 2.8e-11    3.9e-12 / 1.3e-10    7.9e-15 / 2.2e-11
  4     1     2.2e-16 / 5.9e-11    3.3e-16 / 9.8e-11    2.8e-17 / 4.1e-12    2.1e-17 / 4.9e-12
  4     65    6.7e-16 / 1.1e-10    6.4e-16 / 1.0e-10    4.9e-17 / 6.0e-12    6.2e-17 / 8.9e-12
  4     130   6.7e-16 / 1.1e-10    6.4e-16 / 1.0e-10    5.6e-17 / 5.9e-12    5.6e-17 / 9.7e-12
  5     1     1.4e-14 / 2.5e-11    3.6e-15 / 1.2e-10    4.4e-12 / 2.2e-09    2.5e-12 / 1.4e-09
  5     65    2.5e-14 / 1.4e-10    2.7e-14 / 1.2e-10    3.6e-12 / 2.4e-08    2.8e-12 / 2.0e-08
  5     130   6.0e-14 / 1.4e-10    2.5e-14 / 1.2e-10    1.2e-11 / 2.3e-08    6.4e-12 / 2.2e-08
diag Sigma against gpmi_sgp_predict's variance, closest to its allowance: 3.9e-16 / 4.4e-12
general z, case 1 M = 129, 8 draws: 4.1e-11 / 2.3e-09
z = I, case 1 M = 130: L L^T 8.3e-15 / 3.5e-11, eps 5.5e-24 / 3.5e-20
z = I, case 2 M = 130: L L^T 3.1e-12 / 1.5e-11, eps 6.4e-23 / 1.5e-20
z = I, case 3 M = 130: L L^T 5.2e-15 / 2.8e-11, eps 8.8e-25 / 2.8e-20
z = I, case 4 M = 1: L L^T 3.3e-16 / 9.8e-11, eps 4.1e-25 / 9.8e-20
recovered normals against gpmi_draws_normals (case 4, M = 1): 1.7e-16 (allowed 1e-12); acquisition gradients against
fourth-order differences (case 1, 65 points): UpperConfidenceBound 5.0e-8 / 7.5e-6, ExpectedImprovement 4.6e-5 / 7.0e-3
(max |gradient| 5.0 and 1.0e3).
"""
import ctypes as C
import pickle

import numpy as np
import pytest

import sparse_host as sh
import sparse_post_host as sph
from sparse_host import MU, N_RIPPLES, case as _case, check, full_theta, make_gp

pytestmark = pytest.mark.gpu

JITTER = 1e-9  # of the draws
SIZES = {1: (1, 65, 130, 1025, 129), 2: (1, 65, 130), 3: (1, 65, 130), 4: (1, 65, 130), 5: (1, 65, 130)}


def queries(case, M):
    q = np.random.default_rng(700 + 10 * case["number"] + M).uniform(0.0, 1.0, size=(M, case["x"].shape[1]))
    if M >= 3:
        q[1] = case["x"][len(case["x"]) // 2]
        q[2] = case["z"][len(case["z"]) // 2]
    return q


def _quantities(case, mir, ripple=None):
    """The mirror's mu, Sigma and derivatives at every query set of the case, from one state."""
    mir.ripple = ripple or (lambda name, A: A)
    nv = None if case["e"] is None else case["e"] ** 2
    st = mir.state(case["theta"], case["white"], case["y"] - MU, nv)
    out = {}
    for M in SIZES[case["number"]]:
        q = queries(case, M)
        mu, sigma = sph.posterior(mir, st, case["theta"], q)
        out[M, "mu"], out[M, "sigma"], out[M, "var"] = mu + MU, sigma, np.diag(sigma).copy()
        if M != 129:
            out[M, "dmean"], out[M, "dvar"] = sph.derivatives(mir, st, case["theta"], q)
        else:
            out[M, "draws"] = sph.draws(mu + MU, sigma, general_z(), JITTER)[0]
    return out


def general_z():
    return np.random.default_rng(99).standard_normal((8, 129))


_REFERENCE = {}


def reference(number):
    """(case, mirror quantities, allowances), computed once per case and shared by the tests."""
    if number not in _REFERENCE:
        case = _case(number)
        mir = sh.SparseMirror(case["kind"], case["x"], case["z"])
        base = _quantities(case, mir)
        spread = {k: 0.0 for k in base}
        for i in range(N_RIPPLES):
            moved = _quantities(case, mir, sh.rippler(1000 * number + i))
            for k in base:
                spread[k] = max(spread[k], float(np.abs(moved[k] - base[k]).max()))
        allow = {}
        for k, v in base.items():
            scale = float(np.abs(base[k[0], "var"]).max()) if k[1] in ("sigma", "var") else float(np.abs(v).max())
            allow[k] = 10.0 * spread[k] if k[1] == "draws" else max(10.0 * spread[k], 1e-10 * scale)
        _REFERENCE[number] = (case, base, allow)
    return _REFERENCE[number]


_MODELS = {}


def model(number):
    """The fitted device model of a case, shared by the tests that do not change it."""
    if number not in _MODELS:
        _MODELS[number] = make_gp(reference(number)[0])
    return _MODELS[number]


POINTS = [(n, M) for n in (1, 2, 3, 4, 5) for M in (1, 65, 130)] + [(1, 1025)]


@pytest.mark.parametrize("number,M", POINTS)
def test_posterior_and_derivatives_against_the_mirror(number, M):
    case, base, allow = reference(number)
    gp, q = model(number), queries(case, M)
    tag = f"case {number} M = {M}"
    mu, sigma = gp.build_posterior(q)
    assert mu.shape == (M,) and sigma.shape == (M, M)
    assert np.array_equal(sigma, sigma.T)
    check(f"{tag} mu", mu, base[M, "mu"], allow[M, "mu"])
    check(f"{tag} Sigma", sigma, base[M, "sigma"], allow[M, "sigma"])
    assert np.array_equal(gp.build_posterior(q, mean_only=True), mu)
    _, var = gp.engine.predict(q)
    check(f"{tag} diag Sigma against the predictive variance", np.diag(sigma), var, allow[M, "var"])
    dmean, dvar = gp.spatial_derivatives_batch(q)
    assert dmean.shape == q.shape and dvar.shape == q.shape
    check(f"{tag} d mean", dmean, base[M, "dmean"], allow[M, "dmean"])
    check(f"{tag} d var", dvar, base[M, "dvar"], allow[M, "dvar"])
    only_mean, none = gp.engine.spatial_derivatives(q, want_var=False)
    assert none is None and np.array_equal(only_mean, dmean)


@pytest.mark.parametrize("number", [2, 1, 4])
def test_a_derivative_row_does_not_depend_on_the_batch(number):
    """Row 700 of a 1025-point call, the point alone, and the point as row 0 of a 65-point call: case 2 (two tile rows of
    inducing points: the products on 64 x 64 tiles), and cases 1 and 4 (one tile column: the products' other tile shapes;
    case 4 on the large-LDS path)."""
    case, _, _ = reference(number)
    eng = model(number).engine
    big, small = queries(case, 1025), queries(case, 65).copy()
    small[0] = big[700]
    a = eng.spatial_derivatives(big)
    again = eng.spatial_derivatives(big)
    assert np.array_equal(a[0], again[0]) and np.array_equal(a[1], again[1])
    alone = eng.spatial_derivatives(big[700:701])
    first = eng.spatial_derivatives(small)
    for k in (0, 1):
        assert np.array_equal(a[k][700], alone[k][0]), k
        assert np.array_equal(a[k][700], first[k][0]), k


@pytest.mark.parametrize("number,M", [(1, 130), (2, 130), (3, 130), (4, 1)])
def test_factor_identity(number, M):
    """z = I: draws - mu is L^T, and L L^T = Sigma + eps I."""
    case, base, allow = reference(number)
    gp, q = model(number), queries(case, M)
    D, mu, eps, info = gp.engine.posterior_draws(q, n_draws=M, z=np.eye(M), jitter=JITTER)
    assert info == 0
    maxd = float(base[M, "var"].max())
    check(f"case {number} M = {M} eps", eps, JITTER * maxd, JITTER * allow[M, "var"] + 4e-16 * JITTER * maxd)  # (+ the product's own rounding)
    check(f"case {number} M = {M} mu of the draws", mu + MU, base[M, "mu"], allow[M, "mu"])
    Lt = D - mu
    assert np.array_equal(np.tril(Lt, -1), np.zeros((M, M)))
    check(f"case {number} M = {M} L L^T", Lt.T @ Lt, base[M, "sigma"] + JITTER * maxd * np.eye(M), allow[M, "sigma"])


def test_general_normals_against_the_mirror_within_its_own_ripple_spread():
    case, base, allow = reference(1)
    gp, q = model(1), queries(case, 129)
    D = gp.sample_posterior(q, 8, z=general_z(), jitter=JITTER)
    assert D.shape == (8, 129) and gp.last_sample_seed is None
    check("case 1 M = 129 general z", D, base[129, "draws"], allow[129, "draws"])


def test_rows_of_the_stream():
    case, _, _ = reference(1)
    gp, q = model(1), queries(case, 130)
    whole = gp.sample_posterior(q, 8, seed=7)
    assert gp.last_sample_seed == 7
    part = gp.sample_posterior(q, 5, seed=7, first_draw=3)
    assert np.array_equal(whole[3:8], part)
    assert np.array_equal(gp.sample_posterior(q, 8, seed=7), whole)
    assert not np.array_equal(gp.sample_posterior(q, 8, seed=8), whole)
    gp.sample_posterior(q, 1)
    assert isinstance(gp.last_sample_seed, int)


def test_generated_normals_at_one_point():
    """Case 4, M = 1: the draw is mu + sqrt(Sigma + eps) z.  The header documents <= 32 x 2^-53 r between the device's and
    the host's stream: 1e-12 (1 + |z|) leaves over thirty times that for the division and two roundings."""
    from inference_amd._engine import _seed_i64

    case, _, _ = reference(4)
    gp, q = model(4), queries(case, 1)
    eng = gp.engine
    n = 16
    D, mu, eps, info = eng.posterior_draws(q, n_draws=n, seed=2026, jitter=JITTER, first_draw=5)
    assert info == 0
    _, cov = eng.posterior(q)
    z = (D[:, 0] - mu[0]) / np.sqrt(cov[0, 0] + eps)
    host = np.zeros((n, 1))
    assert eng.h.lib.gpmi_draws_normals(_seed_i64(2026), 5, n, 1, host.ctypes.data_as(C.POINTER(C.c_double))) == 0
    err = np.abs(z - host[:, 0]) / (1.0 + np.abs(host[:, 0]))
    print(f"recovered normals against gpmi_draws_normals: {err.max():.3e} (allowed 1e-12)")
    assert err.max() <= 1e-12


def test_state_rules_and_untouched_fit():
    from inference_amd import _lib
    from inference_amd._engine import SparseEngine

    case, base, allow = reference(1)
    q = queries(case, 65)
    eng = SparseEngine(case["x"], case["z"])
    eng.set_targets(case["y"] - MU, case["e"] ** 2)
    calls = (lambda: eng.posterior(q), lambda: eng.posterior_draws(q, n_draws=2, seed=1), lambda: eng.spatial_derivatives(q))

    def refused():
        for call in calls:
            with pytest.raises(_lib.GpmiError, match="needs a successful gpmi_sgp_fit"):
                call()

    refused()  # before a fit
    args = (0, case["theta"], case["white"], 1e-8, case["panel"])  # (0: GPMI_KERNEL_SE)
    F, info = eng.fit(*args)
    assert info == 0
    before = eng.predict(q)

    def untouched(what):
        """The fit behind the call just made: the same predictions, and the same F from a bound evaluation, bit for bit."""
        after = eng.predict(q)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), what
        assert eng.bound(*args)[0] == F and eng.bound(*args)[3] == 0, what

    untouched("gpmi_sgp_bound itself")
    mu, sigma = eng.posterior(q)
    untouched("gpmi_sgp_posterior")
    check("posterior after the refused calls: mu", mu + MU, base[65, "mu"], allow[65, "mu"])
    check("posterior after the refused calls: Sigma", sigma, base[65, "sigma"], allow[65, "sigma"])
    D, _, _, info = eng.posterior_draws(q, n_draws=3, seed=5)
    untouched("gpmi_sgp_posterior_draws")
    assert info == 0 and np.isfinite(D).all()
    dmean, dvar = eng.spatial_derivatives(q)
    untouched("gpmi_sgp_spatial_derivatives")
    check("derivatives after the refused calls: d mean", dmean, base[65, "dmean"], allow[65, "dmean"])
    check("derivatives after the refused calls: d var", dvar, base[65, "dvar"], allow[65, "dvar"])
    eng.spatial_derivatives(q, want_var=False)
    untouched("gpmi_sgp_spatial_derivatives without the variance part")
    assert eng.posterior(np.zeros((0, 3)))[0].shape == (0,) and eng.spatial_derivatives(np.zeros((0, 3)))[0].shape == (0, 3)
    too_many = np.zeros((_lib.DRAWS_MAX_M + 1, 3))
    for call in (lambda: eng.posterior(too_many, mean_only=True), lambda: eng.posterior_draws(too_many, n_draws=1, seed=1)):
        with pytest.raises(_lib.GpmiError, match="mq out of range"):
            call()
    eng.set_inducing(case["z"])
    refused()  # the fit is dropped with the inducing inputs
    F2, info = eng.fit(*args)
    assert info == 0 and F2 == F
    again = eng.predict(q)
    assert np.array_equal(before[0], again[0]) and np.array_equal(before[1], again[1])
    mu2, sigma2 = eng.posterior(q)
    d2 = eng.spatial_derivatives(q)
    assert np.array_equal(mu2, mu) and np.array_equal(sigma2, sigma)
    assert np.array_equal(d2[0], dmean) and np.array_equal(d2[1], dvar)
    eng.close()


@pytest.mark.parametrize("d", [1, 3])
def test_python_surface(d):
    from inference_amd.gp import GpRegressor, Matern52, SparseGpRegressor

    x, y, e = sh.dataset(90, d, seed=8)
    theta = np.array([MU, 0.1] + [np.log(0.3)] * d)
    sparse = SparseGpRegressor(x if d > 1 else x[:, 0], y, y_err=e, inducing_points=12, seed=1, kernel=Matern52, hyperpars=theta)
    exact = GpRegressor(x if d > 1 else x[:, 0], y, y_err=e, kernel=Matern52, hyperpars=theta)
    many = np.random.default_rng(1).uniform(0.0, 1.0, size=(5, d))
    for pts in (many if d > 1 else many[:, 0], many[0] if d > 1 else 0.4):
        assert np.array_equal(sparse.process_points(pts), exact.process_points(pts))
        for name in ("spatial_derivatives", "spatial_derivatives_batch"):
            got, want = getattr(sparse, name)(pts), getattr(exact, name)(pts)
            assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (name, d)
        (mu_s, cov_s), (mu_e, cov_e) = sparse.build_posterior(pts), exact.build_posterior(pts)
        assert mu_s.shape == mu_e.shape and cov_s.shape == cov_e.shape
        assert sparse.build_posterior(pts, mean_only=True).shape == mu_e.shape
        assert sparse.sample_posterior(pts, 4, seed=3).shape == exact.sample_posterior(pts, 4, seed=3).shape
    q = sparse.process_points(many if d > 1 else many[:, 0])
    raw, _ = sparse.engine.posterior(np.ascontiguousarray(q, dtype=float))
    assert np.array_equal(sparse.build_posterior(q)[0], raw + MU)  # the mean function is added
    zero_mean = sparse.sample_posterior(q, 2, seed=3) - MU
    raw_draws = sparse.engine.posterior_draws(np.ascontiguousarray(q, dtype=float), n_draws=2, seed=3)[0]
    assert np.abs(zero_mean - raw_draws).max() <= 1e-15
    with pytest.raises(ValueError, match="cannot be combined"):
        sparse.sample_posterior(q, 2, seed=3, z=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="must have shape"):
        sparse.sample_posterior(q, 2, z=np.zeros((3, 5)))
    clone = pickle.loads(pickle.dumps(sparse))
    for a, b in zip(clone.build_posterior(q), sparse.build_posterior(q)):
        assert np.array_equal(a, b)
    for a, b in zip(clone.spatial_derivatives_batch(q), sparse.spatial_derivatives_batch(q)):
        assert np.array_equal(a, b)
    assert np.array_equal(clone.sample_posterior(q, 3, seed=11), sparse.sample_posterior(q, 3, seed=11))


@pytest.mark.parametrize("name", ["UpperConfidenceBound", "ExpectedImprovement"])
def test_acquisition_functions_on_a_sparse_model(name):
    """`opt_func_gradient_batch` at 65 points against fourth-order differences of `opt_func_batch`; the allowance is ten
    times the difference between the differences at h = 1e-3 and 2e-3."""
    from inference_amd.gp import acquisition

    case, _, _ = reference(1)
    gp = model(1)
    acq = getattr(acquisition, name)()
    acq.update_gp(gp)
    assert acq.mu_max == case["y"].max()
    q = 0.1 + 0.8 * queries(case, 65)
    val, grad = acq.opt_func_gradient_batch(q)
    assert val.shape == (65,) and grad.shape == (65, 3)
    assert np.array_equal(val, acq.opt_func_batch(q))
    fd1, fd2 = sph.fd4_rows(acq.opt_func_batch, q, 1e-3), sph.fd4_rows(acq.opt_func_batch, q, 2e-3)
    tol = 10.0 * float(np.abs(fd1 - fd2).max())
    err = float(np.abs(grad - fd1).max())
    print(f"{name}: max |gradient| {np.abs(grad).max():.3g}, error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (name, err, tol)
    assert float(acq.opt_func(q[0])) == val[0]
