"""
GPU tests of the posterior draws (include/gpmi.h: gpmi_posterior_draws, gpmi_mvn_draws; GpRegressor.sample_posterior,
GpLinearInverter.sample_posterior).  The reference has no sampler: the yardsticks are the NumPy mirror of
tests/draws_host.py (generator, draws_oracle), the NumPy / SciPy regression oracles of tests/matern_host.py and
oracle/gp_oracle.py for the posterior covariance, and - for the routes that take mean and covariance from existing,
golden-pinned entry points (ChangePoint, plugin kernels, GpLinearInverter) - that covariance itself with the derived
backward error of a Cholesky factorisation.  Shapes are the smallest that cross a 128-wide tile edge.
"""
import ctypes as C

import numpy as np
import pytest

import draws_host as dh
import matern_host as mh
import workloads as wl

pytestmark = pytest.mark.gpu

COV_TOL = 1e-10  # the project's posterior-covariance parity tolerance, relative to the largest diagonal entry
JITTER = 1e-9


def cholesky_bound(M, max_diag):
    """|A - L L^T| <= gamma_{M+1} |L| |L^T| <= gamma_{M+1} sqrt(a_ii a_jj) (Higham, Accuracy and Stability of Numerical
    Algorithms, theorem 10.3), times 4 for the blocked accumulation and the test's own product."""
    return 4.0 * (M + 2) * 2.0**-53 * max_diag


def se_wn_model(n=150, d=2):
    from inference_amd.gp import GpRegressor, SquaredExponential, WhiteNoise

    x, y, e = wl.synthetic_dataset(41, n, d)
    theta = np.array([y.mean(), np.log(y.std()), np.log(0.5), np.log(0.6), np.log(0.05)])
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential() + WhiteNoise())
    return gp, mh.OracleGp(x, y, e, mh.HostModel([("se",), ("wn",)], x), theta)


@pytest.fixture(scope="module")
def se_wn():
    return se_wn_model()


def factor_identity(sample, M, mu_want, target, tol, what):
    """With z = eye(M) the rows of D - mu are the columns of L: (D - mu)^T (D - mu) = L L^T, formed in long double, against
    `target` (Sigma + eps I, lower triangle) within `tol`.  D[s][j] is mu[j] exactly for j < s - the factor's zeroed upper
    triangle - so below the diagonal every row holds the same number as the last row, bit for bit."""
    D = sample(np.eye(M))
    assert D.shape == (M, M) and np.isfinite(D).all()
    below = np.tril_indices(M, -1)
    assert np.array_equal(D[below], np.broadcast_to(D[-1], (M, M))[below]), f"{what}: the factor's upper triangle is not zero"
    Lt = D.astype(np.longdouble) - np.asarray(mu_want, dtype=np.longdouble)[None, :]
    G = np.asarray(Lt.T @ Lt, dtype=np.float64)  # G[i][j] = sum_s L[i][s] L[j][s]
    err = float(np.abs(np.tril(G) - np.tril(target)).max())
    print(f"{what}: |L L^T - (Sigma + eps I)| = {err:.3e} (allowed {tol:.3e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return D


def device_case(gp, orc, pts, what):
    """The models gpmi_posterior_draws serves: the target is the CPU oracle's Sigma + eps I."""
    M = len(pts)
    mu_o, S_o = orc.build_posterior(pts)
    maxd = np.diagonal(S_o).max()
    target = dh.sym(S_o) + (JITTER * maxd) * np.eye(M)
    mu_bp = gp.build_posterior(pts, mean_only=True)
    D = factor_identity(lambda z: gp.sample_posterior(pts, M, z=z, jitter=JITTER), M, mu_bp, target, COV_TOL * maxd, what)
    # mu, where the draws hold it bare (below the diagonal of D), is build_posterior's to 1e-13 - and the oracle's to 1e-10
    scale = max(np.abs(mu_bp).max(), 1.0)
    assert np.abs(D[-1][:-1] - mu_bp[:-1]).max(initial=0.0) <= 1e-13 * scale
    assert np.abs(mu_bp - mu_o).max() <= 1e-10 * max(np.abs(mu_o).max(), 1.0)


# ---- 1. the device generator ------------------------------------------------------------------------------------------
def test_device_generator_against_mirror_and_host_entry_point(se_wn):
    """cov = I, mean = 0, jitter = 0: L = I, products with 1 and sums with 0 are exact, so the call returns the device's
    normals themselves.  m = 130: two column tiles, an even number of columns short of the padding."""
    gp, _ = se_wn
    eng = gp.engine
    m, n = 130, 5
    for seed, first in ((2026, 0), (-1, 2**32 + 3)):
        D, eps, info = eng.mvn_draws(np.zeros(m), np.eye(m), n_draws=n, seed=seed, jitter=0.0, first_draw=first)
        assert info == 0 and eps == 0.0
        want, r = dh.normals(seed, first, n, m, with_radius=True)
        ratio = float((np.abs(D - want) / (2.0**-53 * r)).max())
        host = np.empty((n, m))
        from inference_amd._engine import _seed_i64

        assert eng.h.lib.gpmi_draws_normals(_seed_i64(seed), first, n, m, host.ctypes.data_as(C.POINTER(C.c_double))) == 0
        ratio_host = float((np.abs(D - host) / (2.0**-53 * r)).max())
        print(f"seed {seed}, first draw {first}: device vs mirror {ratio:.2f}, device vs gpmi_draws_normals {ratio_host:.2f} "
              f"(in 2^-53 r; bound {dh.NORMAL_ULPS})")
        assert ratio <= dh.NORMAL_ULPS and ratio_host <= dh.NORMAL_ULPS
    # odd m: the last sine is dropped, nothing else moves
    D3, _, _ = eng.mvn_draws(np.zeros(3), np.eye(3), n_draws=2, seed=2026, jitter=0.0)
    D4, _, _ = eng.mvn_draws(np.zeros(4), np.eye(4), n_draws=2, seed=2026, jitter=0.0)
    assert np.array_equal(D3, D4[:, :3])


# ---- 2. the factor identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 128, 130, 257])
def test_factor_identity_se_white_noise(se_wn, M):
    gp, orc = se_wn
    device_case(gp, orc, wl.query_points(41, M, 2), f"SE + WhiteNoise, M = {M}")


def test_factor_identity_matern52():
    from inference_amd.gp import GpRegressor, Matern52

    x, y, e = wl.synthetic_dataset(42, 150, 2)
    theta = np.array([y.mean(), np.log(y.std()), np.log(0.7), np.log(0.9)])
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=Matern52)
    device_case(gp, mh.OracleGp(x, y, e, mh.HostModel([("m52",)], x), theta), wl.query_points(42, 130, 2), "Matern52")


def test_factor_identity_sum_of_kernels():
    from inference_amd.gp import GpRegressor, RationalQuadratic, SquaredExponential

    x, y, e = wl.synthetic_dataset(43, 150, 2)
    theta = np.array([y.mean(), np.log(y.std()), np.log(0.5), np.log(0.6), np.log(0.4 * y.std()), 0.3, np.log(1.1), np.log(0.9)])
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential() + RationalQuadratic())
    assert not gp._generic and gp._sum_kernels is not None
    device_case(gp, mh.OracleGp(x, y, e, mh.HostModel([("se",), ("rq",)], x), theta), wl.query_points(43, 130, 2), "SE + RQ")


def test_factor_identity_dense_y_cov():
    from inference_amd.gp import GpRegressor, SquaredExponential
    from oracle import gp_oracle as orc
    from ycov_builders import correlated_cov, correlated_cov_inputs

    x, y, _ = wl.synthetic_dataset(44, 150, 2)
    Y = correlated_cov(*correlated_cov_inputs(np.random.default_rng(44), 150))
    theta = np.array([y.mean(), np.log(y.std()), np.log(0.5), np.log(0.6)])
    gp = GpRegressor(x, y, y_cov=Y, hyperpars=theta, kernel=SquaredExponential)
    device_case(gp, orc.OracleGp(x, y, kernel=orc.SE, hyperpars=theta, y_cov=Y), wl.query_points(44, 130, 2), "dense y_cov")


def fallback_case(gp, pts, what):
    """ChangePoint and plugin kernels: mean and covariance are build_posterior's (existing code), the target is that
    covariance, the bound the factorisation's own backward error."""
    M = len(pts)
    mu, S = gp.build_posterior(pts)
    maxd = np.diagonal(S).max()
    target = dh.sym(S) + (JITTER * maxd) * np.eye(M)
    D = factor_identity(lambda z: gp.sample_posterior(pts, M, z=z, jitter=JITTER), M, mu, target, cholesky_bound(M, maxd), what)
    assert np.array_equal(D[-1][:-1], mu[:-1])  # (the same numbers went in)


def test_factor_identity_change_point_fallback():
    from inference_amd.gp import ChangePoint, GpRegressor, SquaredExponential

    x, y, e = wl.synthetic_dataset(45, 150, 2)
    s = np.log(y.std())
    theta = np.array([y.mean(), s, np.log(0.5), np.log(0.6), s - 0.3, np.log(0.8), np.log(0.4), 0.5, 0.05])
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=ChangePoint(kernels=[SquaredExponential, SquaredExponential]))
    assert gp._mix is not None
    fallback_case(gp, wl.query_points(45, 130, 2), "ChangePoint (gpmi_mvn_draws)")


def test_factor_identity_plugin_kernel_fallback():
    from inference_amd.gp import GpRegressor
    from inference_amd.gp.covariance import CovarianceFunction

    class Matern32(wl.Matern32Math, CovarianceFunction):
        pass

    x, y, e, _, thetas = wl.plugin_problem()
    gp = GpRegressor(x, y, y_err=e, hyperpars=thetas[0], kernel=Matern32)
    assert gp._generic
    fallback_case(gp, np.random.default_rng(46).uniform(0, 2, (130, 2)), "plugin kernel (gpmi_mvn_draws)")


# ---- 3. general z against the oracle ------------------------------------------------------------------------------------
def test_general_normals_against_oracle_within_its_own_ripple_spread():
    """SE, N = 300, d = 3, length scales 0.4, amplitude 1.3, y_err 0.05; M = 129 uniform points, 8 draws, jitter 1e-9.
    Allowance: ten times the largest movement of the oracle's own draws under 48 symmetric ripples of relative size 1e-13
    on its Sigma - computed without the code under test - and, as a condition, below 1e-9.

    The data: training and query points uniform on [0, 3]^3, 7.5 length scales a side.  The yardstick presupposes a
    well-conditioned case, and whether a case is one can be told from the oracle alone: its Sigma = K_qq - Q^T Q carries
    an ABSOLUTE rounding error of a few ulp of a^2 = 1.69, the ripples are RELATIVE to entries of the size of the
    posterior variance.  On the unit cube 300 points pin the function down to a variance of 0.03, and the oracle's own
    draws then lie 6.9e-11 from the draws it makes from Sigma in long double (6.7e-11 and 7.6e-11 from its own Sigma
    summed in two other orders), 20 times the 3.3e-12 its ripples move them: the allowance of 3.3e-11 would sit below the
    reference's own error.  (The device was 6.7e-11 from the oracle there, with the factor identities above at 2e-15.)
    On [0, 3]^3 the variance stays near the prior's and the oracle's own error is a tenth of the ripple spread.  The test
    asserts that condition too: the oracle's draws from its own Sigma and from the long-double Sigma agree within the
    ripple spread, so that the factor ten is there for the device's summation order and not for the yardstick."""
    from inference_amd.gp import GpRegressor, SquaredExponential

    rng = np.random.default_rng(47)
    x = rng.uniform(0.0, 3.0, (300, 3))
    y = np.sin(2.0 * x[:, 0]) * np.cos(1.5 * x[:, 1]) + 0.3 * x[:, 2] + 0.05 * rng.standard_normal(300)
    e = np.full(300, 0.05)
    pts = rng.uniform(0.0, 3.0, (129, 3))
    theta = np.array([y.mean(), np.log(1.3)] + [np.log(0.4)] * 3)
    model = mh.HostModel([("se",)], x)
    orc = mh.OracleGp(x, y, e, model, theta)
    mu_o, S_o = orc.build_posterior(pts)
    z = rng.standard_normal((8, 129))
    base = dh.draws_oracle(mu_o, S_o, JITTER, z)
    spread = 0.0
    for _ in range(48):
        r = rng.uniform(-1.0, 1.0, S_o.shape)
        r = np.triu(r) + np.triu(r, 1).T
        spread = max(spread, float(np.abs(dh.draws_oracle(mu_o, S_o * (1.0 + 1e-13 * r), JITTER, z) - base).max()))
    allowance = 10.0 * spread
    assert 0.0 < allowance < 1e-9, allowance
    S_ld = dh.posterior_covariance_longdouble(orc.K, model.cross(pts, x, theta[1:]), model.cross(pts, pts, theta[1:]))
    own = float(np.abs(dh.draws_oracle(mu_o, S_ld, JITTER, z) - base).max())
    assert own <= spread, f"not a well-conditioned case: the oracle's own rounding moves its draws by {own:.2e}, its ripples by {spread:.2e}"
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    got = gp.sample_posterior(pts, 8, z=z, jitter=JITTER)
    err = float(np.abs(got - base).max())
    print(f"draws vs oracle: {err:.3e}, allowance {allowance:.3e} (10 x the oracle's spread under 48 ripples of 1e-13); the oracle "
          f"against its long-double Sigma: {own:.3e}; draw scale {np.abs(base - mu_o).max():.2f}")
    assert err <= allowance


# ---- 4. independence from the batch -------------------------------------------------------------------------------------
def test_a_draw_does_not_depend_on_the_batch(se_wn):
    gp, _ = se_wn
    pts = wl.query_points(41, 130, 2)
    big = gp.sample_posterior(pts, 300, seed=99)
    assert gp.last_sample_seed == 99
    assert np.array_equal(gp.sample_posterior(pts, 3, seed=99), big[:3])
    assert np.array_equal(gp.sample_posterior(pts, 3, seed=99, first_draw=297), big[297:])
    assert np.array_equal(gp.sample_posterior(pts, 300, seed=99), big)  # run against run
    assert not np.array_equal(gp.sample_posterior(pts, 3, seed=100), big[:3])
    z = np.random.default_rng(5).standard_normal((300, 130))
    zbig = gp.sample_posterior(pts, 300, z=z)
    assert gp.last_sample_seed is None
    assert np.array_equal(gp.sample_posterior(pts, 3, z=z[:3]), zbig[:3])
    assert np.array_equal(gp.sample_posterior(pts, 3, z=z[297:]), zbig[297:])
    assert np.array_equal(gp.sample_posterior(pts, 300, z=z), zbig)
    # a seeded draw is the supplied-z draw of the generator's own normals, to the generator's few ulp
    zs = dh.normals(99, 0, 3, 130)
    assert np.abs(gp.sample_posterior(pts, 3, z=zs) - big[:3]).max() <= 1e-12
    # seed=None: 64 fresh bits, kept for a repeat
    a = gp.sample_posterior(pts, 2)
    assert 0 <= gp.last_sample_seed < 2**64 and np.array_equal(gp.sample_posterior(pts, 2, seed=gp.last_sample_seed), a)


def test_batch_independence_across_panels_and_tile_shapes(se_wn):
    """m = 1536 (12 column tiles): 3 draws run as 64 x 64 tiles, 4096 + 130 draws as two panels, the first of them - 32 row
    tiles, 384 tiles in all - as 128 x 128 tiles.  The rows must agree bit for bit."""
    gp, _ = se_wn
    m = 1536
    t = np.arange(m) / m
    cov = np.exp(-np.abs(t[:, None] - t[None, :]) / 0.1) + 0.5 * np.eye(m)
    mean = np.sin(6.0 * t)
    eng = gp.engine
    n = 4096 + 130
    big, _, info = eng.mvn_draws(mean, cov, n_draws=n, seed=7)
    assert info == 0 and np.isfinite(big).all()
    for first, k in ((0, 3), (4095, 3), (n - 3, 3)):
        part, _, _ = eng.mvn_draws(mean, cov, n_draws=k, seed=7, first_draw=first)
        assert np.array_equal(part, big[first:first + k]), (first, k)
    # loose sanity of the whole pipeline at this size: the sample covariance of 4226 draws is the matrix's, to sampling error
    emp = np.cov(big[:, ::97].T)
    assert np.abs(emp - cov[::97, ::97]).max() < 6.0 * 1.5 * np.sqrt(2.0 / n)


# ---- 5. failure handling ------------------------------------------------------------------------------------------------
def test_indefinite_covariance_reports_info_and_leaves_the_handle_usable(se_wn):
    gp, _ = se_wn
    eng = gp.engine
    dp = C.POINTER(C.c_double)
    mean, cov = np.zeros(2), np.diag([1.0, -1.0])
    out = np.full((4, 2), 123.25)
    eps, info = C.c_double(-1.0), C.c_int(-9)
    eng.h.call("gpmi_mvn_draws", 2, mean.ctypes.data_as(dp), cov.ctypes.data_as(dp), 0.0, 4, None, 11, 0,
               out.ctypes.data_as(dp), C.byref(eps), C.byref(info))
    assert info.value == 2 and (out == 123.25).all()
    for bad in (np.diag([-1.0, -2.0]), np.diag([np.nan, 1.0]), np.diag([np.inf, 1.0]), np.zeros((2, 2))):
        out[:] = 123.25
        info.value = -9
        eng.h.call("gpmi_mvn_draws", 2, mean.ctypes.data_as(dp), bad.ctypes.data_as(dp), 0.0, 4, None, 11, 0,
                   out.ctypes.data_as(dp), C.byref(eps), C.byref(info))
        assert info.value == 1 and (out == 123.25).all(), bad
    draws, _, info2 = eng.mvn_draws(mean, np.diag([1.0, -1.0]), n_draws=4, seed=11, jitter=0.0)
    assert draws is None and info2 == 2
    # the handle then serves a good call, and the fit behind it is intact
    good, _, info3 = eng.mvn_draws(np.ones(2), np.diag([4.0, 9.0]), n_draws=4, seed=11, jitter=0.0)
    z = dh.normals(11, 0, 4, 2)
    assert info3 == 0 and np.abs(good - (1.0 + z * np.array([2.0, 3.0]))).max() <= 1e-12
    assert np.isfinite(gp.sample_posterior(wl.query_points(41, 5, 2), 2, seed=1)).all()


def test_mvn_draws_needs_no_data_set():
    """gpmi_mvn_draws on a handle that has never seen gpmi_set_data: the same bits as on a regressor's handle."""
    from inference_amd import _lib
    from inference_amd._engine import _DrawsMixin

    class Bare(_DrawsMixin):
        def __init__(self):
            self.h = _lib.Handle()

    bare = Bare()
    t = np.arange(130) / 130.0
    cov = np.exp(-np.abs(t[:, None] - t[None, :]) / 0.3) + 0.1 * np.eye(130)
    a, eps, info = bare.mvn_draws(np.cos(t), cov, n_draws=5, seed=3)
    assert info == 0 and eps == JITTER * 1.1
    assert np.abs(a - dh.draws_oracle(np.cos(t), cov, JITTER, dh.normals(3, 0, 5, 130))).max() <= 1e-12
    gp, _ = se_wn_model(n=40)
    b, _, _ = gp.engine.mvn_draws(np.cos(t), cov, n_draws=5, seed=3)
    assert np.array_equal(a, b)
    bare.h.close()


def test_sample_posterior_raises_linalgerror_on_an_indefinite_model():
    """A plugin 'kernel' that is the negative of a squared exponential: with y_err = 1 the training matrix
    -a^2 C + I is positive definite (a^2 lambda_max(C) <= 20 a^2 = 0.2), the posterior covariance -a^2 C_qq - Q^T Q has a
    negative diagonal - not a covariance, and the call says so."""
    from inference_amd.gp import GpRegressor
    from inference_amd.gp.covariance import CovarianceFunction

    class NegativeSE(CovarianceFunction):
        def __init__(self):
            self.bounds = [(-5.0, 0.0)]
            self.n_params = 1
            self.hyperpar_labels = ["ln a"]

        def pass_spatial_data(self, x):
            self.x = np.asarray(x, dtype=float)

        def estimate_hyperpar_bounds(self, y):
            pass

        def __call__(self, u, v, theta):
            return -np.exp(2 * theta[0]) * np.exp(-0.5 * ((u[:, None, :] - v[None, :, :]) ** 2).sum(axis=2))

        def build_covariance(self, theta):
            return self(self.x, self.x, theta)

        def covariance_and_gradients(self, theta):
            K = self.build_covariance(theta)
            return K, [2.0 * K]

    rng = np.random.default_rng(48)
    x, y = rng.uniform(0, 1, (20, 2)), rng.standard_normal(20)
    gp = GpRegressor(x, y, y_err=np.ones(20), hyperpars=np.array([0.0, np.log(0.1)]), kernel=NegativeSE())
    pts = rng.uniform(0, 1, (6, 2))
    with pytest.raises(np.linalg.LinAlgError, match="leading minor of order 1 .*jitter = 1e-09"):
        gp.sample_posterior(pts, 3, seed=1)
    mu, sig = gp(pts)  # the handle still serves the model
    assert np.isfinite(mu).all()


# ---- 6. the fitted state ------------------------------------------------------------------------------------------------
def test_fitted_state_is_not_touched(se_wn):
    gp, _ = se_wn
    pts = wl.query_points(41, 130, 2)
    L0, (mu0, sig0), post0 = gp.engine.get_L(), gp(pts), gp.build_posterior(pts)
    alpha0 = gp.alpha.copy()
    gp.sample_posterior(pts, 5, seed=3)
    gp.sample_posterior(pts[:7], 200, z=np.ones((200, 7)))
    gp.engine.mvn_draws(np.zeros(300), np.eye(300), n_draws=2, seed=3)
    mu1, sig1 = gp(pts)
    post1 = gp.build_posterior(pts)
    assert np.array_equal(gp.engine.get_L(), L0) and np.array_equal(gp.alpha, alpha0)
    assert np.array_equal(mu1, mu0) and np.array_equal(sig1, sig0)
    assert np.array_equal(post1[0], post0[0]) and np.array_equal(post1[1], post0[1])


# ---- 7. GpLinearInverter ------------------------------------------------------------------------------------------------
def test_linear_inverter_factor_identity_at_130_parameters():
    """The factor identity of test 2 at 130 parameters on [-1, 1] seen through 40 Gaussian-blurred data values: L L^T against
    the CPU oracle's posterior covariance + eps I within the posterior-covariance parity tolerance, 1e-10 of the largest
    diagonal entry.  The mean that went in is calculate_posterior's, and comes back bit for bit below the diagonal.
    (This posterior is ill-conditioned - eigenvalues from 6e-3 down to eps = 6e-12 - and the factorisation, which applies
    explicit inverses of its 128 x 128 diagonal blocks, then leaves |L L^T - A| = 1.4e-13, measured on one MI355X against the
    device's own covariance: inside the tolerance here, far above the 3.6e-16 that the substitution-based bound of
    `cholesky_bound` would allow, which is why that bound is used for the well-conditioned fallback cases alone.)"""
    from inference_amd.gp import GpLinearInverter, SquaredExponential
    from oracle import gp_oracle as orc
    from oracle.linv_oracle import OracleLinearInverter

    n, m = 130, 40
    pos = np.linspace(-1.0, 1.0, n)
    t = np.linspace(-1.0, 1.0, m)
    A = np.exp(-0.5 * ((t[:, None] - pos[None, :]) / 0.08) ** 2)
    A /= A.sum(axis=1, keepdims=True)
    truth = 1.0 / (1.0 + (pos / 0.2) ** 2)
    rng = np.random.default_rng(49)
    y_err = np.full(m, 0.02)
    y = A @ truth + y_err * rng.standard_normal(m)
    gli = GpLinearInverter(y=y, y_err=y_err, model_matrix=A, parameter_spatial_positions=pos.reshape(n, 1),
                           prior_covariance_function=SquaredExponential)
    theta = np.array([0.2, np.log(0.6), np.log(0.15)])
    mean_o, cov_o = OracleLinearInverter(y, y_err, A, pos.reshape(n, 1), orc.SE).calculate_posterior(theta)
    mean, cov = gli.calculate_posterior(theta)
    maxd = np.diagonal(cov_o).max()
    target = dh.sym(cov_o) + (JITTER * maxd) * np.eye(n)
    D = factor_identity(lambda z: gli.sample_posterior(theta, n, z=z, jitter=JITTER), n, mean, target, COV_TOL * maxd,
                        "GpLinearInverter")
    assert np.array_equal(D[-1][:-1], mean[:-1])
    assert np.abs(mean - mean_o).max() <= 1e-10 * max(np.abs(mean_o).max(), 1.0)
    a = gli.sample_posterior(theta, 3, seed=5)
    assert gli.last_sample_seed == 5 and np.array_equal(gli.sample_posterior(theta, 2, seed=5, first_draw=1), a[1:])
    # the calls before and after leave the inverter's own results alone
    mean2, cov2 = gli.calculate_posterior(theta)
    assert np.array_equal(mean2, mean) and np.array_equal(cov2, cov)


# ---- 8. Python argument errors ------------------------------------------------------------------------------------------
def test_python_argument_errors(se_wn):
    gp, _ = se_wn
    pts = wl.query_points(41, 6, 2)
    z = np.zeros((3, 6))
    with pytest.raises(ValueError, match="seed"):
        gp.sample_posterior(pts, 3, seed=1, z=z)
    with pytest.raises(ValueError, match="first_draw"):
        gp.sample_posterior(pts, 3, z=z, first_draw=1)
    with pytest.raises(ValueError, match="shape"):
        gp.sample_posterior(pts, 3, z=z[:2])
    with pytest.raises(ValueError, match="shape"):
        gp.sample_posterior(pts, 3, z=np.zeros((3, 5)))
    from inference_amd._lib import GpmiError

    out = np.zeros(1)
    with pytest.raises(GpmiError, match="16384"):  # (the size is checked before any pointer is read)
        gp.engine.h.call("gpmi_mvn_draws", 16385, None, None, 0.0, 1, None, 0, 0, out.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert gp.sample_posterior(pts, 1, seed=2).shape == (1, 6)
