"""GPU tests of the prediction under a batch of hyper-parameter vectors and its mixture (csrc/predict_batch.hip, the
batched cross-covariance build of csrc/kbuild.hip, gpmi_predict_batch, `GpRegressor.predict_samples` /
`predict_marginalised`) against the host reference of tests/predict_host.py (the CPU oracle per vector, the two-pass
mixture in NumPy) and against the device's own one-at-a-time `set_hyperparameters` + `__call__`.

Tolerance of the parity comparisons: the project's 1e-10 relative, max|a - b| / max|b| per array (test_gpu_parity.check,
which records every comparison for the summary at the end of the run).  Hyper-parameters come from the middle half of
every `hp_bounds` interval, where the oracle's own two routes (solve_triangular, explicit L^-1) agree to 3e-12.  Everything
else in this file is bit for bit: `assert_array_equal`."""
import warnings

import numpy as np
import pytest
from numpy.linalg import LinAlgError
from numpy.testing import assert_array_equal

import predict_host as ph
import workloads as wl
from test_gpu_parity import check

pytestmark = pytest.mark.gpu

T_MAX = 65                # crosses the chunk of 64 rows
T_CASES = (1, 2, 7, 65)
PANEL = 256               # GPMI_PREDICT_PANEL
M_CASES = (1, 5, 128, 129, PANEL + 1)


def _kernel_and_mean(tag):
    from inference_amd import gp

    kinds, wn, mean, _, _, _ = ph.MODELS[tag]
    cov = None
    for k in kinds:
        part = gp.SquaredExponential() if k == wl.SE else gp.RationalQuadratic()
        cov = part if cov is None else cov + part
    if wn:
        cov = cov + gp.WhiteNoise()
    return cov, (gp.LinearMean() if mean == "linear" else gp.ConstantMean())


class Case:
    """One model: the device regressor, T_MAX seeded hyper-parameter vectors, PANEL + 1 points, and - computed once - the
    host reference and the device's own one-at-a-time predictions for all of them."""

    def __init__(self, tag):
        from inference_amd import gp

        self.tag = tag
        _, _, _, seed, n, d = ph.MODELS[tag]
        x, y, e = ph.dataset(tag)
        cov, mean = _kernel_and_mean(tag)
        cov.pass_spatial_data(x)
        mean.pass_spatial_data(x)
        cov.estimate_hyperpar_bounds(y)
        mean.estimate_hyperpar_bounds(y)
        self.thetas = ph.middle_half(list(mean.bounds) + list(cov.bounds), T_MAX, 100 + seed)
        self.points = wl.query_points(seed, max(M_CASES), d)
        cov, mean = _kernel_and_mean(tag)
        self.gp = gp.GpRegressor(x, y, y_err=e, hyperpars=self.thetas[0], kernel=cov, mean=mean)
        assert self.gp._lockstep_predict_ok() and self.gp.hp_bounds == list(self.gp.mean.bounds) + list(self.gp.cov.bounds)
        self.ref_means, self.ref_vars, bad = ph.samples(ph.host_model(tag), self.points, self.thetas)
        assert not bad.any()
        single = []
        for th in self.thetas:
            self.gp.set_hyperparameters(th)
            single.append(self.gp(self.points))
        self.gp.set_hyperparameters(self.thetas[0])
        self.one_means = np.array([s[0] for s in single])
        self.one_vars = np.array([s[1] for s in single]) ** 2


_cases = {}


@pytest.fixture(scope="module")
def case():
    def get(tag):
        if tag not in _cases:
            _cases[tag] = Case(tag)
        return _cases[tag]

    yield get
    _cases.clear()


@pytest.mark.parametrize("T", T_CASES)
@pytest.mark.parametrize("tag", sorted(ph.MODELS))
def test_parity_with_host_reference_and_single_predictions(case, tag, T):
    c = case(tag)
    th = c.thetas[:T]
    weights = np.random.default_rng(T).uniform(0.1, 1.0, T)
    for m in M_CASES:
        pts = c.points[:m]
        mean, std, means, stds = c.gp.predict_marginalised(pts, th, weights=weights, return_samples=True)
        assert mean.shape == (m,) and std.shape == (m,) and means.shape == (T, m) and stds.shape == (T, m)
        for name, rm, rv in (("host", c.ref_means[:T, :m], c.ref_vars[:T, :m]),
                             ("one at a time", c.one_means[:T, :m], c.one_vars[:T, :m])):
            check(means, rm, what=f"{tag} means vs {name}, T={T} m={m}")
            check(stds**2, rv, what=f"{tag} variances vs {name}, T={T} m={m}")
            mix_mean, mix_var = ph.mixture(rm, rv, weights)
            check(mean, mix_mean, what=f"{tag} mixture mean vs {name}, T={T} m={m}")
            check(std**2, mix_var, what=f"{tag} mixture variance vs {name}, T={T} m={m}")
        s_means, s_stds = c.gp.predict_samples(pts, th)
        assert_array_equal(s_means, means)
        assert_array_equal(s_stds, stds)


@pytest.mark.parametrize("tag", sorted(ph.MODELS))
def test_a_row_does_not_depend_on_its_batch(case, tag):
    """The same vector alone, at positions 0 and 6 of a batch of 7, and at position 64 of a batch of 65 (a chunk of its own
    behind a full one that ran as two half-batches)."""
    c = case(tag)
    pts = c.points[:129]
    star = c.thetas[0]
    alone = c.gp.predict_samples(pts, star[None, :])
    seven = c.gp.predict_samples(pts, np.vstack([star[None, :], c.thetas[1:6], star[None, :]]))
    many = c.gp.predict_samples(pts, np.vstack([c.thetas[1:65], star[None, :]]))
    for k in range(2):  # means, standard deviations
        assert_array_equal(seven[k][0], alone[k][0])
        assert_array_equal(seven[k][6], alone[k][0])
        assert_array_equal(many[k][64], alone[k][0])


@pytest.mark.parametrize("tag", ["a", "c", "d", "e"])
def test_mixture_identities(case, tag):
    c = case(tag)
    pts = c.points[:129]
    T = 7
    th = c.thetas[:T]
    mean, std, means, stds = c.gp.predict_marginalised(pts, th, return_samples=True)
    # default weights are full(T, 1 / T)
    mean_w, std_w = c.gp.predict_marginalised(pts, th, weights=np.full(T, 1.0 / T))
    assert_array_equal(mean_w, mean)
    assert_array_equal(std_w, std)
    # all the weight on one vector: that vector's prediction
    one = np.zeros(T)
    one[4] = 1.0
    mean_1, std_1 = c.gp.predict_marginalised(pts, th, weights=3.0 * one)
    assert_array_equal(mean_1, means[4])
    assert_array_equal(std_1, stds[4])
    # four copies of one vector at weight 1/4: its prediction
    mean_4, std_4 = c.gp.predict_marginalised(pts, np.repeat(th[2:3], 4, axis=0), weights=np.full(4, 0.25))
    assert_array_equal(mean_4, means[2])
    assert_array_equal(std_4, stds[2])
    # a permutation of (theta, weight) that leaves row 3 in place: its row bit for bit, the mixture to the last bits
    w = np.random.default_rng(3).uniform(0.1, 1.0, T)
    perm = np.array([5, 0, 6, 3, 1, 2, 4])
    a = c.gp.predict_marginalised(pts, th, weights=w, return_samples=True)
    b = c.gp.predict_marginalised(pts, th[perm], weights=w[perm], return_samples=True)
    assert_array_equal(b[2][3], a[2][3])
    assert_array_equal(b[3][3], a[3][3])
    assert_array_equal(b[2], a[2][perm])
    check(b[0], a[0], 1e-14, what=f"{tag} mixture mean under a permutation")
    check(b[1] ** 2, a[1] ** 2, 1e-14, what=f"{tag} mixture variance under a permutation")


@pytest.mark.parametrize("tag", ["b", "d"])
def test_means_do_not_depend_on_the_variance_being_asked_for(case, tag):
    c = case(tag)
    pts, th = c.points[:PANEL + 1], c.thetas[:7]
    mean, _, means, _ = c.gp.predict_marginalised(pts, th, return_samples=True)
    assert_array_equal(c.gp.predict_samples(pts, th, mean_only=True), means)
    assert_array_equal(c.gp.predict_marginalised(pts, th, mean_only=True), mean)
    only = c.gp.predict_marginalised(pts, th, mean_only=True, return_samples=True)
    assert len(only) == 2
    assert_array_equal(only[0], mean)
    assert_array_equal(only[1], means)


def _state(gp, pts):
    gp._L_cache = None  # the factor as it is on the device now
    return [np.array(gp.hyperpars, copy=True), np.array(gp.alpha, copy=True), np.array(gp.L, copy=True), *gp(pts)]


@pytest.mark.parametrize("tag", ["a", "d", "e"])
def test_fitted_state_is_untouched(case, tag):
    c = case(tag)
    pts = c.points[:37]
    before = _state(c.gp, pts)
    hyperpars = c.gp.hyperpars
    c.gp.predict_marginalised(c.points[:129], c.thetas[1:8], return_samples=True)
    c.gp.predict_samples(c.points[:5], c.thetas[1:3], mean_only=True)
    assert c.gp.hyperpars is hyperpars
    for b, a in zip(before, _state(c.gp, pts)):
        assert_array_equal(a, b)


# ---- a row that does not factorise ------------------------------------------------------------------------------------
def _failing_model(golden):
    """The `fail` fixture's model on the lockstep route: its indefinite data covariance is diagonal, so it is handed to the
    regressor as its vector of data variances (which the constructor, squaring y_err, cannot produce); theta_bad then has
    a negative pivot (the fixture's -1e50 sentinel case), theta_ok and its neighbours factorise."""
    from inference_amd import gp as gp_mod

    g = golden("fail")
    assert not (g["y_cov"] - np.diag(np.diagonal(g["y_cov"]))).any()
    gp = gp_mod.GpRegressor(g["x"], g["y"], y_err=np.full(len(g["y"]), 0.1), hyperpars=g["theta_ok"])
    gp.engine.h.close()
    gp._engine = None
    gp._noise_var = np.diagonal(g["y_cov"]).copy()
    gp.set_hyperparameters(g["theta_ok"])
    assert gp._lockstep_predict_ok()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert gp.marginal_likelihood(g["theta_bad"]) == -1e50
    ok = np.array([g["theta_ok"] + np.array([0.0, 0.1 * k, 0.0, 0.0]) for k in range(4)])
    return gp, np.vstack([ok[:2], g["theta_bad"][None, :], ok[2:]]), ok


def test_failed_row(golden):
    gp, thetas, good = _failing_model(golden)
    pts = wl.query_points(3, 129, 2)
    for call in (gp.predict_samples, gp.predict_marginalised):
        with pytest.raises(LinAlgError, match="Matrix is not positive definite"):
            call(pts, thetas)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        mean, std, means, stds = gp.predict_marginalised(pts, thetas, return_samples=True, failed="skip")
    assert len([w for w in caught if "Cholesky decomposition failure" in str(w.message)]) == 1
    assert np.isnan(means[2]).all() and np.isnan(stds[2]).all()
    assert np.isfinite(np.delete(means, 2, axis=0)).all() and np.isfinite(np.delete(stds, 2, axis=0)).all()
    assert np.isfinite(mean).all() and np.isfinite(std).all()
    # the entry point flags the row
    th = np.array([np.ascontiguousarray(t[gp.cov_slice][gp._stat_slice]) for t in thetas])
    info = gp.engine.predict_batch(gp._kernel_id, th, 0.0, pts, mu_const=thetas[:, 0])[4]
    assert info[2] != 0 and not np.delete(info, 2).any()
    # the mixture is the one over the four good vectors alone, and so are their rows
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean_g, std_g, means_g, stds_g = gp.predict_marginalised(pts, good, return_samples=True, failed="skip")
    assert_array_equal(mean, mean_g)
    assert_array_equal(std, std_g)
    assert_array_equal(np.delete(means, 2, axis=0), means_g)
    assert_array_equal(np.delete(stds, 2, axis=0), stds_g)
    # nothing factorises: NaN mixtures, no error from the device
    bad3 = np.repeat(thetas[2:3], 3, axis=0)
    with pytest.warns(UserWarning):
        mean_n, std_n = gp.predict_marginalised(pts[:5], bad3, failed="skip")
    assert np.isnan(mean_n).all() and np.isnan(std_n).all()


# ---- models outside the lockstep route: one vector at a time, the mixture on the host ------------------------------------
def _one_at_a_time_models(golden):
    from inference_amd import gp as gp_mod

    x, y, e = wl.synthetic_dataset(5, 48, 1)
    idx = np.arange(48)
    y_cov = np.diag(e**2) + 0.004 * np.exp(-np.abs(idx[:, None] - idx[None, :]) / 3.0)
    th = wl.timing_theta(wl.SE, y, 1)
    rng = np.random.default_rng(21)
    dense = gp_mod.GpRegressor(x, y, y_cov=y_cov, hyperpars=th)
    yield "dense y_cov", dense, th + 0.1 * rng.standard_normal((3, th.size)), wl.query_points(5, 21, 1)
    het = gp_mod.GpRegressor(x, y, y_err=e, kernel=gp_mod.SquaredExponential() + gp_mod.HeteroscedasticNoise(),
                             hyperpars=np.concatenate([th, np.full(48, np.log(0.05))]))
    th_het = np.array(het.hyperpars)
    yield "HeteroscedasticNoise", het, th_het + 0.1 * rng.standard_normal((3, th_het.size)), wl.query_points(5, 21, 1)
    g = golden("cp")
    cp = gp_mod.GpRegressor(g["x"], g["y"], y_err=g["y_err"], hyperpars=g["serq_thetas"][1],
                            kernel=gp_mod.ChangePoint(kernels=[gp_mod.SquaredExponential, gp_mod.RationalQuadratic]))
    yield "ChangePoint", cp, np.array(g["serq_thetas"][:3]), g["pts"][:21]


def test_one_at_a_time_route(golden):
    for name, gp, thetas, pts in _one_at_a_time_models(golden):
        assert not gp._lockstep_predict_ok() and len(thetas) == 3
        before = _state(gp, pts)
        hyperpars = gp.hyperpars
        w = np.array([0.5, 0.2, 0.3])
        mean, std, means, stds = gp.predict_marginalised(pts, thetas, weights=w, return_samples=True)
        assert gp.hyperpars is hyperpars
        for b, a in zip(before, _state(gp, pts)):
            assert_array_equal(a, b)
        single = []
        for th in thetas:
            gp.set_hyperparameters(th)
            single.append(gp(pts))
        gp.set_hyperparameters(hyperpars)
        one_means, one_vars = np.array([s[0] for s in single]), np.array([s[1] for s in single]) ** 2
        check(means, one_means, what=f"{name} means")
        check(stds**2, one_vars, what=f"{name} variances")
        mix_mean, mix_var = ph.mixture(one_means, one_vars, w)
        check(mean, mix_mean, what=f"{name} mixture mean")
        check(std**2, mix_var, what=f"{name} mixture variance")
        assert_array_equal(gp.predict_samples(pts, thetas, mean_only=True), means)
        gp.engine.h.close()


def test_boundary_of_the_lockstep_route():
    """Padded N = 4096, the largest lockstep size: T = 2, m = 129 against the one-at-a-time device path."""
    from inference_amd import gp as gp_mod

    x, y, e = wl.synthetic_dataset(17, 4096, 4)
    th = wl.timing_theta(wl.SE, y, 4)
    thetas = th + 0.05 * np.random.default_rng(17).standard_normal((2, th.size))
    pts = wl.query_points(17, 129, 4)
    gp = gp_mod.GpRegressor(x, y, y_err=e, hyperpars=th)
    assert gp.engine.capacity() == 4096 and gp._lockstep_predict_ok()
    mean, std, means, stds = gp.predict_marginalised(pts, thetas, return_samples=True)
    single = []
    for t in thetas:
        gp.set_hyperparameters(t)
        single.append(gp(pts))
    one_means, one_vars = np.array([s[0] for s in single]), np.array([s[1] for s in single]) ** 2
    check(means, one_means, what="N=4096 means")
    check(stds**2, one_vars, what="N=4096 variances")
    mix_mean, mix_var = ph.mixture(one_means, one_vars)
    check(mean, mix_mean, what="N=4096 mixture mean")
    check(std**2, mix_var, what="N=4096 mixture variance")
    gp.engine.h.close()
