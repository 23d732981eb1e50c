"""
GPU tests of `MultiTargetGpRegressor` (gpmi_mt_*, csrc/api_multi.hip): T targets on one device factorisation.

Yardsticks: for SquaredExponential / RationalQuadratic one `OracleGp` per target column at theta_t = [m_t, theta]
(tests/multitarget_host.py: OracleColumns); for kernels the oracle lacks, one single-target `GpRegressor` per column with
`ConstantMean` fixed at m_t.  Tolerance: 1e-10 relative, the project's own for everything behind a factorisation.  Inputs
are workloads.synthetic_dataset / timing_theta and the target recipe of multitarget_host.make_targets.  Every test runs
with the engine's dense host-composition entry points (`*_dense`) made to raise.  A reference is computed once per case
and shared.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

import multitarget_host as mth
import workloads as wl
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-10

# name: (kernel parts, white noise, N, d, T, M)   - what each case reaches is in the table of the README section
CASES = {
    "a_se": (("se",), False, 130, 3, 3, 50),            # one row past a 128 tile of N
    "b_se_wn": (("se",), True, 300, 2, 129, 257),       # one target past a 128-row tile of the target rows; extra diagonal
    "c_rq": (("rq",), False, 257, 17, 1, 1),            # 64 KiB LDS builders
    "d_m52_se": (("m52", "se"), False, 200, 2, 5, 130),  # the sum path
    "e_se": (("se",), False, 640, 1, 130, 2049),        # a second 512 inverse block; the second chunk of the predict loop
}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, tol=RTOL, what=""):
    r = rel(a, b)
    print(f"{what}: {r:.2e}")
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"
    return r


@pytest.fixture(autouse=True)
def no_dense_path(monkeypatch):
    from inference_amd._engine import GpEngine

    def tripwire(name):
        def fail(*args, **kwargs):
            raise AssertionError(f"GpEngine.{name} called: a many-target model left the device path")

        return fail

    for name in dir(GpEngine):
        if name.endswith("_dense"):
            monkeypatch.setattr(GpEngine, name, tripwire(name))


def _kernel(parts, wn):
    import inference_amd.gp as gp

    cls = {"se": gp.SquaredExponential, "rq": gp.RationalQuadratic, "m52": gp.Matern52, "m32": gp.Matern32}
    cov = cls[parts[0]]()
    for p in parts[1:]:
        cov = cov + cls[p]()
    return cov + gp.WhiteNoise() if wn else cov


def _theta(parts, wn, y, d):
    if parts == ("m52", "se"):  # two components of different amplitude and length scales
        return np.array([np.log(y.std())] + [np.log(0.5)] * d + [np.log(0.5 * y.std())] + [0.0] * d)
    return mth.cov_theta(orc.RQ if parts == ("rq",) else orc.SE, y, d, wn)


_data, _models, _refs = {}, {}, {}


def data(name):
    if name not in _data:
        parts, wn, n, d, T, M = CASES[name]
        x, y, e = wl.synthetic_dataset(1, n, d)
        _data[name] = (x, mth.make_targets(x, y, T), e, _theta(parts, wn, y, d), wl.query_points(1, M, d))
    return _data[name]


def model(name):
    """The fitted model of a case (offsets: the column means), built once."""
    from inference_amd.gp import MultiTargetGpRegressor

    if name not in _models:
        parts, wn = CASES[name][:2]
        x, Y, e, theta, _ = data(name)
        _models[name] = MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=theta, kernel=_kernel(parts, wn))
    return _models[name]


def reference(name):
    """lml_t, gradient, alpha, means, sigma, leave-one-out predictions and likelihood of a case from its yardstick."""
    if name in _refs:
        return _refs[name]
    parts, wn = CASES[name][:2]
    x, Y, e, theta, pts = data(name)
    means = Y.mean(axis=0)
    if parts in (("se",), ("rq",)):
        cols = mth.OracleColumns(x, Y, e, orc.RQ if parts == ("rq",) else orc.SE, wn, means, theta)
        ref = dict(lml_t=cols.lml_t(theta), grad=cols.lml_gradient(theta)[1], alpha=cols.alpha(), loo_lik=cols.loo_likelihood(theta))
        ref["means"], ref["sigma"] = cols.predict(pts)
        ref["loo_mu"], ref["loo_sigma"] = cols.loo_predictions()
    else:
        from inference_amd.gp import GpRegressor

        ref = dict(lml_t=[], grad=0.0, alpha=[], means=[], loo_mu=[], loo_lik=0.0)
        for t in range(Y.shape[1]):
            th = np.concatenate([[means[t]], theta])
            gp = GpRegressor(x, Y[:, t], y_err=e, hyperpars=th, kernel=_kernel(parts, wn))
            ref["lml_t"].append(gp.marginal_likelihood(th))
            ref["grad"] = ref["grad"] + gp.marginal_likelihood_gradient(th)[1][1:]
            ref["alpha"].append(gp.alpha)
            mu, ref["sigma"] = gp(pts)
            ref["means"].append(mu)
            lmu, ref["loo_sigma"] = gp.loo_predictions()
            ref["loo_mu"].append(lmu)
            ref["loo_lik"] += gp.loo_likelihood(th)
            gp.engine.close()
        ref["lml_t"] = np.array(ref["lml_t"])
        for k in ("alpha", "means", "loo_mu"):
            ref[k] = np.stack(ref[k], axis=1)
    _refs[name] = ref
    return ref


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_one_model_per_target(name):
    gp, ref = model(name), reference(name)
    theta, pts = data(name)[3:]
    T, M = CASES[name][4:]
    check(gp.marginal_likelihood(theta, per_target=True), ref["lml_t"], what=f"{name} lml_t")
    check(gp.marginal_likelihood(theta), ref["lml_t"].sum(), what=f"{name} LML")
    lml, grad = gp.marginal_likelihood_gradient(theta)
    check(lml, ref["lml_t"].sum(), what=f"{name} LML of the gradient call")
    check(grad, ref["grad"], what=f"{name} gradient")
    assert gp.alpha.shape == ref["alpha"].shape == (gp.n_points, T)
    check(gp.alpha, ref["alpha"], what=f"{name} alpha")
    means, sigma = gp(pts)
    assert means.shape == (M, T) and sigma.shape == (M,)
    check(means, ref["means"], what=f"{name} means")
    check(sigma, ref["sigma"], what=f"{name} sigma")
    lmu, lsig = gp.loo_predictions()
    check(lmu, ref["loo_mu"], what=f"{name} loo means")
    check(lsig, ref["loo_sigma"], what=f"{name} loo sigma")
    check(gp.loo_likelihood(theta), ref["loo_lik"], what=f"{name} loo_likelihood")
    check(gp._lml_t, ref["lml_t"], what=f"{name} lml_t of the fit")


# ---- 2. one target is GpRegressor ---------------------------------------------------------------------------------------
def test_one_target_is_the_single_target_regressor():
    from inference_amd.gp import GpRegressor, MultiTargetGpRegressor, SquaredExponential

    x, Y, e, theta, pts = data("a_se")
    m0 = 0.3
    th = np.concatenate([[m0], theta])
    one = GpRegressor(x, Y[:, 0], y_err=e, hyperpars=th, kernel=SquaredExponential)
    gp = MultiTargetGpRegressor(x, Y[:, 0], y_err=e, hyperpars=theta, kernel=SquaredExponential, target_means=m0)
    assert gp.n_targets == 1 and gp.alpha.shape == (130, 1)
    check(gp.alpha[:, 0], one.alpha, what="alpha")
    mu, sig = gp(pts)
    rmu, rsig = one(pts)
    check(mu[:, 0], rmu, what="mean")
    assert np.array_equal(sig, rsig), "sigma is the same device path: the same bits"
    check(gp.marginal_likelihood(theta), one.marginal_likelihood(th), what="LML")
    lml, grad = gp.marginal_likelihood_gradient(theta)
    rl, rg = one.marginal_likelihood_gradient(th)
    check(lml, rl, what="LML of the gradient call")
    check(grad, rg[1:], what="gradient")
    lmu, lsig = gp.loo_predictions()
    rlmu, rlsig = one.loo_predictions()
    check(lmu[:, 0], rlmu, what="loo mean")
    check(lsig, rlsig, what="loo sigma")
    check(gp.loo_likelihood(theta), one.loo_likelihood(th), what="loo_likelihood")
    one.engine.close()
    gp.engine.close()


# ---- 3. permuting the target columns ----------------------------------------------------------------------------------
def test_permuted_target_columns():
    from inference_amd.gp import MultiTargetGpRegressor

    name = "b_se_wn"  # 129 targets: the permutation moves columns across the 128-row tile of the target rows
    gp = model(name)
    x, Y, e, theta, pts = data(name)
    perm = np.random.default_rng(11).permutation(Y.shape[1])
    assert perm[128] != 128 and (perm != np.arange(Y.shape[1])).sum() > 100
    pg = MultiTargetGpRegressor(x, Y[:, perm], y_err=e, hyperpars=theta, kernel=_kernel(*CASES[name][:2]))
    assert np.array_equal(pg.alpha, gp.alpha[:, perm]), "alpha: rows are independent in the row solves"
    mu, sig = gp(pts)
    pmu, psig = pg(pts)
    assert np.array_equal(pmu, mu[:, perm]), "means: one product per row"
    assert np.array_equal(psig, sig), "sigma does not see the targets"
    assert np.array_equal(pg.marginal_likelihood(theta, per_target=True), gp.marginal_likelihood(theta, per_target=True)[perm])
    check(pg.marginal_likelihood(theta), gp.marginal_likelihood(theta), 1e-13, "LML under the permutation")
    g0, g1 = gp.marginal_likelihood_gradient(theta), pg.marginal_likelihood_gradient(theta)
    check(g1[0], g0[0], 1e-13, "LML of the gradient call under the permutation")
    check(g1[1], g0[1], 1e-13, "gradient under the permutation")
    pg.engine.close()


# ---- 4. repeatability and state -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_se", "b_se_wn"])
def test_repeated_calls_and_the_fit_keep_their_bits(name):
    gp = model(name)
    theta, pts = data(name)[3:]
    other = theta + 0.15
    fitted = (gp(pts), gp.engine.mt_alpha(), gp.loo_predictions())

    def same(a, b):
        if isinstance(a, tuple):
            return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
        return np.array_equal(np.asarray(a), np.asarray(b))

    calls = [lambda: gp.marginal_likelihood(other), lambda: gp.marginal_likelihood(other, per_target=True),
             lambda: gp.marginal_likelihood_gradient(other), lambda: gp.loo_likelihood(other),
             lambda: gp.marginal_likelihood_batch(np.array([theta, other])), lambda: gp(pts), lambda: gp.engine.mt_alpha(),
             lambda: gp.loo_predictions()]
    for k, f in enumerate(calls):
        assert same(f(), f()), f"call {k} repeated gave other bits"
    # ... and none of the evaluations at another theta has touched the fit
    again = (gp(pts), gp.engine.mt_alpha(), gp.loo_predictions())
    assert same(again, fitted), "the fit changed under evaluations at other hyper-parameters"
    lml_t = gp._lml_t.copy()
    gp.set_hyperparameters(theta)
    assert np.array_equal(gp._lml_t, lml_t) and same((gp(pts), gp.alpha, gp.loo_predictions()), fitted), "a second fit gave other bits"
    assert np.array_equal(gp.marginal_likelihood(theta, per_target=True), lml_t), "lane 1 and the fit disagree in lml_t"


# ---- 5. failures and limits ---------------------------------------------------------------------------------------------
def test_a_matrix_that_does_not_factorise():
    """-1e50 from marginal_likelihood and from the row of marginal_likelihood_batch, LinAlgError from set_hyperparameters;
    the model then still answers.  The matrix is made indefinite by an amplitude whose square overflows.  (Duplicated
    rows in x with length scales e^6 and no data errors, the other recipe for a singular matrix, are printed as well: the
    a^2 1e-12 jitter of the covariance builders keeps that matrix positive definite - the CPU oracle factorises it too,
    smallest diagonal of L 5.8e-7 - so no failure is asserted for it, only that all three calls agree.)"""
    from numpy.linalg import LinAlgError

    from inference_amd.gp import MultiTargetGpRegressor, SquaredExponential

    x, y, _ = wl.synthetic_dataset(1, 65, 3)
    x = np.vstack([x, x])
    Y = mth.make_targets(x, np.concatenate([y, y]), 3)
    good = mth.cov_theta(orc.SE, y, 3)
    gp = MultiTargetGpRegressor(x, Y, hyperpars=good, kernel=SquaredExponential)  # (y_err = None)
    before = gp(x[:7])
    bad = good.copy()
    bad[0] = 400.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert gp.marginal_likelihood(bad) == -1e50
        assert np.array_equal(gp.marginal_likelihood(bad, per_target=True), np.full(3, -1e50))
        vals = gp.marginal_likelihood_batch(np.array([good, bad, good]))
        assert gp.loo_likelihood(bad) == -1e50
    assert vals[1] == -1e50 and vals[0] == vals[2] == gp.marginal_likelihood(good)
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_gradient(bad)
    with pytest.raises(LinAlgError):
        gp.set_hyperparameters(bad)
    gp.set_hyperparameters(good)
    after = gp(x[:7])
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    flat = np.array([good[0], 6.0, 6.0, 6.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        value = gp.marginal_likelihood(flat)
        row = gp.marginal_likelihood_batch(flat[None, :])[0]
    try:
        gp.set_hyperparameters(flat)
        fitted = True
    except LinAlgError:
        fitted = False
    print(f"duplicated rows, length scales e^6: marginal_likelihood {value}, fit {'succeeds' if fitted else 'raises'}")
    assert row == value and fitted == (value != -1e50)
    gp.engine.close()


def test_calls_out_of_order_return_an_argument_error():
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    x, Y, e, theta, pts = data("a_se")
    R = np.ascontiguousarray(Y - Y.mean(axis=0)[None, :])
    eng = GpEngine(x, np.zeros(len(x)), noise_var=e**2)
    arg_error = dict(match="status -1")  # GPMI_ERR_ARG
    with pytest.raises(_lib.GpmiError, **arg_error):
        eng.mt_targets = 3
        eng.mt_fit(_lib.KERNEL_SE, theta, 0.0)
    for T in (0, _lib.MT_MAX_T + 1):
        rc = eng.h.lib.gpmi_mt_set_targets(eng.h.ctx, _lib.dptr(R), T)
        assert rc == -1 and b"GPMI_MT_MAX_T" in eng.h.lib.gpmi_last_error(eng.h.ctx)
    eng.mt_set_targets(R)
    for call in (eng.mt_alpha, lambda: eng.mt_predict(pts), eng.mt_loo):
        with pytest.raises(_lib.GpmiError, **arg_error):
            call()
    lml, lml_t, info = eng.mt_fit(_lib.KERNEL_SE, theta, 0.0)
    assert info == 0
    first = (eng.mt_predict(pts), eng.mt_alpha())
    # a single-target fit on the same handle takes lane 0: the many-target answers are refused until the next gpmi_mt_fit
    eng.fit(_lib.KERNEL_SE, theta, 0.0, np.zeros(len(x)))
    with pytest.raises(_lib.GpmiError, **arg_error):
        eng.mt_alpha()
    # a new data set drops the targets
    noise = _lib.as_f64(e**2)
    eng.h.call("gpmi_set_data", _lib.dptr(eng.x), _lib.dptr(eng.y), _lib.dptr(noise), None, eng.n, eng.d)
    for call in (lambda: eng.mt_lml(_lib.KERNEL_SE, theta, 0.0), lambda: eng.mt_fit(_lib.KERNEL_SE, theta, 0.0),
                 lambda: eng.mt_lml_grad(_lib.KERNEL_SE, theta, 0.0), lambda: eng.mt_loo_terms(_lib.KERNEL_SE, theta, 0.0)):
        with pytest.raises(_lib.GpmiError, **arg_error):
            call()
    # ... and the handle still fits and predicts, with the bits of the first time
    eng.mt_set_targets(R)
    assert eng.mt_fit(_lib.KERNEL_SE, theta, 0.0)[0] == lml
    again = (eng.mt_predict(pts), eng.mt_alpha())
    assert np.array_equal(again[0][0], first[0][0]) and np.array_equal(again[0][1], first[0][1])
    assert np.array_equal(again[1], first[1])
    eng.close()


def test_the_most_targets_once():
    """T = GPMI_MT_MAX_T on N = 130: a memory-shape test (32 tiles of target rows on two tiles of points), checked
    against the NumPy mirror, whose factorisation is one for all targets as well."""
    from inference_amd import _lib
    from inference_amd.gp import MultiTargetGpRegressor, SquaredExponential

    x, _, e, theta, pts = data("a_se")
    _, y, _ = wl.synthetic_dataset(1, 130, 3)
    T = _lib.MT_MAX_T
    Y = mth.make_targets(x, y, T)
    gp = MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    mirror = mth.MultiTargetMirror(x, Y, e, orc.SE, False, None, theta)
    assert gp.alpha.shape == (130, T)
    check(gp.alpha, mirror.alpha, what="alpha")
    check(gp._lml_t, mirror.marginal_likelihood(theta, per_target=True), what="lml_t")
    mu, sig = gp(pts)
    rmu, rsig = mirror(pts)
    check(mu, rmu, what="means")
    check(sig, rsig, what="sigma")
    lml, grad = gp.marginal_likelihood_gradient(theta)
    rl, rg = mirror.marginal_likelihood_gradient(theta)
    check(lml, rl, what="LML")
    check(grad, rg, what="gradient")
    check(gp.loo_likelihood(theta), mirror.loo_likelihood(theta), what="loo_likelihood")
    gp.engine.close()


def test_the_handle_gives_its_memory_back():
    """The target rows and every workspace of the many-target calls are the handle's: gone with it, to the byte."""
    from inference_amd import _lib
    from inference_amd.gp import MultiTargetGpRegressor, SquaredExponential

    def live():
        out = (C.c_int64 * 2)()
        assert _lib.load().gpmi_live_bytes(out) == 0
        return out[0], out[1]

    x, Y, e, theta, pts = data("a_se")
    start = live()
    gp = MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    gp(pts), gp.alpha, gp.loo_predictions(), gp.marginal_likelihood_gradient(theta), gp.loo_likelihood(theta)
    held = live()
    assert held[0] > start[0] + 8 * 128 * (256 + 32) * 2, "the target rows are device memory of the handle"
    gp.engine.mt_set_targets(Y[:, :2] - Y[:, :2].mean(axis=0)[None, :])  # (replaces the three targets and their workspaces)
    assert live()[0] < held[0]
    gp.engine.close()
    assert live() == start


# ---- 6. the search ------------------------------------------------------------------------------------------------------
def test_the_search_ends_inside_its_bounds_and_above_its_starts():
    from inference_amd.gp import MultiTargetGpRegressor, SquaredExponential

    x, Y, e, _, _ = data("a_se")
    np.random.seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp = MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=None, kernel=SquaredExponential, n_starts=3)
    log = gp.search_log
    assert log["starts"].shape == (3, 4) and log["start_values"].shape == (3,) and log["values"].shape == (3,)
    for v, (lo, hi) in zip(gp.hyperpars, gp.hp_bounds):
        assert lo <= v <= hi
    found = gp.marginal_likelihood(gp.hyperpars)
    print(f"search: start values {log['start_values']}, optima {log['values']}, chosen {found}")
    assert found >= log["start_values"].max()
    assert found == pytest.approx(log["values"].max(), rel=1e-12)
    gp.engine.close()
