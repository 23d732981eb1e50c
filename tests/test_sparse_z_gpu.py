"""GPU tests of the gradient of the variational bound by the inducing inputs (gpmi_sgp_bound_zgrad), of
gpmi_sgp_set_inducing and of SparseGpRegressor.set_inducing_points / optimise_inducing_points, against the NumPy mirror
tests/sparse_z_host.py.

Allowances follow tests/test_sparse_gpu.py: the mirror's K_mm and K_mn entries are rippled by 1e-13 relative 48 times; the
allowance of dF/dZ is 10 x its largest movement under those ripples, floored at 1e-10 x max |dF/dZ|.  Each test prints the
device's error next to the allowance.

Cases (those of tests/test_sparse_gpu.py: the smallest shapes at which the device paths differ):
  1  SE + WhiteNoise, y_err   N = 300   d = 3   m = 33    panel_rows 128: three panels, the last ragged; Z rows of x
  2  Matern52, y_err          N = 2100  d = 2   m = 130   panel_rows 512: three tiles of inducing points, five panels
  3  RQ + WhiteNoise          N = 257   d = 17  m = 64    no y_err, one ragged panel, five chunks of dimensions
  4  Matern32, y_err          N = 200   d = 64  m = 1     the widest points (112 KiB of LDS), one inducing point
  5  SE, y_err                N = 70    d = 1   m = 129   more inducing points than data

Measured on one MI355X, dF/dZ device error / allowance (max |dF/dZ|); printed by `pytest -m gpu -s tests/test_sparse_z_gpu.py`:
  1     4.8e-10 / 7.4e-9    (7.4e1)       panel_rows 64 / 128 / 0: 4.8e-10 each
  2     3.2e-6  / 8.1e-6    (3.9e2)
  3     2.4e-8  / 5.5e-7    (9.7e1)
  4     1.3e-10 / 4.3e-8    (4.3e2)
  5     6.7e-10 / 2.5e-6    (2.5e4)
after the indefinite model's info = 2 (two coincident inducing points, eps = 1e-8 a^2): 2.9e-4 / 8.6e-3; end to end: F
1050.794 -> 1718.952 in 117 evaluations (exact log marginal likelihood at the final theta 1720.048), F 9.3e-5 from the
mirror (allowed 2.5e-4), mean 1.8e-5 (5.1e-5), variance 7.5e-7 (2.2e-6); over Z alone 1050.794 -> 1099.004.
"""
import pickle

import numpy as np
import pytest
from numpy.linalg import LinAlgError

import matern_host as mh
import sparse_host as sh
import sparse_z_host as szh
from sparse_host import MU, N_RIPPLES, case as _case, check, full_theta, make_gp

pytestmark = pytest.mark.gpu

GPMI_ERR_ARG = -1


def mirror_zgrad(case, seed=None, z=None, jitter=1e-8):
    mir = sh.SparseMirror(case["kind"], case["x"], case["z"] if z is None else z, jitter=jitter,
                          ripple=None if seed is None else sh.rippler(seed))
    nv = None if case["e"] is None else case["e"] ** 2
    return szh.inducing_gradient(mir, case["theta"], case["white"], case["y"] - MU, nv)


def zgrad_allowance(case, base, seed0, z=None, jitter=1e-8):
    spread = max(float(np.abs(mirror_zgrad(case, seed0 + i, z, jitter) - base).max()) for i in range(N_RIPPLES))
    return max(10.0 * spread, 1e-10 * float(np.abs(base).max()))


_REFERENCE = {}


def reference(number):
    """(case, the mirror's dF/dZ, its allowance), computed once per case and shared by the tests."""
    if number not in _REFERENCE:
        case = _case(number)
        base = mirror_zgrad(case)
        _REFERENCE[number] = (case, base, zgrad_allowance(case, base, 1000 * number))
    return _REFERENCE[number]


def device_bound(gp, case, zgrad=True, jitter=None):
    th, white = gp._split(full_theta(case))
    return gp.engine.bound(gp._kernel_id, th, white, gp.jitter if jitter is None else jitter, gp.panel_rows, True, True,
                           want_zgrad=zgrad)


@pytest.mark.parametrize("number", [1, 2, 3, 4, 5])
def test_zgrad_against_the_mirror(number):
    case, base, allow = reference(number)
    gp = make_gp(case)
    F, grad, gz = gp.marginal_likelihood_gradient(full_theta(case), inducing_points=True)
    assert gz.shape == case["z"].shape and grad.shape == full_theta(case).shape and np.isfinite(gz).all()
    print(f"case {number}: max |dF/dZ| {np.abs(base).max():.3e}")
    check(f"case {number} dF/dZ", gz, base, allow)


def test_the_other_results_keep_their_bits_and_repeats_are_bit_identical():
    case, _, _ = reference(1)
    gp = make_gp(case)
    q = np.random.default_rng(41).uniform(0.0, 1.0, size=(17, 3))
    before = gp(q)
    plain = device_bound(gp, case, zgrad=False)
    a = device_bound(gp, case)
    b = device_bound(gp, case)
    again = device_bound(gp, case, zgrad=False)
    assert len(plain) == 4 and len(a) == 5 and plain[3] == 0 and a[3] == 0 and b[3] == 0
    for other in (a, b, again):
        assert plain[0] == other[0] and np.array_equal(plain[1], other[1]) and np.array_equal(plain[2], other[2])
    assert np.array_equal(a[4], b[4])
    after = gp(q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    F2, g2 = gp.marginal_likelihood_gradient(full_theta(case))
    F3, g3, _ = gp.marginal_likelihood_gradient(full_theta(case), inducing_points=True)
    assert F2 == F3 and np.array_equal(g2, g3)


def test_panel_sizes_agree():
    """panel_rows 64 (rounded up to 128), 128 and 0 (one panel here) group the sums over the data differently."""
    case, base, allow = reference(1)
    for rows in (64, 128, 0):
        gp = make_gp(case, panel_rows=rows)
        check(f"panel_rows {rows} dF/dZ", device_bound(gp, case)[4], base, allow)


def test_set_inducing_equals_a_fresh_object_and_drops_the_fit():
    from inference_amd import _lib

    case, _, _ = reference(1)
    z2 = np.clip(case["z"] + np.random.default_rng(77).uniform(-0.03, 0.03, size=case["z"].shape), 0.0, 1.0)
    q = np.random.default_rng(42).uniform(0.0, 1.0, size=(9, 3))
    gp = make_gp(case)
    eng = gp.engine
    eng.set_inducing(z2)
    moved = device_bound(gp, case)
    fresh = device_bound(make_gp(case, z=z2), case)
    assert moved[3] == 0 and fresh[3] == 0 and moved[0] == fresh[0]
    for k in (1, 2, 4):
        assert np.array_equal(moved[k], fresh[k]), k
    # the fit of the constructor is gone: gpmi_sgp_predict is a bad call order until the next fit, the object stays usable
    mean, var = np.zeros(len(q)), np.zeros(len(q))
    rc = eng.h.lib.gpmi_sgp_predict(eng.ptr, _lib.dptr(q), len(q), _lib.dptr(mean), _lib.dptr(var))
    assert rc == GPMI_ERR_ARG
    with pytest.raises(_lib.GpmiError, match="gpmi_sgp_predict needs a successful gpmi_sgp_fit"):
        eng.predict(q)
    assert np.array_equal(device_bound(gp, case)[4], moved[4])
    th, white = gp._split(full_theta(case))
    F, info = eng.fit(gp._kernel_id, th, white, gp.jitter, gp.panel_rows)
    assert info == 0 and F == moved[0]
    ref = make_gp(case, z=z2)(q)
    got = eng.predict(q)
    assert np.array_equal(got[0] + MU, ref[0]) and np.array_equal(np.sqrt(np.abs(got[1])), ref[1])
    # a NaN is refused and the old inducing inputs stay
    bad = z2.copy()
    bad[5, 1] = np.nan
    assert eng.h.lib.gpmi_sgp_set_inducing(eng.ptr, _lib.dptr(bad)) == GPMI_ERR_ARG
    with pytest.raises(_lib.GpmiError, match="must be finite"):
        eng.set_inducing(bad)
    kept = device_bound(gp, case)
    assert kept[0] == moved[0] and np.array_equal(kept[1], moved[1]) and np.array_equal(kept[4], moved[4])
    with pytest.raises(ValueError):
        eng.set_inducing(z2[:-1])


def test_regressor_set_inducing_points():
    case, _, _ = reference(1)
    z2 = np.clip(case["z"] + np.random.default_rng(78).uniform(-0.03, 0.03, size=case["z"].shape), 0.0, 1.0)
    q = np.random.default_rng(43).uniform(0.0, 1.0, size=(9, 3))
    gp = make_gp(case)
    old_bound, old_pred = gp.bound, gp(q)
    for bad in (z2[:-1], z2[:, :2], np.where(np.arange(z2.size).reshape(z2.shape) == 4, np.inf, z2)):
        with pytest.raises(ValueError):
            gp.set_inducing_points(bad)
    assert np.array_equal(gp.inducing_points, case["z"]) and gp.bound == old_bound
    assert all(np.array_equal(a, b) for a, b in zip(gp(q), old_pred))
    gp.set_inducing_points(z2)
    fresh = make_gp(case, z=z2)
    assert np.array_equal(gp.inducing_points, z2) and gp.bound == fresh.bound
    assert all(np.array_equal(a, b) for a, b in zip(gp(q), fresh(q)))
    clone = pickle.loads(pickle.dumps(gp))
    assert np.array_equal(clone.inducing_points, z2)
    assert clone.marginal_likelihood(full_theta(case)) == fresh.bound  # (the engine is rebuilt from the moved Z)
    # a fit that fails (eps = 0, two coincident inducing inputs, a = 1) puts the previous Z and fit back
    unit = dict(case, theta=case["theta"].copy())
    unit["theta"][0] = 0.0
    gp = make_gp(unit, jitter=0.0, z=z2)
    kept_bound, kept_pred = gp.bound, gp(q)
    z3 = z2.copy()
    z3[1] = z3[0]
    with pytest.raises(LinAlgError):
        gp.set_inducing_points(z3)
    assert np.array_equal(gp.inducing_points, z2) and gp.bound == kept_bound
    assert all(np.array_equal(a, b) for a, b in zip(gp(q), kept_pred))
    assert gp.marginal_likelihood(full_theta(unit)) == kept_bound


def test_an_indefinite_model_is_an_info_return():
    """eps = 0 with the first two inducing points coincident and a = 1: the second pivot of K_mm is exactly 0."""
    case = dict(reference(1)[0])
    case["z"] = case["z"].copy()
    case["z"][1] = case["z"][0]
    case["theta"] = case["theta"].copy()
    case["theta"][0] = 0.0
    gp = make_gp(case)  # (jitter 1e-8: a valid model)
    assert device_bound(gp, case, zgrad=False, jitter=0.0)[3] == 2
    assert device_bound(gp, case, jitter=0.0)[3] == 2
    gp.jitter = 0.0
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_gradient(full_theta(case), inducing_points=True)
    gp.jitter = 1e-8
    got = device_bound(gp, case)
    assert got[3] == 0
    base = mirror_zgrad(case)
    check("dF/dZ after the failed calls", got[4], base, zgrad_allowance(case, base, 7000))


def test_optimise_inducing_points_end_to_end():
    """SE + WhiteNoise, N = 2000, d = 1, m = 8, Z a seeded random subset, theta given; the joint search over [theta | Z].
    The exact log marginal likelihood is the bound at Z = x, eps = 0 in its dense form, where Q = K_nn K_nn^-1 K_nn = K_nn
    and the trace term is 0: ln N(r | 0, K_nn + Sigma), formed here without the solve by the singular K_nn."""
    from inference_amd.gp import SparseGpRegressor, SquaredExponential, WhiteNoise
    from scipy.linalg import cholesky, solve_triangular

    n, m = 2000, 8
    x, y, _ = sh.dataset(n, 1, seed=9)
    theta0 = np.array([MU, 0.0, np.log(0.25), np.log(0.2)])
    gp = SparseGpRegressor(x, y, inducing_points=m, kernel=SquaredExponential() + WhiteNoise(), hyperpars=theta0, seed=3)
    z0 = gp.inducing_points.copy()
    lo, hi = np.array(gp.hp_bounds).T
    assert (theta0 > lo).all() and (theta0 < hi).all()  # (the search starts where the model stands)
    assert gp.bound == gp.marginal_likelihood(theta0)
    F_before, F_after = gp.optimise_inducing_points()
    log = gp.inducing_log
    print(f"F {F_before:.6f} -> {F_after:.6f} in {log['evaluations']} evaluations, warnflag {log['warnflag']}")
    assert F_before == log["F_before"] and F_after == log["F_after"] == gp.bound
    assert F_after >= F_before
    z, th = gp.inducing_points, np.asarray(gp.hyperpars)
    assert z.shape == z0.shape and not np.array_equal(z, z0)
    assert (z >= x.min(axis=0)).all() and (z <= x.max(axis=0)).all()
    assert (th >= lo).all() and (th <= hi).all()

    white = float(np.exp(2.0 * th[3]))
    q = np.linspace(-0.1, 1.1, 23).reshape(-1, 1)

    def mirror_values(seed=None):
        mir = sh.SparseMirror("se", x, z, ripple=None if seed is None else sh.rippler(seed))
        st = mir.state(th[1:3], white, y - th[0], None)
        mean, var = mir.predict(th[1:3], white, y - th[0], None, q, st=st)
        return dict(F=np.array([st["F"]]), mean=mean + th[0], var=var)

    base = mirror_values()
    spread = {k: 0.0 for k in base}
    for i in range(N_RIPPLES):
        moved = mirror_values(8000 + i)
        for k in base:
            spread[k] = max(spread[k], float(np.abs(moved[k] - base[k]).max()))
    scale = dict(F=abs(base["F"][0]), mean=float(np.abs(base["mean"]).max()), var=float(np.exp(2.0 * th[1])))
    allow = {k: max(10.0 * spread[k], 1e-10 * scale[k]) for k in base}
    check("F at the optimum", gp.bound, base["F"][0], allow["F"])
    C = cholesky(mh.cross("se", x, x, th[1:3]) + white * np.eye(n), lower=True)
    v = solve_triangular(C, y - th[0], lower=True)
    exact = float(-0.5 * (n * sh.LN_2PI + 2.0 * np.log(np.diag(C)).sum() + v @ v))
    print(f"the exact log marginal likelihood at the final theta: {exact:.6f}")
    assert F_after <= exact + allow["F"]
    mean, std = gp(q)
    check("mean at the optimum", mean, base["mean"], allow["mean"])
    check("variance at the optimum", std**2, np.abs(base["var"]), allow["var"])
    # at the fixed hyper-parameters alone, from the start again
    gp.set_hyperparameters(theta0)
    gp.set_inducing_points(z0)
    Fb, Fa = gp.optimise_inducing_points(hyperpars=False, maxiter=30)
    print(f"Z alone: F {Fb:.6f} -> {Fa:.6f}")
    assert Fb == F_before and Fa >= Fb and np.array_equal(gp.hyperpars, theta0)
    # the constructor's keyword, with hyper-parameters given: the same search over Z alone
    gp = SparseGpRegressor(x, y, inducing_points=m, kernel=SquaredExponential() + WhiteNoise(), hyperpars=theta0, seed=3,
                           optimise_inducing=True)
    assert gp.inducing_log["F_before"] == F_before and gp.bound == gp.inducing_log["F_after"] >= Fa
    assert np.array_equal(gp.hyperpars, theta0) and not np.array_equal(gp.inducing_points, z0)
