"""
The entry points that were added after the flag-ordered tail, on a lane that HAS the CU-masked stream pair: gpmi_ggp_*
(GeneralisedGpRegressor), gpmi_lml_hessian, gpmi_mt_* (MultiTargetGpRegressor), the M x M factorisation of the joint
draws (draws_tail) and the m x m one of the linear inverter (linv_factor).  Their own test files stop at N = 640, where a
handle has no pair and every factorisation runs in stream order on the full chip.  Here N = 5130: np = 5248 >= 5120, lane 0
owns the pair, lane 1 borrows it, and a factorisation of the N x N matrix is ONE flag-ordered launch of 41 tile rows
(csrc/potrf_flow.hip); the draws' Sigma (M = 1100) and the inverter's data-space matrix (m = 1100) are 9-row launches on
the borrowed pair, whose cached task lists then have another size than the fit's.

Every family follows one pattern on one handle (`three_schedules`): compute under the default schedule with the
in-kernel stamps on and require the witness; compute again under GPMI_OPT_NO_FLOW = 1 (the stream-ordered twin on the same
handle: no flag-ordered launch may be booked); switch back to 0 and compute a third time.  All three results must be the
SAME BITS: the schedules reorder execution, never a summation, so bit equality with the stream-ordered schedule is the
sharpest check there is - and the stream-ordered values themselves are pinned by the small-N mirrors of each family, by
the large-N parity tests and by part H of tests/test_kernels_gpu.py.  The generalised GP is anchored in addition to a
NumPy mirror run at this very size (tests/golden/generalised_pair.npz).

The witness: GPMI_PROF_FLOW launches > 0 (one per flag-ordered launch, booked by potrf_flow_tail), with exactly the
FLOPs of launches of the expected number of tile rows (kernel_host.flow_update_flops); RuntimeWarning is an error and the
handle's `_no_flow` must still be unset - a call that timed out and was silently repeated in stream order fails the
test.  Each regressor is closed before the next family opens one: two handles that own a pair are never alive together.
"""
import numpy as np
import pytest

import generalised_host as gh
import kernel_host as kh
import workloads as wl
from inference_amd import _lib
from inference_amd.gp import (GeneralisedGpRegressor, GpLinearInverter, GpRegressor, MultiTargetGpRegressor, Poisson,
                              SquaredExponential)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::RuntimeWarning")]

N, D = 5130, 2
FIT_ROWS = -(-N // 128)  # 41 tile rows: np = 5248
SMALL = 1100             # M of the draws, m of the inverter: 9 tile rows


def _stamps(h, on):
    h.call("gpmi_profile_enable", (2 << _lib.PROF_SYRK) if on else 0)
    h.call("gpmi_profile_reset")


def _flow_booked(h):
    """(launches, FLOPs) under GPMI_PROF_FLOW since the last reset; resets"""
    import ctypes as C

    launches, flops = C.c_int64(-1), C.c_double(-1.0)
    h.call("gpmi_profile_read", _lib.PROF_FLOW, C.byref(launches), None, C.byref(flops), None)
    h.call("gpmi_profile_reset")
    return launches.value, flops.value


def _witness(h, what, rows, expect_flow=True):
    """Prints what the last computation booked and holds it to launches of `rows` tile rows (a tuple: any mix of them)."""
    launches, flops = _flow_booked(h)
    rows = (rows,) if isinstance(rows, int) else tuple(rows)
    print(f"\nFLOW-WITNESS {what}: FLOW launches {launches}, FLOPs {flops:.6e}; a launch of {rows} tile rows books "
          f"{[kh.flow_update_flops(r) for r in rows]}")
    assert not getattr(h, "_no_flow", False), f"{what}: the handle has fallen back to the stream-ordered schedule"
    if not expect_flow:
        assert launches == 0, f"{what}: {launches} flag-ordered launches under GPMI_OPT_NO_FLOW"
        return launches
    assert launches > 0, f"{what}: no flag-ordered launch - the computation ran in stream order"
    if len(rows) == 1:
        assert flops == launches * kh.flow_update_flops(rows[0]), \
            f"{what}: {launches} launches booked {flops!r} FLOPs, not {launches} x {kh.flow_update_flops(rows[0])!r}"
    return launches


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), \
            f"{what}: {key} differs in {int((x != y).sum()) if x.shape == y.shape else 'shape'} entries"


def three_schedules(h, compute, what, rows):
    """compute() -> dict of results, run under the default schedule (witnessed), under GPMI_OPT_NO_FLOW = 1 and under the
    default schedule again: the same bits three times.  Returns the first result."""
    _stamps(h, True)
    try:
        first = compute()
        _witness(h, f"{what}, default schedule", rows)
        h.call("gpmi_set_option", _lib.OPT_NO_FLOW, 1)
        try:
            stream = compute()
            _witness(h, f"{what}, GPMI_OPT_NO_FLOW", rows, expect_flow=False)
        finally:
            h.call("gpmi_set_option", _lib.OPT_NO_FLOW, 0)
        again = compute()
        _witness(h, f"{what}, default schedule again", rows)
    finally:
        _stamps(h, False)
    _same_bits(first, stream, f"{what}: flag-ordered against stream-ordered")
    _same_bits(first, again, f"{what}: flag-ordered again")
    return first


@pytest.fixture(scope="module")
def data():
    """(x, y, y_err, theta = [mean, ln a, ln l_1, ln l_2]) of the Gaussian families"""
    x, y, e = wl.synthetic_dataset(7, N, D)
    return x, y, e, wl.timing_theta(wl.SE, y, D)


# ------------------------------------------------------------------------------------------------ GeneralisedGpRegressor
def test_generalised_regressor(golden):
    """Poisson, SE, d = 2 (generalised_host.PAIR_CASES): one factorisation of B per Newton step, each a 41-row flag-ordered
    launch behind gpmi_ggp_*'s own potrf_pair_quiesce and L.early reset; marginal_likelihood and its gradient at theta2
    run on lane 1, which borrows lane 0's pair, and must leave the fit's bits alone.  Against the mirror at this size:
    logq, mode, alpha, mean and variance within the fixture's allowances (the ripple recipe of make_golden_generalised.py),
    Newton steps and halvings exactly.  An overflowing amplitude (theta[0] = 400: B is not finite inside the task kernel)
    returns -1e50 with exactly one warning, and the handle then returns its earlier bits."""
    name = "poisson_se_pair"
    c, g = gh.make_case(name), golden("generalised_pair")
    theta, theta2, pts = c["theta"], c["theta2"], c["pts"]
    gp = GeneralisedGpRegressor(c["x"], c["y"], likelihood=Poisson(c["aux_arg"]), kernel=SquaredExponential(), hyperpars=theta)
    eng = gp.engine
    try:
        assert gp.offset == float(g[f"{name}_offset"])

        def compute():
            gp.set_hyperparameters(theta)
            log = gp.newton_log
            mu, sig = gp(pts)
            out = dict(logq=gp._logq, mode=gp.mode, alpha=gp.alpha, counts=np.array([log["iterations"], log["halvings"]]),
                       mu=mu, sig=sig)
            out["lml2"] = gp.marginal_likelihood(theta2)
            out["lml2_g"], out["grad2"] = gp.marginal_likelihood_gradient(theta2)
            # the fit after the lane-1 evaluations: downloaded again, predicted again
            f1, g1 = eng.ggp_mode()
            mu1, sig1 = gp(pts)
            for key, val in (("mode", f1), ("alpha", g1), ("mu", mu1), ("sig", sig1)):
                assert np.array_equal(out[key], val), f"{key} of the fit changed under evaluations at theta2"
            return out

        res = three_schedules(eng.h, compute, "GeneralisedGpRegressor", FIT_ROWS)
        assert res["lml2"] == res["lml2_g"]
        assert tuple(res["counts"]) == tuple(g[f"{name}_newton"]), (res["counts"], g[f"{name}_newton"])
        for what, got in (("logq", res["logq"]), ("f", res["mode"]), ("g", res["alpha"]), ("mean", res["mu"]),
                          ("var", res["sig"] ** 2)):
            err, allow = float(np.abs(np.asarray(got) - g[f"{name}_{what}"]).max()), float(g[f"{name}_allow_{what}"])
            print(f"{name} {what:5s} error {err:9.2e}  allowance {allow:9.2e}")
            assert err <= allow, (what, err, allow)
        # a^2 overflows: one warning, -1e50, and nothing of it stays on the handle
        big = theta.copy()
        big[0] = 400.0
        with pytest.warns(RuntimeWarning) as rec:
            assert gp.marginal_likelihood(big) == -1e50
        assert len(rec) == 1
        assert not getattr(eng.h, "_no_flow", False)
        assert gp.marginal_likelihood(theta2) == res["lml2"]
        mu, sig = gp(pts)
        assert np.array_equal(mu, res["mu"]) and np.array_equal(sig, res["sig"])
        gp.set_hyperparameters(theta)
        assert gp._logq == res["logq"] and np.array_equal(gp.mode, res["mode"])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ the exact Hessian
def test_exact_hessian(data):
    """GpRegressor.marginal_likelihood_hessian(theta, "exact"), SE with a constant mean: lml, gradient and H the same bits
    in the three runs, H bit-symmetric."""
    x, y, e, theta = data
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    try:
        def compute():
            lml, grad, H = gp.marginal_likelihood_hessian(theta, "exact")
            assert np.array_equal(H, H.T), "the Hessian is not bit-symmetric"
            return dict(lml=lml, grad=grad, H=H)

        res = three_schedules(gp.engine.h, compute, "marginal_likelihood_hessian", FIT_ROWS)
        assert np.isfinite(res["H"]).all() and res["H"].shape == (4, 4)
    finally:
        gp.engine.close()


# ------------------------------------------------------------------------------------------------ MultiTargetGpRegressor
def test_multi_target_regressor(data):
    """T = 3 targets on one factorisation: the fit's alpha, the per-target LML, the gradient and the leave-one-out
    likelihood (the last three at shifted hyper-parameters: lane 1 on the borrowed pair)."""
    x, y, e, theta = data
    rng = np.random.default_rng(31)
    Y = np.stack([y, 0.5 * y + np.sin(4.0 * x[:, 0]), np.cos(3.0 * x[:, 1]) + 0.1 * rng.standard_normal(N)], axis=1)
    theta_cov = theta[1:].copy()
    theta2 = theta_cov + 0.1
    gp = MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=theta_cov, kernel=SquaredExponential)
    try:
        def compute():
            gp.set_hyperparameters(theta_cov)
            out = dict(alpha=gp.alpha, lml_fit=gp._lml, lml_fit_t=gp._lml_t)
            out["lml_t"] = gp.marginal_likelihood(theta2, per_target=True)
            out["lml"], out["grad"] = gp.marginal_likelihood_gradient(theta2)
            out["loo"] = gp.loo_likelihood(theta2)
            return out

        res = three_schedules(gp.engine.h, compute, "MultiTargetGpRegressor", FIT_ROWS)
        assert res["alpha"].shape == (N, 3) and res["lml_t"].shape == (3,)
        assert np.isfinite(res["alpha"]).all() and np.isfinite(res["grad"]).all() and np.isfinite(res["loo"])
    finally:
        gp.engine.close()


# ---------------------------------------------------------------------------------------------------------- joint draws
def test_posterior_draws_and_the_refit_after_them(data):
    """sample_posterior at M = 1100 points with the caller's normals: Sigma + eps I is factored as a 9-row flag-ordered
    launch on the borrowed pair, which rebuilds the lane's cached task lists for 9 rows; the refit that follows is a
    41-row launch again and must give the alpha of the first fit.  (Points in [0.9, 1.9]^2, mostly outside the data, with
    jitter 1e-6: max diag Sigma is then the prior variance and Sigma + eps I is safely positive definite.)"""
    x, y, e, theta = data
    theta = theta.copy()
    theta[2:] = np.log(0.1)
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    h = gp.engine.h
    rng = np.random.default_rng(32)
    pts = 0.9 + rng.uniform(0.0, 1.0, (SMALL, D))
    z = rng.standard_normal((4, SMALL))
    try:
        alpha0 = gp.alpha.copy()

        def compute():
            out = dict(draws=gp.sample_posterior(pts, 4, z=z, jitter=1e-6))
            out["booked_by_draws"] = np.array(_flow_booked(h))
            gp.set_hyperparameters(theta)
            out["alpha"] = gp.alpha.copy()
            return out

        _stamps(h, True)
        try:
            first = compute()
            _witness(h, "refit after the draws, default schedule", FIT_ROWS)
            h.call("gpmi_set_option", _lib.OPT_NO_FLOW, 1)
            try:
                stream = compute()
                _witness(h, "refit after the draws, GPMI_OPT_NO_FLOW", FIT_ROWS, expect_flow=False)
            finally:
                h.call("gpmi_set_option", _lib.OPT_NO_FLOW, 0)
            again = compute()
            _witness(h, "refit after the draws, default schedule again", FIT_ROWS)
        finally:
            _stamps(h, False)
        print(f"\nFLOW-WITNESS draws at M = {SMALL}: (launches, FLOPs) default {first['booked_by_draws']}, NO_FLOW "
              f"{stream['booked_by_draws']}, default again {again['booked_by_draws']}; a 9-row launch books "
              f"{kh.flow_update_flops(9)}")
        for r in (first, again):
            assert tuple(r["booked_by_draws"]) == (1.0, kh.flow_update_flops(-(-SMALL // 128)))
        assert tuple(stream["booked_by_draws"]) == (0.0, 0.0)
        for r, what in ((stream, "stream-ordered"), (again, "flag-ordered again")):
            assert first["draws"].tobytes() == r["draws"].tobytes(), f"draws: flag-ordered against {what}"
            assert first["alpha"].tobytes() == r["alpha"].tobytes(), f"alpha of the refit: flag-ordered against {what}"
        assert first["draws"].shape == (4, SMALL) and np.isfinite(first["draws"]).all()
        assert first["alpha"].tobytes() == alpha0.tobytes(), "the refit after the draws does not give the first fit's alpha"
    finally:
        gp.engine.close()


# ------------------------------------------------------------------------------------------------------ linear inversion
def test_linear_inverter():
    """5130 parameter positions (the handle owns the pair), m = 1100 observations: the data-space matrix A K A^T + S is
    factored as a 9-row flag-ordered launch.  marginal_likelihood, its gradient and the posterior mean."""
    rng = np.random.default_rng(33)
    pos = rng.uniform(0.0, 1.0, (N, D))
    centres = rng.uniform(0.0, 1.0, (SMALL, D))
    A = np.exp(-0.5 * ((centres[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2) / 0.1 ** 2)
    A /= A.sum(axis=1, keepdims=True)
    truth = np.sin(3.0 * pos[:, 0]) + np.cos(2.0 * pos[:, 1])
    y_err = np.full(SMALL, 0.05)
    y = A @ truth + y_err * rng.standard_normal(SMALL)
    theta = np.array([0.3, 0.0, np.log(0.3), np.log(0.3)])
    inv = GpLinearInverter(y, y_err, A, pos, SquaredExponential, device=None)
    try:
        def compute():
            out = dict(lml=inv.marginal_likelihood(theta))
            out["lml_g"], out["grad"] = inv.marginal_likelihood_gradient(theta)
            out["mean"] = inv.calculate_posterior_mean(theta)
            return out

        res = three_schedules(inv.engine.h, compute, "GpLinearInverter", -(-SMALL // 128))
        assert res["lml"] == res["lml_g"] and np.isfinite(res["grad"]).all() and res["mean"].shape == (N,)
        # a sanity anchor, far from sharp: the posterior mean reproduces the data within a few standard errors
        assert np.abs(A @ res["mean"] - y).max() <= 8.0 * 0.05
    finally:
        inv.engine.h.close()
