"""
GPU tests of the exact Hessian of the log-marginal likelihood (gpmi_lml_hessian, `GpRegressor.marginal_likelihood_hessian`,
`laplace_approximation`) against the long-double NumPy mirror of tests/hessian_host.py on `workloads.synthetic_dataset`
(y_err = 0.1: a well-conditioned K).

Error of an entry: |device - mirror| over the mirror's |T1| + |T2| + |T3| of that entry.  Tolerance: 1e-10; an entry
beyond it is held to ten times the largest movement of the float64 mirror's own entry under 48 symmetric relative ripples
of 1e-13 on its K (computed without the device, and only when an entry needs it).  Every case prints both figures.

Shapes: the smallest at which each path can go wrong (the table in `CASES`).
"""
import ctypes as C

import numpy as np
import pytest
from numpy.linalg import LinAlgError

import hessian_host as hh
import workloads as wl

pytestmark = pytest.mark.gpu

TOL = 1e-10

# name -> (kind, N, d, white noise, linear mean, duplicated rows of x)
CASES = {
    "se_const_130x3": ("se", 130, 3, False, False, False),     # one row past a 128 tile, a ragged 64 tile in both contractions
    "se_wn_300x2": ("se", 300, 2, True, False, False),         # the ln sigma row and column, extra diagonal in the ln a terms
    "rq_257x17": ("rq", 257, 17, False, False, False),         # the 64 KiB-LDS builder path, the kappa row and column
    "m32_dup_200x2": ("m32", 200, 2, False, False, True),      # the t = 0 guard of g2
    "m52_linear_640x1": ("m52", 640, 1, False, True, False),   # a second 512 inverse block, n_mean = 2
    "se_70x64": ("se", 70, 64, False, False, False),           # d = 64 without shape or noise parameter: a pair table of 65
    # the length-scale block has 22 * 23 / 2 = 253 sums: the 256-sum LDS slab flushes inside RQ's kappa tail
    "rq_wn_134x22": ("rq", 134, 22, True, False, False),
    # PT = 67, the widest pair table: RQ's contraction with the > 64 KiB LDS opt-in, the kappa rows next to the ln sigma column
    "rq_wn_70x64": ("rq", 70, 64, True, False, False),
}


def kernel_of(kind, wn):
    from inference_amd.gp import Matern32, Matern52, RationalQuadratic, SquaredExponential, WhiteNoise

    k = {"se": SquaredExponential, "rq": RationalQuadratic, "m32": Matern32, "m52": Matern52}[kind]()
    return k + WhiteNoise() if wn else k


def case_inputs(name):
    kind, n, d, wn, linear, dup = CASES[name]
    x, y, e = wl.synthetic_dataset(1, n, d)
    if dup:
        x = x.copy()
        x[1::2] = x[0::2]
    scale = 0.5 * max(1.0, np.sqrt(d / 3.0))  # keeps u = sum_k q_k of order one in many dimensions
    mean = [float(y.mean())] + ([0.1] * d if linear else [])
    kern = [np.log(y.std())] + ([0.3] if kind == "rq" else []) + list(np.log(scale * np.linspace(0.8, 1.25, d)))
    theta = np.array(mean + kern + ([np.log(0.2)] if wn else []))
    return kind, x, y, e, theta, wn, linear


_built = {}


def build(name):
    """(regressor, theta, long-double mirror, mirror arguments) of a case, computed once and shared."""
    if name not in _built:
        from inference_amd.gp import ConstantMean, GpRegressor, LinearMean

        kind, x, y, e, theta, wn, linear = case_inputs(name)
        gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=kernel_of(kind, wn), mean=LinearMean if linear else ConstantMean)
        phi = np.array(gp.mean.mean_and_gradients(theta[gp.mean_slice])[1])
        n_mean = len(phi)
        args = (kind, x, y, e**2, theta[:n_mean], phi, theta[n_mean: len(theta) - (1 if wn else 0)], theta[-1] if wn else None)
        _built[name] = (gp, theta, hh.hessian(*args, dtype=np.longdouble), args)
    return _built[name]


def assert_parity(name, H, mirror, args):
    ref, scale = np.asarray(mirror["H"], dtype=float), np.asarray(mirror["scale"], dtype=float)
    diff = np.abs(H - ref)
    err = float((diff / scale).max())
    if err <= TOL:
        print(f"{name}: {err:.2e} of sum |terms| (tolerance {TOL:.0e})")
        return
    spread = hh.ripple_spread(*args)
    ok = (diff <= TOL * scale) | (diff <= 10.0 * spread)
    worst = float((diff / np.maximum(spread, 1e-300))[diff > TOL * scale].max())
    print(f"{name}: {err:.2e} of sum |terms| (beyond {TOL:.0e}); the entries beyond it are at most {worst:.2f} x the mirror's own "
          f"spread under 48 ripples of 1e-13 (allowance 10 x)")
    assert ok.all(), f"{name}: entries {np.argwhere(~ok).tolist()} beyond both allowances"


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_hessian_against_the_long_double_mirror(name):
    gp, theta, mirror, args = build(name)
    lml, grad, H = gp.marginal_likelihood_hessian(theta, method="exact")
    P = theta.size
    assert H.shape == (P, P) and grad.shape == (P,)
    assert np.array_equal(H, H.T), "the matrix is symmetric bit for bit"
    assert abs(lml - mirror["lml"]) <= 1e-10 * abs(mirror["lml"])
    g_ref = np.asarray(mirror["grad"], dtype=float)
    assert np.abs(grad - g_ref).max() <= 1e-10 * max(np.abs(g_ref).max(), 1.0)
    lml2, grad2 = gp.marginal_likelihood_gradient(theta)
    assert lml == lml2 and np.array_equal(grad[gp.cov_slice], grad2[gp.cov_slice]), "the gradient's own bits"
    assert np.isfinite(H).all()
    assert_parity(name, H, mirror, args)


def test_grouped_call_is_bit_equal(monkeypatch):
    """GPMI_HESS_GIB small enough for two parameters per group (N = 130: padded matrices of 256 x 288 doubles, three per
    parameter): five parameters in groups of 2, 2 and 1, the later groups' products formed again for every earlier one."""
    gp, theta, mirror, args = build("se_const_130x3")
    whole = gp.marginal_likelihood_hessian(theta, method="exact")
    per_matrix = 256 * 288 * 8
    monkeypatch.setenv("GPMI_HESS_GIB", repr(2.5 * 3 * per_matrix / 2.0**30))
    grouped = gp.marginal_likelihood_hessian(theta, method="exact")
    assert whole[0] == grouped[0] and np.array_equal(whole[1], grouped[1]) and np.array_equal(whole[2], grouped[2])
    monkeypatch.setenv("GPMI_HESS_GIB", repr(0.5 * 3 * per_matrix / 2.0**30))
    from inference_amd._lib import GpmiError

    with pytest.raises(GpmiError, match="GPMI_HESS_GIB"):
        gp.marginal_likelihood_hessian(theta, method="exact")
    monkeypatch.delenv("GPMI_HESS_GIB")
    again = gp.marginal_likelihood_hessian(theta, method="exact")
    assert np.array_equal(whole[2], again[2]), "a repeated call returns the same bits"


def test_repeated_call_and_fitted_state_are_bit_identical():
    gp, theta, _, _ = build("se_wn_300x2")
    pts = wl.query_points(1, 40, 2)
    before = (gp.hyperpars.copy(), np.array(gp.alpha), gp(pts))
    a = gp.marginal_likelihood_hessian(theta + 0.05, method="exact")
    b = gp.marginal_likelihood_hessian(theta + 0.05, method="exact")
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[2], a[2].T)
    after = (gp.hyperpars, np.array(gp.alpha), gp(pts))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])


def test_noise_row_is_zero_without_noise():
    """sigma^2 = 0 (ln sigma = -400): the last row, column and gradient entry are exact zeros, the rest is the model
    without the WhiteNoise term."""
    gp, theta, _, _ = build("se_wn_300x2")
    th = theta.copy()
    th[-1] = -400.0
    _, grad, H = gp.marginal_likelihood_hessian(th, method="exact")
    assert np.all(H[-1] == 0.0) and np.all(H[:, -1] == 0.0) and grad[-1] == 0.0
    assert np.isfinite(H).all() and np.abs(H[:-1, :-1]).max() > 0.0


def test_failed_factorisation_raises_and_leaves_the_handle_usable(golden):
    """The `fail` fixture's indefinite diagonal data covariance as the regressor's data variances (the recipe of
    tests/test_predict_batch_gpu.py): theta_bad has a negative pivot, theta_ok factorises."""
    from inference_amd import gp as gp_mod

    g = golden("fail")
    assert not (g["y_cov"] - np.diag(np.diagonal(g["y_cov"]))).any()
    gp = gp_mod.GpRegressor(g["x"], g["y"], y_err=np.full(len(g["y"]), 0.1), hyperpars=g["theta_ok"])
    gp.engine.h.close()
    gp._engine = None
    gp._noise_var = np.diagonal(g["y_cov"]).copy()
    gp.set_hyperparameters(g["theta_ok"])
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_hessian(g["theta_bad"], method="exact")
    lml, grad, H = gp.marginal_likelihood_hessian(g["theta_ok"], method="exact")
    assert np.isfinite(H).all() and np.array_equal(H, H.T), "the handle that refused a matrix evaluates the next one"
    assert lml == gp.marginal_likelihood_gradient(g["theta_ok"])[0]
    gp.engine.close()


def test_fd_agrees_with_exact():
    """method="fd" (second-order central differences of the device gradient, h = 1e-4 max(1, |theta_i|)) against
    "exact".  Allowance, measured as in tests/test_hessian_cpu.py: ten times what the same scheme at the same steps leaves
    between the device's LML and its own gradient, both sides over their largest magnitude."""
    gp, theta, mirror, _ = build("se_const_130x3")
    lml, grad, H = gp.marginal_likelihood_hessian(theta, method="exact")
    _, grad_fd, H_fd = gp.marginal_likelihood_hessian(theta, method="fd")
    assert np.array_equal(H_fd, H_fd.T) and np.array_equal(grad_fd, gp.marginal_likelihood_gradient(theta)[1])
    fd_g = np.empty(theta.size)
    for i in range(theta.size):
        h = gp.FD_HESSIAN_STEP * max(1.0, abs(theta[i]))
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd_g[i] = (gp.marginal_likelihood(tp) - gp.marginal_likelihood(tm)) / (tp[i] - tm[i])
    ref_err = float(np.abs(fd_g - grad).max() / np.abs(grad).max())
    scale = np.asarray(mirror["scale"], dtype=float)
    err = float(np.abs(H_fd - H).max() / scale.max())
    print(f"fd vs exact: {err:.2e} of the largest sum |terms|; the scheme on the device's own LML / gradient {ref_err:.2e}")
    assert err <= 10.0 * ref_err


def test_models_without_an_exact_path():
    from inference_amd.gp import GpRegressor, RationalQuadratic, SquaredExponential

    x, y, e = wl.synthetic_dataset(1, 60, 2)
    kernel = SquaredExponential() + RationalQuadratic()
    theta = np.array([y.mean(), np.log(y.std()) - 0.3, np.log(0.5), np.log(0.6), np.log(y.std()) - 0.5, 0.2, np.log(0.9), np.log(0.8)])
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=kernel)
    with pytest.raises(NotImplementedError, match="fd"):
        gp.marginal_likelihood_hessian(theta, method="exact")
    lml, grad, H = gp.marginal_likelihood_hessian(theta, method="auto")
    assert H.shape == (8, 8) and np.isfinite(H).all() and np.array_equal(H, H.T)
    gp.engine.close()


def test_laplace_approximation():
    from inference_amd.gp import GpRegressor, SquaredExponential

    x, y, e = wl.synthetic_dataset(1, 130, 2)
    np.random.seed(5)
    gp = GpRegressor(x, y, y_err=e, kernel=SquaredExponential, n_starts=4)  # theta from the constructor's search
    lap = gp.laplace_approximation()
    P = gp.n_hyperpars
    assert np.array_equal(lap.mean, gp.hyperpars) and lap.hessian.shape == (P, P) and lap.std.shape == (P,)
    assert np.abs(lap.covariance @ (-lap.hessian) - np.eye(P)).max() <= 1e-8
    assert np.array_equal(lap.sample(5, seed=3), lap.sample(5, seed=3)) and lap.sample(5, seed=3).shape == (5, P)
    sign, logdet = np.linalg.slogdet(-lap.hessian)
    want = lap.lml - 0.5 * 130 * np.log(2 * np.pi) + 0.5 * P * np.log(2 * np.pi) - 0.5 * logdet
    assert sign > 0 and abs(lap.log_evidence - want) <= 1e-9 * abs(want)
    mean, var = gp.predict_marginalised(wl.query_points(1, 10, 2), lap.sample(8, seed=1))[:2]
    assert np.isfinite(mean).all()
    # far from a maximum -H is not positive definite: the message names the eigenvalue and a parameter
    with pytest.raises(LinAlgError, match="smallest eigenvalue"):
        gp.laplace_approximation(gp.hyperpars + np.r_[0.0, 3.0, -2.0, 2.0])
    gp.engine.close()


def test_the_handle_gives_its_memory_back():
    from inference_amd import _lib
    from inference_amd.gp import GpRegressor, SquaredExponential

    def live():
        out = (C.c_int64 * 2)()
        assert _lib.load().gpmi_live_bytes(out) == 0
        return out[0], out[1]

    x, y, e = wl.synthetic_dataset(1, 130, 3)
    theta = wl.timing_theta(wl.SE, y, 3)
    start = live()
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential)
    held0 = live()
    gp.marginal_likelihood_hessian(theta, method="exact")
    assert live()[0] >= held0[0] + 2 * 4 * 256 * 288 * 8, "D_i and G_i of the four parameters are the handle's device memory"
    gp.engine.close()
    assert live() == start
