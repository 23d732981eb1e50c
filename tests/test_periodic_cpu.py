"""
CPU tests of the Periodic kernel: the NumPy mirror's derivatives (tests/periodic_host.py) against fourth-order
differences, the host accuracy check of kmath::sinpi_sq (tools/kmath_periodic_check.cpp), the class's argument checks,
labels, bounds and pickling, its routing onto the device entry points (`device_plan`), and the refusals of the regressors
that do not take it.  No GPU: every argument check here runs before a device is touched.
"""
import os
import pickle
import subprocess

import numpy as np
import pytest

import periodic_host as ph

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CASES = [(1, [0]), (3, [1]), (3, [0, 2]), (3, [0, 1, 2])]


def _d4(f, h):
    """fourth-order central difference of f at 0 with step h"""
    return (f(-2 * h) - 8 * f(-h) + 8 * f(h) - f(2 * h)) / (12 * h)


@pytest.mark.parametrize("d,dims", CASES)
def test_mirror_parameter_derivatives_against_fourth_order_differences(d, dims):
    """dK/dtheta_j of the mirror against fourth-order differences of its K in long double, step 1e-4: truncation
    ~ h^4 K^(5) / 30 with K^(5) ~ (2 pi u)^5 ~ 1e8 for ln p at the 7 periods the data span, so ~ 1e-9 of that derivative's
    own size ~ 2 pi u; rounding ~ 1e-19 / 1e-4 - tolerance 1e-9 of the largest element."""
    x, _, _ = ph.dataset(20, d)
    theta = ph.theta_for(d, dims)
    _, grads = ph.build_and_grads(x, theta, dims)
    assert len(grads) == theta.size == 1 + d + len(dims)
    for j, G in enumerate(grads):
        e = np.zeros(theta.size)
        e[j] = 1.0
        fd = _d4(lambda t: ph.cross(x, x, theta + t * e, dims, np.longdouble), 1e-4)
        G0 = G - (2.0 * ph.JITTER * np.exp(2 * theta[0]) * np.eye(len(x)) if j == 0 else 0.0)
        err = float(np.abs(G0 - fd).max() / np.abs(fd).max())
        print(f"d={d} dims={dims} dK/dtheta_{j}: {err:.2e}")
        assert err <= 1e-9, (d, dims, j, err)


@pytest.mark.parametrize("d,dims", CASES)
def test_mirror_point_derivatives_against_fourth_order_differences(d, dims):
    """A_kn K(q, x_n) = dK(q, x_n)/dq_k against fourth-order differences in q (long double, step 1e-4), tolerance 1e-9;
    R against the second derivative's closed form; the class's gradient_terms equal the mirror's."""
    from inference_amd.gp import Periodic

    x, _, _ = ph.dataset(20, d)
    theta = ph.theta_for(d, dims)
    cov = Periodic(periodic_dims=dims)
    cov.pass_spatial_data(x)
    rng = np.random.default_rng(5)
    for q in rng.uniform(0.0, ph.SPAN, size=(3, d)):
        A, R = ph.gradient_terms(q, x, theta, dims)
        assert A.shape == (d, len(x)) and R.shape == (d,)
        k = ph.cross(q[None, :], x, theta, dims)[0]
        for i in range(d):
            e = np.zeros(d)
            e[i] = 1.0
            fd = _d4(lambda t: ph.cross((q + t * e)[None, :], x, theta, dims, np.longdouble)[0], 1e-4)
            err = float(np.abs(A[i] * k - fd).max() / np.abs(fd).max())
            assert err <= 1e-9, (d, dims, i, err)
        a2, l, p = ph.split(theta, d, dims)
        want = np.array([a2 / l[i] ** 2 * ((2 * np.pi / p[i]) ** 2 if i in dims else 1.0) for i in range(d)])
        assert np.allclose(R, want, rtol=1e-14, atol=0)
        Ac, Rc = cov.gradient_terms(q, x, theta)
        # (the two form the sine's argument in another order: 2^-53 x the 44 radians of 7 periods, absolute)
        assert np.abs(Ac - A).max() <= 1e-13 * np.abs(A).max() and np.allclose(Rc, R, rtol=1e-14, atol=0)


def test_sinpi_sq_accuracy_on_the_host(tmp_path):
    """tools/kmath_periodic_check.cpp: sin^2(pi r) against long double at 1e7 uniform and 1e6 log-uniform r, the ties,
    r = 0 and whole periods added; non-zero exit beyond 4 x 2^-53 relative."""
    exe = str(tmp_path / "kmath_periodic_check")
    src = os.path.join(ROOT, "tools", "kmath_periodic_check.cpp")
    inc = os.path.join(ROOT, "inference-tools_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-I", inc, src, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


def test_header_constants():
    import re

    from inference_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"#define\s+GPMI_KERNEL_PER\s+5\b", header) and _lib.KERNEL_PER == 5
    assert re.search(r"#define\s+GPMI_MAX_PERIODIC\s+8\b", header) and _lib.MAX_PERIODIC == 8
    assert re.search(r"int\s+gpmi_set_periodic\(gpmi_ctx\*\s*\w*,\s*int\s+n_per,\s*const\s+int\*\s*dims\)", header)


def test_argument_checks():
    from inference_amd.gp import Periodic

    x, _, _ = ph.dataset(20, 3)
    with pytest.raises(ValueError, match="empty"):
        Periodic(periodic_dims=[])
    with pytest.raises(ValueError, match="distinct"):
        Periodic(periodic_dims=[1, 1])
    with pytest.raises(ValueError, match="distinct"):
        Periodic(periodic_dims=[-1])
    with pytest.raises(ValueError, match="integers"):
        Periodic(periodic_dims=[0.5])
    with pytest.raises(ValueError, match="periodic dimension 3"):
        Periodic(periodic_dims=[0, 3]).pass_spatial_data(x)
    wide = np.random.default_rng(0).uniform(size=(12, 9))
    with pytest.raises(ValueError, match="at most 8"):
        Periodic().pass_spatial_data(wide)  # None: all 9
    with pytest.raises(ValueError, match="at most 8"):
        Periodic(periodic_dims=list(range(9))).pass_spatial_data(wide)
    cov = Periodic(periodic_dims=[8, 0])  # 2 of 9, stored sorted
    cov.pass_spatial_data(wide)
    assert cov.periodic_dims == [0, 8] and cov.n_params == 1 + 9 + 2


def test_labels_bounds_and_pickle():
    from inference_amd import _lib
    from inference_amd.gp import Periodic, SquaredExponential
    from inference_amd.gp.covariance import _pairwise_abs_mean_and_range

    x, y, _ = ph.dataset(65, 3)
    cov = Periodic(periodic_dims=[2, 0])
    assert cov._gpmi_kernel == _lib.KERNEL_PER
    cov.pass_spatial_data(x)
    assert cov.periodic_dims == [0, 2] and cov.n_params == 6
    assert cov.hyperpar_labels == ["Periodic log-amplitude", "Periodic log-scale 0", "Periodic log-scale 1",
                                   "Periodic log-scale 2", "Periodic log-period 0", "Periodic log-period 2"]
    cov.estimate_hyperpar_bounds(y)
    se = SquaredExponential()
    se.pass_spatial_data(x)
    se.estimate_hyperpar_bounds(y)
    assert cov.bounds[0] == se.bounds[0] and cov.bounds[2] == se.bounds[2]  # amplitude and the plain dimension: as SE
    assert cov.bounds[1] == cov.bounds[3] == (-2.3, 2.3)
    for b, k in zip(cov.bounds[4:], [0, 2]):
        mean_abs, rng = _pairwise_abs_mean_and_range(x[:, k])
        assert b == (np.log(mean_abs) - 3, np.log(rng) + 1)
    allp = Periodic()
    allp.pass_spatial_data(x)
    assert allp.periodic_dims == [0, 1, 2] and allp.n_params == 7
    given = [(-1.0, 1.0)] * 6
    assert Periodic(periodic_dims=[0, 2], hyperpar_bounds=given).bounds == given
    back = pickle.loads(pickle.dumps(cov))
    assert type(back) is Periodic and back.bounds == cov.bounds and back.n_params == 6 and back.periodic_dims == [0, 2]
    assert back.hyperpar_labels == cov.hyperpar_labels and np.array_equal(back.x, cov.x) and back._engine is None


def test_device_plan():
    from inference_amd import _lib
    from inference_amd.gp import (ChangePoint, HeteroscedasticNoise, Matern52, Periodic, RationalQuadratic,
                                  SquaredExponential, WhiteNoise)
    from inference_amd.gp.covariance import device_plan, heteroscedastic_slice, periodic_dims_of, sum_kernels

    x, _, _ = ph.dataset(65, 2)
    cov = Periodic(periodic_dims=[1])
    cov.pass_spatial_data(x)
    assert device_plan(cov) == (_lib.KERNEL_PER, cov, slice(0, 4), None) and periodic_dims_of(cov) == [1]
    cov = Periodic(periodic_dims=[1]) + WhiteNoise()
    cov.pass_spatial_data(x)
    plan = device_plan(cov)
    assert plan[0] == _lib.KERNEL_PER and plan[1] is cov.components[0] and plan[2] == slice(0, 4) and plan[3] == 4
    cov = Periodic() + HeteroscedasticNoise() + WhiteNoise()
    cov.pass_spatial_data(x)
    plan = device_plan(cov)
    assert plan[0] == _lib.KERNEL_PER and plan[2] == slice(0, 5) and heteroscedastic_slice(cov) == slice(5, 5 + 65)
    assert plan[3] == 5 + 65 and periodic_dims_of(cov) == [0, 1]
    cov = SquaredExponential() + Periodic(periodic_dims=[0]) + WhiteNoise()
    cov.pass_spatial_data(x)
    plan = device_plan(cov)
    assert plan[0] == _lib.KERNEL_SUM and list(plan[2]) == list(range(3 + 4)) and plan[3] == 7
    assert sum_kernels(cov) == [_lib.KERNEL_SE, _lib.KERNEL_PER] and periodic_dims_of(cov) == [0]
    cov = Periodic(periodic_dims=[0]) + Periodic(periodic_dims=[0])
    cov.pass_spatial_data(x)
    assert device_plan(cov)[0] == _lib.KERNEL_SUM and sum_kernels(cov) == [_lib.KERNEL_PER] * 2
    cov = Matern52() + Periodic(periodic_dims=[1]) + RationalQuadratic() + SquaredExponential()
    cov.pass_spatial_data(x)
    assert device_plan(cov)[0] == _lib.KERNEL_SUM and len(sum_kernels(cov)) == 4
    # components that disagree on the periodic dimensions, and a ChangePoint holding a Periodic: the generic route
    cov = Periodic(periodic_dims=[0]) + Periodic(periodic_dims=[1])
    cov.pass_spatial_data(x)
    assert device_plan(cov) is None
    cov = ChangePoint([Periodic(periodic_dims=[0]), SquaredExponential()])
    cov.pass_spatial_data(x)
    assert device_plan(cov) is None
    cov = ChangePoint([Periodic(periodic_dims=[0]), SquaredExponential()]) + WhiteNoise()
    cov.pass_spatial_data(x)
    assert device_plan(cov) is None
    # SE sums and mixtures keep their plans
    cov = ChangePoint([Matern52(), SquaredExponential()])
    cov.pass_spatial_data(x)
    assert device_plan(cov)[0] == -1 and periodic_dims_of(cov) is None


def test_other_regressors_refuse_the_kernel_before_any_device_call():
    from inference_amd.gp import (GeneralisedGpRegressor, MultiTargetGpRegressor, Periodic, SparseGpRegressor, WhiteNoise,
                                  select_inducing_points)

    x, y, e = ph.dataset(40, 2)
    with pytest.raises(NotImplementedError, match="Periodic"):
        SparseGpRegressor(x, y, y_err=e, kernel=Periodic(periodic_dims=[0]), inducing_points=8)
    with pytest.raises(NotImplementedError, match="Periodic"):
        SparseGpRegressor(x, y, y_err=e, kernel=Periodic() + WhiteNoise(), inducing_points=8, inducing_method="greedy")
    with pytest.raises(NotImplementedError, match="Periodic"):
        select_inducing_points(x, 8, Periodic(periodic_dims=[0]), ph.theta_for(2, [0]))
    with pytest.raises(NotImplementedError, match="Periodic"):
        MultiTargetGpRegressor(x, np.stack([y, 2 * y], axis=1), y_err=e, kernel=Periodic(periodic_dims=[1]))
    with pytest.raises(NotImplementedError, match="Periodic"):
        GeneralisedGpRegressor(x, (y > 0).astype(float), kernel=Periodic())


def test_exact_hessian_is_refused_for_the_kernel():
    """`_exact_hessian_ok` is a property of the model alone: "exact" raises before a device call ("auto" takes "fd")."""
    from inference_amd.gp import GpRegressor, Periodic

    x, y, e = ph.dataset(20, 1)
    gp = GpRegressor.__new__(GpRegressor)  # the check reads the plan only: no device handle
    cov = Periodic()
    cov.pass_spatial_data(x)
    from inference_amd.gp.covariance import device_plan

    gp._generic, gp._mix, gp._het_slice, gp._y_cov = False, None, None, None
    gp._kernel_id = device_plan(cov)[0]
    assert gp._exact_hessian_ok() is False
