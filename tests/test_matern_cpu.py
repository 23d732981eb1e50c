"""
CPU tests of the Matern32 / Matern52 kernels: the classes and their routing onto the device entry points, pickling,
`gradient_terms` against central differences of the oracle kernel (tests/matern_host.py), and the host accuracy check of
kmath::matern_profile (tools/kmath_matern_check.cpp).  No GPU.
"""
import os
import pickle
import subprocess

import numpy as np
import pytest

import matern_host as mh

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

KINDS = {"m32": "Matern32", "m52": "Matern52"}


def _cls(kind):
    import inference_amd.gp as gp

    return getattr(gp, KINDS[kind])


@pytest.mark.parametrize("kind", list(KINDS))
def test_classes_labels_and_bounds(kind):
    from inference_amd import _lib
    from inference_amd.gp import SquaredExponential
    from inference_amd.gp.covariance import _StationaryDeviceKernel

    x, y, _ = mh.dataset(65, 3, far=False)
    cov = _cls(kind)()
    assert isinstance(cov, _StationaryDeviceKernel) and cov._n_shape_params == 0
    assert cov._gpmi_kernel == {"m32": _lib.KERNEL_M32, "m52": _lib.KERNEL_M52}[kind] == {"m32": 3, "m52": 4}[kind]
    cov.pass_spatial_data(x)
    assert cov.n_params == 4
    name = KINDS[kind]
    assert cov.hyperpar_labels == [f"{name} log-amplitude"] + [f"{name} log-scale {i}" for i in range(3)]
    cov.estimate_hyperpar_bounds(y)
    se = SquaredExponential()
    se.pass_spatial_data(x)
    se.estimate_hyperpar_bounds(y)
    assert cov.bounds == se.bounds  # bounds as for SquaredExponential
    given = [(-1.0, 1.0)] * 4
    assert _cls(kind)(hyperpar_bounds=given).bounds == given


def test_header_constants():
    import re

    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"#define\s+GPMI_KERNEL_M32\s+3\b", header)
    assert re.search(r"#define\s+GPMI_KERNEL_M52\s+4\b", header)


def test_device_plan():
    from inference_amd import _lib
    from inference_amd.gp import (ChangePoint, HeteroscedasticNoise, Matern32, Matern52, RationalQuadratic,
                                  SquaredExponential, WhiteNoise)
    from inference_amd.gp.covariance import device_plan, heteroscedastic_slice, sum_kernels

    x, _, _ = mh.dataset(65, 2, far=False)
    for cls, kid in ((Matern32, _lib.KERNEL_M32), (Matern52, _lib.KERNEL_M52)):
        cov = cls()
        cov.pass_spatial_data(x)
        assert device_plan(cov) == (kid, cov, slice(0, 3), None)
        cov = cls() + WhiteNoise()
        cov.pass_spatial_data(x)
        plan = device_plan(cov)
        assert plan[0] == kid and plan[1] is cov.components[0] and plan[2] == slice(0, 3) and plan[3] == 3
        cov = cls() + HeteroscedasticNoise()
        cov.pass_spatial_data(x)
        plan = device_plan(cov)
        assert plan[0] == kid and plan[3] is None and heteroscedastic_slice(cov) == slice(3, 3 + 65)
    cov = Matern52() + SquaredExponential()
    cov.pass_spatial_data(x)
    plan = device_plan(cov)
    assert plan[0] == _lib.KERNEL_SUM and list(plan[2]) == list(range(6))
    assert sum_kernels(cov) == [_lib.KERNEL_M52, _lib.KERNEL_SE]
    cov = Matern32() + RationalQuadratic() + WhiteNoise()
    cov.pass_spatial_data(x)
    plan = device_plan(cov)
    assert plan[0] == _lib.KERNEL_SUM and plan[3] == 7 and sum_kernels(cov) == [_lib.KERNEL_M32, _lib.KERNEL_RQ]
    cov = ChangePoint([Matern52(), SquaredExponential()])
    cov.pass_spatial_data(x)
    assert device_plan(cov)[0] == -1
    assert cov.device_terms(np.arange(8.0))[0] == [_lib.KERNEL_M52, _lib.KERNEL_SE]


@pytest.mark.parametrize("kind", list(KINDS))
def test_pickle_round_trip(kind):
    x, y, _ = mh.dataset(65, 3, far=False)
    cov = _cls(kind)()
    cov.pass_spatial_data(x)
    cov.estimate_hyperpar_bounds(y)
    back = pickle.loads(pickle.dumps(cov))
    assert type(back) is type(cov) and back.bounds == cov.bounds and back.n_params == cov.n_params
    assert back.hyperpar_labels == cov.hyperpar_labels and np.array_equal(back.x, cov.x) and back._engine is None


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_gradient_terms_against_central_differences(kind, d):
    """A_kn K(v, x_n) = dK(v, x_n)/dv_k against central differences of the oracle kernel in its first argument, step
    1e-5 l: truncation ~ h^2 K''' ~ 1e-10, rounding ~ 1e-16 / 1e-5 = 1e-11 - tolerance 1e-6 of the largest element."""
    x, _, _ = mh.dataset(65, d, far=False)
    theta = mh.theta_for(kind, d)
    scales = np.exp(theta[1:])
    cov = _cls(kind)()
    cov.pass_spatial_data(x)
    rng = np.random.default_rng(5)
    for q in rng.uniform(4.5, 6.0, size=(4, d)):  # query points away from the data
        A, R = cov.gradient_terms(q, x, theta)
        assert A.shape == (d, len(x)) and R.shape == (d,)
        k = mh.cross(kind, q[None, :], x, theta)[0]
        for i in range(d):
            h = np.zeros(d)
            h[i] = 1e-5 * scales[i]
            fd = (mh.cross(kind, (q + h)[None, :], x, theta)[0] - mh.cross(kind, (q - h)[None, :], x, theta)[0]) / (2 * h[i])
            err = np.abs(A[i] * k - fd).max() / np.abs(fd).max()
            assert err <= 1e-6, (kind, d, i, err)
        assert np.allclose(R, mh.G0[kind] * (np.exp(theta[0]) / scales) ** 2, rtol=1e-14, atol=0)
        Ao, Ro = mh.gradient_terms(kind, q, x, theta)
        assert np.allclose(A, Ao, rtol=1e-13, atol=0) and np.allclose(R, Ro, rtol=1e-14, atol=0)


def test_rq_and_changepoint_keep_the_reference_error():
    from inference_amd.gp import ChangePoint, Matern52, RationalQuadratic

    for cov in (RationalQuadratic(), ChangePoint([Matern52(), Matern52()])):
        with pytest.raises(NotImplementedError, match="Gradient calculations are not yet available"):
            cov.gradient_terms(None, None, None)


def test_matern_profile_accuracy_on_the_host(tmp_path):
    """tools/kmath_matern_check.cpp: C and g against long double at 1e7 values of s, log-uniform over [1e-30, 1e5], s = 0
    and the underflow edge; non-zero exit beyond (8 + 2 t) 2^-53 relative, C(0) != 1 or a NaN."""
    exe = str(tmp_path / "kmath_matern_check")
    src = os.path.join(ROOT, "tools", "kmath_matern_check.cpp")
    inc = os.path.join(ROOT, "inference-tools_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-I", inc, src, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
