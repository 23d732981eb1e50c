"""
CPU tests of sums of stationary covariance kernels (GPMI_KERNEL_SUM): which covariance objects `device_plan` maps onto
the fused device sum, the parameter gather of the sum plan, labels and bounds against the reference (tests/golden/
sum.npz), and the C-ABI declarations (header, ctypes table).
"""
import os
import re

import numpy as np
import pytest

from inference_amd import _lib
from inference_amd.gp.covariance import (
    ChangePoint,
    HeteroscedasticNoise,
    RationalQuadratic,
    SquaredExponential,
    WhiteNoise,
    device_plan,
    sum_kernels,
)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SE, RQ = SquaredExponential, RationalQuadratic


def _sum(*parts):
    cov = parts[0]
    for p in parts[1:]:
        cov = cov + p
    return cov


def _prepared(cov, d=2, n=40):
    x = np.random.default_rng(0).uniform(0, 1, (n, d))
    cov.pass_spatial_data(x)
    return cov


@pytest.mark.parametrize(
    "parts, kinds",
    [
        ((SE(), RQ()), [_lib.KERNEL_SE, _lib.KERNEL_RQ]),
        ((SE(), SE()), [_lib.KERNEL_SE, _lib.KERNEL_SE]),
        ((SE(), RQ(), WhiteNoise()), [_lib.KERNEL_SE, _lib.KERNEL_RQ]),
        ((WhiteNoise(), RQ(), SE()), [_lib.KERNEL_RQ, _lib.KERNEL_SE]),
        ((RQ(), SE(), WhiteNoise(), SE()), [_lib.KERNEL_RQ, _lib.KERNEL_SE, _lib.KERNEL_SE]),
        ((RQ(), SE(), SE(), RQ(), WhiteNoise()), [_lib.KERNEL_RQ, _lib.KERNEL_SE, _lib.KERNEL_SE, _lib.KERNEL_RQ]),
    ],
)
def test_device_plan_accepts_sums(parts, kinds):
    cov = _prepared(_sum(*parts))
    plan = device_plan(cov)
    assert plan is not None
    kid, main, idx, wn = plan
    assert kid == _lib.KERNEL_SUM
    assert main is cov
    assert sum_kernels(cov) == kinds
    # the gathered indices are the stationary components' parameters, in component order
    want = [i for comp, sl in zip(cov.components, cov.slices) if not isinstance(comp, WhiteNoise)
            for i in range(sl.start, sl.stop)]
    assert list(idx) == want
    wn_pos = [sl.start for comp, sl in zip(cov.components, cov.slices) if isinstance(comp, WhiteNoise)]
    assert wn == (wn_pos[0] if wn_pos else None)


@pytest.mark.parametrize(
    "parts",
    [
        (SE(), SE(), SE(), SE(), SE()),                 # more than four stationary components
        (SE(), RQ(), WhiteNoise(), WhiteNoise()),        # two WhiteNoise terms
        (SE(), RQ(), HeteroscedasticNoise()),            # per-point noise
        (ChangePoint(kernels=[SE, SE]), SE()),           # a ChangePoint inside the sum
    ],
)
def test_device_plan_rejects_out_of_scope_sums(parts):
    cov = _prepared(_sum(*parts))
    plan = device_plan(cov)
    assert plan is None or plan[0] != _lib.KERNEL_SUM


def test_single_kernel_plans_unchanged():
    assert device_plan(_prepared(SE()))[0] == _lib.KERNEL_SE
    plan = device_plan(_prepared(RQ() + WhiteNoise()))
    assert plan[0] == _lib.KERNEL_RQ and plan[2] == slice(0, 4) and plan[3] == 4


def test_sum_theta_gather():
    cov = _prepared(_sum(RQ(), WhiteNoise(), SE()), d=3)
    _, _, idx, wn = device_plan(cov)
    theta = np.arange(cov.n_params, dtype=float)
    # RQ: 5 parameters, WhiteNoise: 1, SE: 4
    assert list(theta[idx]) == [0, 1, 2, 3, 4, 6, 7, 8, 9]
    assert wn == 5


def _golden_sum():
    return np.load(os.path.join(ROOT, "tests", "golden", "sum.npz"))


@pytest.mark.parametrize(
    "tag, parts, d",
    [
        ("serq", lambda: (SE(), RQ()), 2),
        ("sese", lambda: (SE(), SE()), 1),
        ("serqwn", lambda: (SE(), RQ(), WhiteNoise()), 2),
        ("rqsesewn", lambda: (RQ(), SE(), SE(), WhiteNoise()), 3),
    ],
)
def test_labels_and_bounds_match_reference(tag, parts, d):
    from inference_amd.gp.mean import ConstantMean

    g = _golden_sum()
    x, y = g[f"{tag}_x"], g[f"{tag}_y"]
    assert x.shape[1] == d
    cov, mean = _sum(*parts()), ConstantMean()
    cov.pass_spatial_data(x)
    mean.pass_spatial_data(x)
    cov.estimate_hyperpar_bounds(y)
    mean.estimate_hyperpar_bounds(y)
    labels = [*mean.hyperpar_labels, *cov.hyperpar_labels]
    bounds = [*mean.bounds, *cov.bounds]
    assert labels == list(g[f"{tag}_labels"])
    np.testing.assert_allclose(np.array(bounds, dtype=float), g[f"{tag}_bounds"], rtol=1e-12, atol=0)


def test_sum_in_header_and_signatures():
    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    assert re.search(r"#define\s+GPMI_KERNEL_SUM\s+2\b", header)
    assert re.search(r"int\s+gpmi_set_sum\s*\(\s*gpmi_ctx\s*\*\s*ctx\s*,\s*int\s+nk\s*,\s*const\s+int\s*\*\s*kernels\s*\)",
                     header)
    assert _lib.KERNEL_SUM == 2
    assert "gpmi_set_sum" in _lib.SIGNATURES
