"""
The oracle at 17 .. 64 spatial dimensions, on its own: that tests/matern_host.py meets, without any device, the conditions
tests/test_dimensions_gpu.py relies on when it holds the device kernels to the project's tolerances at these d.  This is
not a test of the device.

  1. the float64 oracle's K agrees with an np.longdouble evaluation far inside the 1e-13 the device is held to; the
     correlations are neither 0 nor 1; K + sigma^2 is well conditioned; no length-scale component of the likelihood
     gradients is so small that the element-wise half of `check_each` (floor 1e-6) would leave it unconstrained;
  2. a kernel that ignored the axes >= 16 - every d the suite used before these files - would be seen: its K, alpha,
     likelihoods' gradients and predictive means differ from the true ones by far more than any tolerance;
  3. with the length scales the other test files use, none of that holds at d = 64: K is its own diagonal.

And the limit itself: 65 columns are refused in Python, with the limit in the message, before the native library is
touched.
"""
import os
import re

import numpy as np
import pytest

import dims_host as dh
import matern_host as mh

N = 130


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _offdiag(C):
    """The off-diagonal correlations that are neither the far row's (exactly or nearly 0) nor the duplicated pair's (1)."""
    C = C[:-1, :-1]
    keep = np.triu(np.ones(C.shape, dtype=bool), 1)
    keep[0, 1] = False
    return C[keep]


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(kind, d):
        if (kind, d) not in cache:
            x, y, e = mh.dataset(N, d)
            parts = [(kind,)]
            theta = dh.model_theta(parts, d, dh.seed_for(kind, d))
            cache[(kind, d)] = (x, y, e, parts, theta, mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta))
        return cache[(kind, d)]

    return get


# ------------------------------------------------------------------------------------------------ 1. conditions
@pytest.mark.parametrize("d", dh.DIMS)
@pytest.mark.parametrize("kind", dh.KINDS)
def test_oracle_meets_the_conditions_of_the_gpu_tests(oracles, kind, d):
    x, y, e, parts, theta, orc = oracles(kind, d)
    K = mh.cross(kind, x, x, theta[1:])
    Kl = dh.cross_ld(kind, x, x, theta[1:])
    err = float(np.abs(K - Kl).max() / np.abs(Kl).max())
    off = _offdiag(K / np.exp(2.0 * theta[1]))
    cond = float(np.linalg.cond(orc.K))
    sl = dh.scale_slices(parts, d)[0]
    _, g_lml = orc.marginal_likelihood_gradient(theta)
    _, g_loo = orc.loo_likelihood_gradient(theta)
    r_lml = float(np.abs(g_lml[sl]).min() / np.abs(g_lml).max())
    r_loo = float(np.abs(g_loo[sl]).min() / np.abs(g_loo).max())
    print(f"{kind} d={d}: float64 vs longdouble K {err:.1e}; off-diagonal C {off.min():.3f} .. {off.max():.3f} "
          f"(median {np.median(off):.3f}); cond {cond:.1e}; smallest / largest gradient component: LML {r_lml:.1e}, "
          f"LOO {r_loo:.1e}")
    assert err <= 1e-14
    assert 0.05 <= off.min() and off.max() <= 0.9
    assert cond <= 1e5
    assert r_lml >= 1e-5 and r_loo >= 1e-5
    # the two special rows the GPU file asserts on: the copy of row 0, and the row 10^3 away (exactly 0 where the
    # covariance has an exponential tail; RationalQuadratic's power law leaves ~1e-8 a^2, which is not 0)
    assert K[0, 1] == K[0, 0] == np.exp(2.0 * theta[1])
    if kind == "rq":
        assert 0.0 < np.abs(K[-1, :-1]).max() < 1e-7 * K[0, 0]
    else:
        assert not K[-1, :-1].any()


@pytest.mark.parametrize("d", (17, 33, 64))
@pytest.mark.parametrize("tag", list(dh.MODELS))
def test_regressor_models_are_well_conditioned(tag, d):
    """The models of the GPU file's regressor tests: cond <= 1e5 as for the single kernels, and no component of alpha or
    of either gradient below the 1e-6 floor of `check_each` - all of them are compared element by element."""
    x, y, e = mh.dataset(N, d)
    parts = dh.MODELS[tag](d)
    theta = dh.model_theta(parts, d)
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta)
    assert theta.size == orc.m.n_params + 1
    cond = float(np.linalg.cond(orc.K))
    _, g_lml = orc.marginal_likelihood_gradient(theta)
    _, g_loo = orc.loo_likelihood_gradient(theta)
    ratios = [float(np.abs(v).min() / np.abs(v).max()) for v in (orc.alpha, g_lml, g_loo)]
    print(f"{tag} d={d}: {theta.size} parameters; cond {cond:.1e}; smallest / largest of alpha {ratios[0]:.1e}, "
          f"LML gradient {ratios[1]:.1e}, LOO gradient {ratios[2]:.1e}")
    assert cond <= 1e5
    assert min(ratios) >= 1e-5


def test_the_sum_of_four_reaches_the_largest_parameter_count():
    parts = dh.MODELS["se+rq+m32+m52"](64)
    assert dh.model_theta(parts, 64).size - 1 == 4 * 64 + 5 == 261


# ------------------------------------------------------------------------------------------------ 2. sensitivity
@pytest.mark.parametrize("d", dh.DIMS)
@pytest.mark.parametrize("kind", dh.KINDS)
def test_dropping_the_axes_from_16_on_is_visible(oracles, kind, d):
    x, y, e, parts, theta, orc = oracles(kind, d)
    _, xt, tt, kept = dh.truncated(parts, x, theta)
    assert xt.shape == (N, 16) and tt.size == theta.size - (d - 16)
    cut = mh.OracleGp(xt, y, e, mh.HostModel(parts, xt), tt)
    pts = np.random.default_rng(d).uniform(0.0, 4.0, size=(37, d))
    diffs = {
        "K": rel(cut.K, orc.K),
        "alpha": rel(cut.alpha, orc.alpha),
        "lml": rel(cut.marginal_likelihood(tt), orc.marginal_likelihood(theta)),
        "lml gradient": rel(cut.marginal_likelihood_gradient(tt)[1], orc.marginal_likelihood_gradient(theta)[1][kept]),
        "loo": rel(cut.loo_likelihood(tt), orc.loo_likelihood(theta)),
        "loo gradient": rel(cut.loo_likelihood_gradient(tt)[1], orc.loo_likelihood_gradient(theta)[1][kept]),
        "mu": rel(cut(pts[:, :16])[0], orc(pts)[0]),
    }
    print(f"{kind} d={d}: without the axes >= 16: " + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
    for what, v in diffs.items():
        assert v > 1e-3, f"{what}: a kernel that ignored the axes >= 16 would differ by only {v:.1e}"


# ------------------------------------------------------------------------------------------------ 3. the trap
def test_unscaled_length_scales_make_K_diagonal_at_d_64():
    """Why `theta_dims` exists: with `theta_for` as the other files use it, the largest off-diagonal correlation at
    d = 64 is below 1e-12 for SquaredExponential - and below the 0.05 that condition 1 asks for with every kernel - so a
    comparison of anything behind the factorisation would pass whatever a kernel did with most of the axes."""
    x, _, _ = mh.dataset(N, 64)
    for kind in dh.KINDS:
        th = mh.theta_for(kind, 64)
        off = _offdiag(mh.cross(kind, x, x, th) / np.exp(2.0 * th[0]))
        print(f"{kind}: largest off-diagonal C with unscaled length scales {off.max():.1e}")
        assert off.max() < (1e-12 if kind == "se" else 0.05)


# ------------------------------------------------------------------------------------------------ the limit of 64
def test_65_dimensions_are_refused_before_the_library_is_loaded(monkeypatch):
    from inference_amd import _lib
    from inference_amd.gp import (ChangePoint, GpRegressor, Matern32, Matern52, RationalQuadratic, SquaredExponential,
                                  WhiteNoise, _messages)

    def no_load():
        raise AssertionError("the native library was asked for")

    monkeypatch.setattr(_lib, "load", no_load)
    assert _messages.MAX_DIMENSIONS == 64
    header = os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "gpmi_internal.h")
    with open(header) as f:  # the Python limit is the library's
        assert re.search(r"constexpr int GPMI_MAX_D = (\d+);", f.read()).group(1) == str(_messages.MAX_DIMENSIONS)
    x, y, e = mh.dataset(20, 65, far=False)
    for kernel in (SquaredExponential, RationalQuadratic(), Matern52() + WhiteNoise(),
                   ChangePoint([SquaredExponential(), Matern32()], axis=64), mh.HostKernel("se")):
        with pytest.raises(ValueError, match=r"65 spatial dimensions.*\n.*at most 64"):
            GpRegressor(x, y, y_err=e, kernel=kernel, hyperpars=np.zeros(3))
    for cls in (SquaredExponential, RationalQuadratic, Matern32, Matern52):
        cov = cls()
        with pytest.raises(ValueError, match=r"65 spatial dimensions.*\n.*at most 64"):
            cov.pass_spatial_data(x)
        cov.pass_spatial_data(x[:, :64])  # the limit itself is admitted
        assert cov.n_params == 64 + 1 + (cls is RationalQuadratic)
