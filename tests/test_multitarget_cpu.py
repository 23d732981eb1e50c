"""
CPU tests of the many-target model: the NumPy / SciPy mirror (tests/multitarget_host.py) against sums and stacks of
single-target `OracleGp`s, its gradient against a finite difference, the argument checks of
`MultiTargetGpRegressor` that need no device, and the header / ctypes entries of gpmi_mt_*.  No GPU is needed.
"""
import os
import re

import numpy as np
import pytest

import multitarget_host as mth
import workloads as wl
from oracle import gp_oracle as orc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RTOL = 1e-12  # the identities behind the mirror were measured at 5e-16 .. 4e-15 on these inputs

# (kernel, white noise, N, d, T, M)
CASES = {"se_130x3": (orc.SE, False, 130, 3, 3, 50), "se_wn_300x129": (orc.SE, True, 300, 2, 129, 257)}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, tol, what):
    r = rel(a, b)
    print(f"{what}: {r:.2e}")
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"


_built = {}


def build(name):
    """(mirror, per-column oracles, theta, query points) of a case, computed once and shared."""
    if name not in _built:
        kernel, wn, n, d, T, M = CASES[name]
        x, y, e = wl.synthetic_dataset(1, n, d)
        Y = mth.make_targets(x, y, T)
        theta = mth.cov_theta(kernel, y, d, wn)
        means = Y.mean(axis=0)
        mirror = mth.MultiTargetMirror(x, Y, e, kernel, wn, means, theta)
        cols = mth.OracleColumns(x, Y, e, kernel, wn, means, theta)
        _built[name] = (mirror, cols, theta, wl.query_points(1, M, d))
    return _built[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_mirror_matches_the_sums_over_single_target_oracles(name):
    mirror, cols, theta, pts = build(name)
    # (the big case at the fitted theta alone: every column of the yardstick repeats the whole O(N^3) evaluation)
    for th, tag in ((theta, "fit theta"), (theta + 0.1, "other theta"))[:2 if mirror.T <= 8 else 1]:
        ref_t = cols.lml_t(th)
        check(mirror.marginal_likelihood(th, per_target=True), ref_t, RTOL, f"lml_t ({tag})")
        check(mirror.marginal_likelihood(th), ref_t.sum(), RTOL, f"LML ({tag})")
        lml, grad = mirror.marginal_likelihood_gradient(th)
        rl, rg = cols.lml_gradient(th)
        check(lml, rl, RTOL, f"LML of the gradient call ({tag})")
        check(grad, rg, RTOL, f"gradient ({tag})")
        check(mirror.loo_likelihood(th), cols.loo_likelihood(th), RTOL, f"loo_likelihood ({tag})")
    check(mirror.alpha, cols.alpha(), RTOL, "alpha")
    mu, sig = mirror(pts)
    rmu, rsig = cols.predict(pts)
    check(mu, rmu, RTOL, "means")
    check(sig, rsig, RTOL, "sigma")
    lmu, lsig = mirror.loo_predictions()
    rlmu, rlsig = cols.loo_predictions()
    check(lmu, rlmu, RTOL, "loo means")
    check(lsig, rlsig, RTOL, "loo sigma")


def _fd4(f, theta, h):
    """Central fourth-order finite difference of f along every coordinate."""
    out = np.empty(theta.size)
    for j in range(theta.size):
        e = np.zeros(theta.size)
        e[j] = h
        out[j] = (-f(theta + 2 * e) + 8 * f(theta + e) - 8 * f(theta - e) + f(theta - 2 * e)) / (12 * h)
    return out


def test_mirror_gradient_against_a_finite_difference():
    """The tolerance is what the same finite difference leaves on `OracleGp`'s own single-target gradient at the same
    step (the worst of the target columns), times ten."""
    mirror, cols, theta, _ = build("se_130x3")
    h = 1e-3
    ref_err = 0.0
    for t, g in enumerate(cols.gps):
        th = cols.theta(t, theta)
        grad = g.marginal_likelihood_gradient(th)[1][1:]
        fd = _fd4(lambda c: g.marginal_likelihood(np.concatenate([th[:1], c])), theta, h)
        ref_err = max(ref_err, rel(fd, grad))
    _, grad = mirror.marginal_likelihood_gradient(theta)
    err = rel(_fd4(mirror.marginal_likelihood, theta, h), grad)
    print(f"finite difference vs analytic gradient: single-target oracle {ref_err:.2e}, mirror {err:.2e}")
    assert err <= 10 * ref_err


def _model(**kw):
    from inference_amd.gp import MultiTargetGpRegressor

    x, y, e = wl.synthetic_dataset(1, 40, 2)
    args = dict(x=x, Y=mth.make_targets(x, y, 3), y_err=e, hyperpars=mth.cov_theta(orc.SE, y, 2))
    args.update(kw)
    return MultiTargetGpRegressor(**args)


def test_argument_checks_need_no_device(monkeypatch):
    import inference_amd.gp as gp
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    def no_device(*a, **k):
        raise AssertionError("a device context was created before the arguments were checked")

    monkeypatch.setattr(GpEngine, "__init__", no_device)
    x, y, e = wl.synthetic_dataset(1, 40, 2)
    Y = mth.make_targets(x, y, 3)
    with pytest.raises(ValueError):
        _model(Y=np.zeros((40, 3, 2)))
    with pytest.raises(ValueError):
        _model(Y=Y[:39])
    with pytest.raises(ValueError):
        _model(x=np.zeros((40, 65)), hyperpars=np.zeros(66))
    with pytest.raises(NotImplementedError, match="own covariance matrix"):
        _model(y_err=np.full((40, 3), 0.1))
    with pytest.raises(ValueError):
        _model(target_means=np.zeros(4))
    with pytest.raises(ValueError):
        _model(Y=np.zeros((40, _lib.MT_MAX_T + 1)))
    for kernel in (gp.ChangePoint(kernels=[gp.SquaredExponential, gp.SquaredExponential]),
                   gp.SquaredExponential() + gp.HeteroscedasticNoise(), _PluginKernel()):
        with pytest.raises(NotImplementedError):
            _model(kernel=kernel)


def _PluginKernel():
    from inference_amd.gp.covariance import CovarianceFunction

    class Plugin(CovarianceFunction):
        n_params = 1
        hyperpar_labels = ["a"]
        bounds = [(-1.0, 1.0)]

        def pass_spatial_data(self, x):
            self.x = x

        def estimate_hyperpar_bounds(self, y):
            pass

        def __call__(self, u, v, theta):
            return np.zeros((len(u), len(v)))

        def build_covariance(self, theta):
            return np.eye(len(self.x))

        def covariance_and_gradients(self, theta):
            return np.eye(len(self.x)), [np.eye(len(self.x))]

    return Plugin()


def test_construction_without_a_device_is_lazy_up_to_the_fit(monkeypatch):
    """Everything before the fit - coercion, offsets, labels, bounds - is host work: the engine is a lazy property."""
    from inference_amd._engine import GpEngine
    from inference_amd.gp import MultiTargetGpRegressor, SquaredExponential, WhiteNoise

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(GpEngine, "__init__", stop)
    x, y, e = wl.synthetic_dataset(1, 40, 2)
    Y = mth.make_targets(x, y, 3)
    seen = {}
    orig = MultiTargetGpRegressor.set_hyperparameters

    def spy(self, theta):
        seen.update(labels=self.hyperpar_labels, bounds=self.hp_bounds, means=self.target_means, T=self.n_targets,
                    engine=self._engine)
        return orig(self, theta)

    monkeypatch.setattr(MultiTargetGpRegressor, "set_hyperparameters", spy)
    with pytest.raises(Stop):
        MultiTargetGpRegressor(x, Y, y_err=e, hyperpars=np.zeros(4), kernel=SquaredExponential() + WhiteNoise())
    assert seen["engine"] is None and seen["T"] == 3 and len(seen["labels"]) == 4 == len(seen["bounds"])
    assert np.array_equal(seen["means"], Y.mean(axis=0))
    ref = SquaredExponential() + WhiteNoise()
    ref.pass_spatial_data(x)
    ref.estimate_hyperpar_bounds((Y - Y.mean(axis=0)[None, :]).ravel())
    assert seen["bounds"] == ref.bounds
    with pytest.raises(Stop):
        MultiTargetGpRegressor(x[:, 0], Y[:, 0], hyperpars=np.zeros(2), target_means=1.5)
    assert seen["T"] == 1 and np.array_equal(seen["means"], [1.5])


def test_header_and_ctypes_declare_the_entry_points():
    from inference_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    m = re.search(r"#define\s+GPMI_MT_MAX_T\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.MT_MAX_T
    names = ["gpmi_mt_set_targets", "gpmi_mt_fit", "gpmi_mt_lml", "gpmi_mt_lml_grad", "gpmi_mt_loo_terms", "gpmi_mt_alpha",
             "gpmi_mt_predict", "gpmi_mt_loo"]
    for name in names:
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\s*\(", header), name
    assert "api_multi.hip" in open(os.path.join(ROOT, "inference-tools_amd", "csrc", "Makefile")).read()
