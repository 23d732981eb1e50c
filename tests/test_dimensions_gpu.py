"""
GPU tests at 17 .. 64 spatial dimensions - the upper three quarters of what gpmi_set_data admits (GPMI_MAX_D = 64), where
every kernel that takes d has resources that grow with it: the [d][64] point panels in dynamic LDS (64 KiB at d = 64, plus
32 B of static LDS in the sum gradient), the length scales carried by value (KParams, CovParams of four components), the
n_theta + 1 = 4 d + 6 partials per tile of the gradient contraction, the d right-hand sides per point of the predictive
gradient and its chunks of 1024 // d points.

The yardstick is the NumPy / SciPy oracle of tests/matern_host.py; tests/test_dimensions_cpu.py shows that the oracle
alone meets these tolerances at these sizes (its K within 4e-16 of np.longdouble, cond <= 2e4) and that dropping the axes
from 16 on would move every compared quantity by more than 1e-3.  The length scales grow like sqrt(d)
(dims_host.theta_dims): with the other files' scales K would be its own diagonal at d = 64 and nothing behind the
factorisation would depend on the axes at all.  Tolerances are the project's own for the same quantities: 1e-13 of the
largest element for covariance elements, 1e-10 relative behind a factorisation (`check_each`: also element by element),
1e-12 between a batch member and its single evaluation.  Sizes are small on purpose: n = 130 is three covariance tiles
of 64 and two factor tiles of 128, both ragged; n = 65 one tile and one row.  Every test runs with the dense
host-composition entry points (`*_dense`) made to raise.  Every comparison prints its achieved error.
"""
import copy
import math

import numpy as np
import pytest

import dims_host as dh
import matern_host as mh

pytestmark = pytest.mark.gpu

RTOL = 1e-10
N = 130
KERNEL_ID = {"se": 0, "rq": 1, "m32": 3, "m52": 4}
REFUSAL = "Gradient calculations are not yet available"
GRADIENT_MODELS = ("se", "m52", "se+wn")  # the models with predictive-gradient kernels on the device


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not np.isnan(a).any()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, tol=RTOL, what=""):
    r = rel(a, b)
    print(f"{what}: {r:.2e} (tol {tol:.0e})")
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"
    return r


def check_each(a, b, tol=RTOL, what="", floor=1e-6, etol=1e-7):
    """`check` plus the element-wise half of tests/test_gpu_parity.py's check_each: every element larger than `floor` x
    the largest is held to `etol` relative to itself."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    check(a, b, tol, what)
    big = np.abs(b) > floor * np.abs(b).max()
    r = float((np.abs(a - b)[big] / np.abs(b)[big]).max()) if big.any() else 0.0
    print(f"{what} (element-wise, {int(big.sum())} of {big.size}): {r:.2e} (tol {etol:.0e})")
    assert r <= etol, f"{what}: element-wise relative error {r:.3e} > {etol:.1e}"
    return r


@pytest.fixture(autouse=True)
def no_dense_path(monkeypatch):
    from inference_amd._engine import GpEngine

    def tripwire(name):
        def fail(*args, **kwargs):
            raise AssertionError(f"GpEngine.{name} called: the model left the device path")

        return fail

    for name in dir(GpEngine):
        if name.endswith("_dense"):
            monkeypatch.setattr(GpEngine, name, tripwire(name))


def _cls(kind):
    import inference_amd.gp as gp

    return {"m32": gp.Matern32, "m52": gp.Matern52, "se": gp.SquaredExponential, "rq": gp.RationalQuadratic,
            "wn": gp.WhiteNoise}[kind]


def _device_cov(parts):
    import inference_amd.gp as gp

    objs = [gp.ChangePoint([_cls(k)() for k in p[1]], axis=p[2]) if p[0] == "cp" else _cls(p[0])() for p in parts]
    cov = objs[0]
    for o in objs[1:]:
        cov = cov + o
    return cov


def _gp(parts, x, y, e, theta, **kw):
    from inference_amd.gp import GpRegressor

    return GpRegressor(x, y, y_err=e, kernel=_device_cov(parts), hyperpars=theta, **kw)


def _queries(x, m, seed):
    u = np.random.default_rng(seed).uniform(0.0, 4.0, size=(m, x.shape[1]))
    u[0] = x[2]  # a query point on a training point
    return u


# ------------------------------------------------------------------------------------------------ A. build and cross
def _check_special_rows(K, Kq, amp2, power_law):
    """Row 1 of the data is a copy of row 0: C(0) = 1 exactly; the last row is 10^3 away: exp(-s) underflows to exactly
    0.0 (a RationalQuadratic's power-law tail leaves ~1e-8 a^2 there - compared with the oracle like any element)."""
    assert np.array_equal(K, K.T)
    assert K[0, 1] == amp2 == K[1, 0]
    assert Kq[0, 2] == amp2
    if power_law:
        assert 0.0 < np.abs(K[-1, :-1]).max() < 1e-7 * amp2 and 0.0 < np.abs(Kq[:, -1]).max() < 1e-7 * amp2
    else:
        assert not K[-1, :-1].any() and not K[:-1, -1].any() and not Kq[:, -1].any()


@pytest.mark.parametrize("n", [65, N])
@pytest.mark.parametrize("d", dh.DIMS)
@pytest.mark.parametrize("kind", dh.KINDS)
def test_build_and_cross(kind, d, n):
    x, _, _ = mh.dataset(n, d)
    theta = dh.theta_dims(kind, d, dh.seed_for(kind, d))
    cov = _cls(kind)()
    cov.pass_spatial_data(x)
    K = cov.build_covariance(theta)
    check(K, mh.build(kind, x, theta), 1e-13, f"d={d} build_covariance {kind} n={n}")
    u = _queries(x, 7, n + d)
    Kq = cov(u, x, theta)
    assert Kq.shape == (7, n)
    check(Kq, mh.cross(kind, u, x, theta), 1e-13, f"d={d} cov(u, x) {kind} n={n}")
    a = math.exp(theta[0])
    _check_special_rows(K, Kq, a * a, kind == "rq")


@pytest.mark.parametrize("d", [33, 64])
def test_build_and_cross_sum_of_four(d):
    """gpmi_covariance / gpmi_cross_covariance with GPMI_KERNEL_SUM: ksum_kernel with a CovParams of four components,
    every one with d length scales of its own."""
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    parts = dh.MODELS["se+rq+m32+m52"](d)
    x, y, e = mh.dataset(N, d)
    theta = dh.model_theta(parts, d)[1:]
    model = mh.HostModel(parts, x)
    u = _queries(x, 7, d)
    eng = GpEngine(x, y, noise_var=e**2)
    try:
        eng.set_sum([KERNEL_ID[p[0]] for p in parts])
        K = eng.covariance(_lib.KERNEL_SUM, theta)
        Kq = eng.cross_covariance(_lib.KERNEL_SUM, theta, u)
    finally:
        eng.close()
    check(K, model.build_and_grads(theta, grads=False)[0], 1e-13, f"d={d} covariance se+rq+m32+m52")
    check(Kq, model.cross(u, x, theta), 1e-13, f"d={d} cross covariance se+rq+m32+m52")
    amp2 = 0.0
    for sl in model.slices:  # a_m^2 in component order, as the kernel sums them
        a = math.exp(theta[sl][0])
        amp2 += a * a
    _check_special_rows(K, Kq, amp2, True)


# ------------------------------------------------------------------------------------------------ B. the regressor surface
@pytest.fixture(scope="module")
def cases():
    """(x, y, y_err, parts, theta, oracle, query points) per model and d, computed once."""
    cache = {}

    def get(tag, d, far=True):
        key = (tag, d, far)
        if key not in cache:
            x, y, e = mh.dataset(N, d, far=far)
            parts = dh.MODELS[tag](d)
            theta = dh.model_theta(parts, d)
            pts = _queries(x, 37, d)
            cache[key] = (x, y, e, parts, theta, mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta), pts)
        return cache[key]

    return get


@pytest.mark.parametrize("d", [17, 33, 64])
@pytest.mark.parametrize("tag", list(dh.MODELS))
def test_regressor_surface(cases, tag, d):
    from inference_amd import _lib

    x, y, e, parts, theta, orc, pts = cases(tag, d)
    gp = _gp(parts, x, y, e, theta)
    w = f"d={d} {tag}"
    assert gp._generic is False and gp.n_hyperpars == theta.size
    if tag.startswith("cp"):
        assert gp._kernel_id == -1
    elif sum(p[0] != "wn" for p in parts) > 1:
        assert gp._kernel_id == _lib.KERNEL_SUM
    else:
        assert gp._kernel_id == KERNEL_ID[parts[0][0]]
    check(gp.K_xx, orc.K, 1e-13, f"{w} K_xx")
    L = gp.L
    assert np.all(np.triu(L, 1) == 0.0)
    check(L, orc.L, what=f"{w} L")
    check_each(gp.alpha, orc.alpha, what=f"{w} alpha")
    check(gp.marginal_likelihood(theta), orc.marginal_likelihood(theta), what=f"{w} lml")
    v, g = gp.marginal_likelihood_gradient(theta)
    ov, og = orc.marginal_likelihood_gradient(theta)
    assert g.shape == (theta.size,)
    check(v, ov, what=f"{w} lml (gradient call)")
    check_each(g, og, what=f"{w} lml gradient")
    check(gp.loo_likelihood(theta), orc.loo_likelihood(theta), what=f"{w} loo")
    v, g = gp.loo_likelihood_gradient(theta)
    ov, og = orc.loo_likelihood_gradient(theta)
    check(v, ov, what=f"{w} loo (gradient call)")
    check_each(g, og, what=f"{w} loo gradient")
    mu, sig = gp(pts)
    omu, osig = orc(pts)
    check(mu, omu, what=f"{w} mu")
    check(sig, osig, what=f"{w} sigma")
    pm, pc = gp.build_posterior(pts[:16])
    om, oc = orc.build_posterior(pts[:16])
    check(pm, om, what=f"{w} posterior mean")
    check(pc, oc, what=f"{w} posterior covariance")
    if tag not in GRADIENT_MODELS:  # no gradient_terms, as in the reference: the documented refusal, not a fall-back
        for call in (gp.gradient, gp.spatial_derivatives, gp.spatial_derivatives_batch):
            with pytest.raises(NotImplementedError, match=REFUSAL):
                call(pts[:2])
    assert gp._generic is False


@pytest.mark.parametrize("d", [17, 33, 64])
@pytest.mark.parametrize("tag", GRADIENT_MODELS)
def test_predictive_gradients_across_a_chunk(cases, tag, d):
    """gpmi_gradient solves d right-hand sides per point in chunks of 1024 // d points: one point more than a chunk
    (61, 32 and 17 points), and two.  No far point: the oracle's gradient_terms divides by K(q, x_n).  WhiteNoise is
    part of the factor and of alpha only: the oracle's cross-covariance terms take the kernel's own parameters."""
    x, y, e, parts, theta, orc, pts = cases(tag, d, far=False)
    gp = _gp(parts, x, y, e, theta)
    kind = parts[0][0]
    if tag.endswith("+wn"):
        orc = copy.copy(orc)
        orc.theta = theta[:-1]
    for m in (1024 // d + 1, 2):
        q = _queries(x, m, 100 * d + m)
        w = f"d={d} {tag} m={m}"
        gmu, gcov = gp.gradient(q)
        omu, ocov = orc.gradient(q, kind)
        assert gmu.shape == (m, d) and gcov.shape == (m, d, d)
        check(gmu, omu, what=f"{w} gradient mean")
        check(gcov, ocov, what=f"{w} gradient covariance")
        dmu, dvar = gp.spatial_derivatives(q)
        odmu, odvar = orc.spatial_derivatives(q, kind)
        assert dmu.shape == dvar.shape == (m, d)
        check(dmu, odmu, what=f"{w} d mu / dx")
        check(dvar, odvar, what=f"{w} d var / dx")


# ------------------------------------------------------------------------------------------------ C. lockstep batches, d = 64
@pytest.mark.parametrize("tag", ["se", "rq", "se+rq+m32+m52"])
def test_lockstep_batches_at_64_dimensions(cases, tag):
    d, T = 64, 5
    x, y, e, parts, theta, orc, _ = cases(tag, d)
    gp = _gp(parts, x, y, e, theta)
    thetas = dh.batch_thetas(parts, d, T)
    w = f"d={d} {tag}"
    lml = gp.marginal_likelihood_batch(thetas)
    gv, gg = gp.marginal_likelihood_gradient_batch(thetas)
    lv, lg = gp.loo_likelihood_gradient_batch(thetas)
    assert lml.shape == gv.shape == lv.shape == (T,) and gg.shape == lg.shape == (T, theta.size)
    for t, th in enumerate(thetas):
        ov, og = orc.marginal_likelihood_gradient(th)
        check(lml[t], ov, what=f"{w} lml batch [{t}] vs oracle")
        check(gv[t], ov, what=f"{w} gradient batch [{t}]: lml vs oracle")
        check_each(gg[t], og, what=f"{w} gradient batch [{t}]: gradient vs oracle")
        olv, olg = orc.loo_likelihood_gradient(th)
        check(lv[t], olv, what=f"{w} loo gradient batch [{t}]: loo vs oracle")
        check_each(lg[t], olg, what=f"{w} loo gradient batch [{t}]: gradient vs oracle")
        check(lml[t], gp.marginal_likelihood(th), 1e-12, f"{w} lml batch [{t}] vs single")
        sv, sg = gp.marginal_likelihood_gradient(th)
        check(gv[t], sv, 1e-12, f"{w} gradient batch [{t}]: lml vs single")
        check(gg[t], sg, 1e-12, f"{w} gradient batch [{t}]: gradient vs single")
        sv, sg = gp.loo_likelihood_gradient(th)
        check(lv[t], sv, 1e-12, f"{w} loo gradient batch [{t}]: loo vs single")
        check(lg[t], sg, 1e-12, f"{w} loo gradient batch [{t}]: gradient vs single")


@pytest.mark.parametrize("tag", ["se", "rq", "se+rq+m32+m52"])
def test_marginalised_prediction_at_64_dimensions(cases, tag):
    d, T = 64, 3
    x, y, e, parts, theta, _, pts = cases(tag, d)
    gp = _gp(parts, x, y, e, theta)
    assert gp._lockstep_predict_ok()
    thetas = dh.batch_thetas(parts, d, T)
    q = pts[:9]
    means, sigs = gp.predict_samples(q, thetas)
    mix_mu, mix_sig = gp.predict_marginalised(q, thetas)
    model = mh.HostModel(parts, x)
    each = [mh.OracleGp(x, y, e, model, th)(q) for th in thetas]
    om, os_ = np.array([r[0] for r in each]), np.array([r[1] for r in each])
    w = f"d={d} {tag}"
    check(means, om, what=f"{w} predict_samples: means")
    check(sigs, os_, what=f"{w} predict_samples: sigmas")
    mean = om.mean(axis=0)
    check(mix_mu, mean, what=f"{w} predict_marginalised: mean")
    check(mix_sig, np.sqrt((os_**2 + (om - mean) ** 2).mean(axis=0)), what=f"{w} predict_marginalised: sigma")


# ------------------------------------------------------------------------------------------------ D. the limit
def test_65_dimensions_are_refused_and_the_handle_lives_on():
    import ctypes as C

    from inference_amd import _lib
    from inference_amd._lib import dptr

    x65, y, e = mh.dataset(N, 65)
    x64 = np.ascontiguousarray(x65[:, :64])
    noise = e**2
    h = _lib.Handle()
    try:
        with pytest.raises(_lib.GpmiError, match=r"GPMI_MAX_D \(64\)"):
            h.call("gpmi_set_data", dptr(x65), dptr(y), dptr(noise), None, N, 65)
        h.call("gpmi_set_data", dptr(x64), dptr(y), dptr(noise), None, N, 64)
        theta = dh.model_theta([("se",)], 64)
        mu, theta_cov = np.full(N, theta[0]), np.ascontiguousarray(theta[1:])
        alpha, logdet, info = np.empty(N), C.c_double(0.0), C.c_int(0)
        h.call("gpmi_fit", _lib.KERNEL_SE, dptr(theta_cov), theta_cov.size, 0.0, dptr(mu), dptr(alpha),
               C.byref(logdet), C.byref(info))
        assert info.value == 0
        orc = mh.OracleGp(x64, y, e, mh.HostModel([("se",)], x64), theta)
        check_each(alpha, orc.alpha, what="d=64 alpha after a refused d=65 data set")
        check(logdet.value, np.log(np.diag(orc.L)).sum(), what="d=64 log-determinant after a refused d=65 data set")
        # refused again with a fit in place: the handle keeps that fit
        with pytest.raises(_lib.GpmiError, match=r"GPMI_MAX_D \(64\)"):
            h.call("gpmi_set_data", dptr(x65), dptr(y), dptr(noise), None, N, 65)
        K = np.empty((N, N))
        h.call("gpmi_get_K", dptr(K))
        check(K, orc.K, 1e-13, "d=64 K_xx after a second refusal")
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ E. more than one chunk
@pytest.mark.parametrize("T", [64, 65, 130])
def test_gradient_batches_beyond_one_chunk(T):
    """The lockstep gradient workspace of a fresh handle holds min(T, 64) problems, and that is the chunk: 64 is one
    chunk exactly, 65 a chunk and a single problem, 130 two chunks and two.  After a likelihood batch of 200 has grown
    the workspace, the same 130 run as one chunk and must not change in any bit."""
    d = 3
    x, y, e = mh.dataset(N, d)
    parts = [("se",)]
    theta = np.concatenate([[0.1], mh.theta_for("se", d)])
    rng = np.random.default_rng(T)
    thetas = theta[None, :] + 0.1 * rng.standard_normal((T, theta.size))
    gp = _gp(parts, x, y, e, theta)
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), theta)
    first = (*gp.marginal_likelihood_gradient_batch(thetas), *gp.loo_likelihood_gradient_batch(thetas))
    assert first[1].shape == first[3].shape == (T, theta.size)
    for t in sorted({0, 63, 64, 65, T - 1}):
        if t < T:
            ov, og = orc.marginal_likelihood_gradient(thetas[t])
            check(first[0][t], ov, what=f"T={T} gradient batch [{t}]: lml vs oracle")
            check_each(first[1][t], og, what=f"T={T} gradient batch [{t}]: gradient vs oracle")
            ov, og = orc.loo_likelihood_gradient(thetas[t])
            check(first[2][t], ov, what=f"T={T} loo gradient batch [{t}]: loo vs oracle")
            check_each(first[3][t], og, what=f"T={T} loo gradient batch [{t}]: gradient vs oracle")
    single = [gp.marginal_likelihood_gradient(t) for t in thetas]
    check(first[0], [s[0] for s in single], 1e-12, f"T={T} gradient batch: lml vs single")
    check(first[1], np.array([s[1] for s in single]), 1e-12, f"T={T} gradient batch: gradient vs single")
    single = [gp.loo_likelihood_gradient(t) for t in thetas]
    check(first[2], [s[0] for s in single], 1e-12, f"T={T} loo gradient batch: loo vs single")
    check(first[3], np.array([s[1] for s in single]), 1e-12, f"T={T} loo gradient batch: gradient vs single")
    grow = theta[None, :] + 0.1 * rng.standard_normal((200, theta.size))
    lml = gp.marginal_likelihood_batch(grow)
    check(lml[:3], [orc.marginal_likelihood(t) for t in grow[:3]], what=f"T={T} lml batch of 200 vs oracle")
    again = (*gp.marginal_likelihood_gradient_batch(thetas), *gp.loo_likelihood_gradient_batch(thetas))
    for a, b, what in zip(first, again, ("lml", "lml gradient", "loo", "loo gradient")):
        assert np.array_equal(a, b), f"T={T} {what}: changed after the workspace grew (max {np.abs(a - b).max():.2e})"
