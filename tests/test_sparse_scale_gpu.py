"""GPU tests of the inducing-point model and the greedy selection at the shapes where the device's schedules change
(tests/sparse_host.py: SCALE_CASES), against the mirrors' values in tests/golden/sparse_scale.npz
(tests/golden/make_golden_sparse_scale.py; tests/test_sparse_scale_cpu.py checks the fixture itself).

Every case first proves through gpmi_sgp_schedule / gpmi_select_schedule that it runs the branch it is named after, and
that the neighbouring smaller shape does not:
  tiles3      SE + WhiteNoise   N = 700     d = 2  m = 300   panel_rows 256    m_pad = 384: three 128-row tiles in both
                                                                               factorisations, three panels (the last of 188 rows)
  run4        Matern32          N = 32700   d = 1  m = 200   panel_rows 32768  4 data tiles per workgroup of the Z pass
  run8        Matern52          N = 32700   d = 1  m = 450   panel_rows 32768  8 tiles, m_pad = 512
  run16       Matern32          N = 32700   d = 1  m = 1000  panel_rows 32768  16 tiles, m_pad = 1024
  long        SE + WhiteNoise   N = 262444  d = 1  m = 5     panel_rows 0      the weights pass strides; 33 default panels
  max_m       Matern52          N = 300     d = 3  m = 4096  panel_rows 0      the limit of m; 8 tiles per workgroup in the K_mm term
  bench_like  SE + WhiteNoise   N = 16385   d = 8  m = 512   panel_rows 0      three default panels, the last of one row;
                                                                               cond(K_mm + eps I) = 2.4e6, the benchmark's regime

Allowances (the project's rule, unchanged; measured by the fixture's maker against the mirror, never against the device):
10 x the largest movement of the quantity under ripples of 1e-13 relative on the mirror's K_mm, K_mn and K_mq, floored at
1e-10 of its scale.  48 ripples per case, 8 for run16 and 6 for max_m (<case>/ripples in the fixture).  tiles3's posterior,
draws and derivatives are compared with a mirror computed here, by the same rule with 48 ripples.

Measured on one MI355X, device error / allowance (`pytest -m gpu -s tests/test_sparse_scale_gpu.py` prints them; also in
the README, "Large data: inducing points"):
  case        cond    F                    gradient             dF/dZ                alpha                mean                 variance
  tiles3      1.1e3   2.3e-11 / 1.7e-8     4.8e-9 / 4.3e-7      1.1e-8 / 2.9e-8      3.5e-10 / 1.2e-8     1.8e-13 / 1.1e-10    8.5e-14 / 1.2e-10
  run4        44      4.7e-10 / 1.8e-5     2.7e-7 / 4.8e-5      3.5e-6 / 1.1e-4      7.4e-11 / 1.4e-8     4.6e-14 / 1.3e-10    6.7e-16 / 1.2e-10
  run8        4.4e2   2.8e-9 / 2.7e-6      1.8e-7 / 2.0e-5      5.2e-6 / 4.7e-5      1.7e-9 / 7.8e-8      4.4e-14 / 1.3e-10    1.5e-15 / 1.2e-10
  run16       37      2.3e-10 / 1.7e-5     1.2e-7 / 4.6e-5      1.2e-6 / 1.5e-4      3.2e-11 / 2.0e-8     1.1e-14 / 1.3e-10    7.2e-16 / 1.2e-10
  long        92      2.1e-8 / 1.8e-5      2.7e-4 / 7.1e-3      5.0e-5 / 2.9e-3      2.5e-10 / 3.4e-9     2.6e-12 / 1.3e-10    8.9e-16 / 1.2e-10
  max_m       22      6.2e-11 / 8.7e-7     9.5e-10 / 1.7e-6     2.6e-10 / 3.5e-7     1.7e-10 / 9.8e-10    4.8e-14 / 5.5e-11    4.8e-14 / 1.2e-10
  bench_like  2.4e6   2.4e-4 / 1.3e-3      3.5e-2 / 2.3e1       1.3e-2 / 3.0e-2      3.2e-5 / 7.9e-4      1.8e-7 / 7.9e-7      7.9e-11 / 3.6e-10
run4 / run8 / run16 at panel_rows 8192 (runs of 2 / 2 / 4 tiles): F 4.7e-10 / 3.0e-9 / 2.3e-10, gradient 2.7e-7 / 1.8e-7 / 1.2e-7,
dF/dZ 3.6e-6 / 5.2e-6 / 1.2e-6, alpha 7.4e-11 / 1.7e-9 / 3.2e-11 (the allowances above).  tiles3 against the mirror computed
here: mu 2.7e-13 / 1.3e-10, Sigma 6.0e-14 / 1.1e-10, diag Sigma against the predictive variance 2.7e-15 / 1.1e-10, d mean
1.8e-11 / 6.8e-10, d var 3.4e-12 / 9.3e-10, L L^T 6.0e-14 / 1.1e-10; after the refused calls and at panel_rows 32768: F 2.4e-11,
dF/dZ 1.1e-8.  bench_like: cond(K_mm + eps I) 2.4e6; the mirror's own spread under one ripple F 1.3e-4, gradient 2.3, dF/dZ
3.0e-3, alpha 7.9e-5, mean 7.9e-8, variance 3.6e-11.  Selection at n = 66000, weighted / unweighted: the mirror's pivots,
trace 1.9e-9 / 8.8e-4 and 7.3e-12 / 6.6e-6, pivot variances 2.2e-16 / 1e-10 each; with 700 rows of weight 0 appended the
trace keeps its bits.  The sixteen tests take 2.4 s together (the mirrors' work is in the fixture).
"""
import ctypes as C

import numpy as np
import pytest

import sparse_host as sh
import sparse_post_host as sph
from sparse_host import MU, N_RIPPLES, check, full_theta, make_gp

pytestmark = pytest.mark.gpu

GPMI_OK, GPMI_ERR_ARG = 0, -1
QUANTITIES = ("F", "grad", "gz", "alpha", "mean", "var")
JITTER = 1e-9  # of the draws

_CASES, _MODELS = {}, {}


def scale_case(name):
    if name not in _CASES:
        _CASES[name] = sh.scale_case(name)
    return _CASES[name]


def model(name):
    """The fitted device model of a case, shared by the tests that do not change it."""
    if name not in _MODELS:
        _MODELS[name] = make_gp(scale_case(name))
    return _MODELS[name]


def expected(golden, name):
    g = golden("sparse_scale")
    case = scale_case(name)
    assert np.array_equal(g[f"{name}/x_ends"], case["x"][[0, -1]]) and np.array_equal(g[f"{name}/z_ends"], case["z"][[0, -1]])
    want = {k: g[f"{name}/{k}"] for k in QUANTITIES + ("alpha_idx",)}
    return case, want, dict(zip(QUANTITIES, g[f"{name}/allow"]))


def assert_on_its_branch(name):
    from inference_amd._engine import sgp_schedule

    kind, n, d, m, panel, white, ell = sh.SCALE_CASES[name]
    want, neighbour, other = sh.SCALE_SCHEDULE[name]
    got, near = sgp_schedule(n, m, panel), sgp_schedule(*neighbour)
    assert {k: got[k] for k in want} == want, got
    assert {k: near[k] for k in other} == other, near
    if name == "long":
        assert n > 256 * got["weight_blocks"] and neighbour[0] <= 256 * near["weight_blocks"]
    return got


def device_bound(gp, case, zgrad, panel_rows=None):
    th, white = gp._split(full_theta(case))
    return gp.engine.bound(gp._kernel_id, th, white, gp.jitter, gp.panel_rows if panel_rows is None else panel_rows, True, True,
                           want_zgrad=zgrad)


def compare_all(tag, gp, case, want, allow):
    """F, gradient, dF/dZ and alpha of the regressor's calls and of the engine's, against the fixture; the Z call keeps the
    bits of the call without Z and a repeated call is bit-identical."""
    theta = full_theta(case)
    check(f"{tag} F", gp.marginal_likelihood(theta), want["F"][0], allow["F"])
    F, grad, gz = gp.marginal_likelihood_gradient(theta, inducing_points=True)
    assert gz.shape == case["z"].shape and np.isfinite(gz).all()
    check(f"{tag} F (gradient call)", F, want["F"][0], allow["F"])
    check(f"{tag} gradient", grad, want["grad"], allow["grad"])
    print(f"{tag}: max |dF/dZ| {np.abs(want['gz']).max():.3e}")
    check(f"{tag} dF/dZ", gz, want["gz"], allow["gz"])
    F2, grad2 = gp.marginal_likelihood_gradient(theta)
    assert F2 == F and np.array_equal(grad2, grad)
    plain, a, b = device_bound(gp, case, False), device_bound(gp, case, True), device_bound(gp, case, True)
    assert plain[3] == 0 and a[3] == 0 and b[3] == 0
    assert plain[0] == a[0] == b[0] == F and np.array_equal(plain[1], a[1]) and np.array_equal(plain[2], a[2])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4]) and np.array_equal(a[4], gz)
    check(f"{tag} alpha", a[2][want["alpha_idx"]], want["alpha"], allow["alpha"])
    check(f"{tag} sum alpha", a[2].sum(), want["grad"][0], allow["grad"])
    return a


@pytest.mark.parametrize("name", sh.SCALE_NAMES)
def test_bound_gradients_and_prediction_against_the_fixture(golden, name):
    assert_on_its_branch(name)
    case, want, allow = expected(golden, name)
    if name == "bench_like":
        g = golden("sparse_scale")
        print(f"bench_like: cond(K_mm + eps I) {float(g['bench_like/cond']):.3g}; the mirror's own spread under "
              f"{int(g['bench_like/ripples'])} ripples of 1e-13: " + ", ".join(f"{k} {v:.2e}" for k, v in zip(QUANTITIES, g["bench_like/spread"])))
    gp = model(name)
    compare_all(name, gp, case, want, allow)
    mean, std = gp(case["q"])
    check(f"{name} mean", mean, want["mean"], allow["mean"])
    check(f"{name} variance", std**2, np.abs(want["var"]), allow["var"])
    again = gp(case["q"])
    assert np.array_equal(mean, again[0]) and np.array_equal(std, again[1])


@pytest.mark.parametrize("name", ["run4", "run8", "run16"])
def test_a_shorter_run_agrees(golden, name):
    """The same model at panel_rows = 8192: four panels and, as the query shows, a shorter run of tiles per workgroup (2, 2
    and 4 against 4, 8 and 16).  A cross-check of the two groupings, not the reference."""
    from inference_amd._engine import sgp_schedule

    kind, n, d, m, panel, white, ell = sh.SCALE_CASES[name]
    long_run, short_run = assert_on_its_branch(name), sgp_schedule(n, m, 8192)
    assert short_run["data_run_tiles"] < long_run["data_run_tiles"] and short_run["panels"] == 4
    case, want, allow = expected(golden, name)
    gp = make_gp(case, panel_rows=8192)
    compare_all(f"{name} at panel_rows 8192", gp, case, want, allow)


# ---- tiles3: the fitted model's other results, against a mirror computed here ------------------------------------------

def tiles3_queries(M):
    case = scale_case("tiles3")
    q = np.random.default_rng(700 + 10 * case["number"] + M).uniform(0.0, 1.0, size=(M, 2))
    q[1] = case["x"][len(case["x"]) // 2]
    q[2] = case["z"][len(case["z"]) // 2]
    return q


def _tiles3_quantities(case, mir, ripple=None):
    mir.ripple = ripple or (lambda name, A: A)
    st = mir.state(case["theta"], case["white"], case["y"] - MU, case["e"] ** 2)
    mu, sigma = sph.posterior(mir, st, case["theta"], tiles3_queries(130))
    dmean, dvar = sph.derivatives(mir, st, case["theta"], tiles3_queries(65))
    return dict(mu=mu + MU, sigma=sigma, var=np.diag(sigma).copy(), dmean=dmean, dvar=dvar)


_TILES3 = []


def tiles3_reference():
    """(mirror quantities, allowances) by the rule of tests/test_sparse_post_gpu.py, computed once."""
    if not _TILES3:
        case = scale_case("tiles3")
        mir = sh.SparseMirror(case["kind"], case["x"], case["z"])
        base = _tiles3_quantities(case, mir)
        spread = {k: 0.0 for k in base}
        for i in range(N_RIPPLES):
            moved = _tiles3_quantities(case, mir, sh.rippler(1000 * case["number"] + 500 + i))
            for k in base:
                spread[k] = max(spread[k], float(np.abs(moved[k] - base[k]).max()))
        scale = {k: float(np.abs(base["var" if k in ("sigma", "var") else k]).max()) for k in base}
        _TILES3.append((base, {k: max(10.0 * spread[k], 1e-10 * scale[k]) for k in base}))
    return _TILES3[0]


def test_tiles3_posterior_and_derivatives():
    assert_on_its_branch("tiles3")
    base, allow = tiles3_reference()
    gp = model("tiles3")
    q = tiles3_queries(130)
    mu, sigma = gp.build_posterior(q)
    assert mu.shape == (130,) and sigma.shape == (130, 130) and np.array_equal(sigma, sigma.T)
    check("tiles3 M = 130 mu", mu, base["mu"], allow["mu"])
    check("tiles3 M = 130 Sigma", sigma, base["sigma"], allow["sigma"])
    _, var = gp.engine.predict(q)
    check("tiles3 M = 130 diag Sigma against the predictive variance", np.diag(sigma), var, allow["var"])
    q = tiles3_queries(65)
    dmean, dvar = gp.spatial_derivatives_batch(q)
    assert dmean.shape == q.shape and dvar.shape == q.shape
    check("tiles3 M = 65 d mean", dmean, base["dmean"], allow["dmean"])
    check("tiles3 M = 65 d var", dvar, base["dvar"], allow["dvar"])
    # a row does not depend on the batch: the point alone, and as row 0 of another batch
    eng = gp.engine
    whole = eng.spatial_derivatives(q)
    other = tiles3_queries(130)[:64].copy()
    other[0] = q[40]
    alone, first = eng.spatial_derivatives(q[40:41]), eng.spatial_derivatives(other)
    for k in (0, 1):
        assert np.array_equal(whole[k], (dmean, dvar)[k])
        assert np.array_equal(whole[k][40], alone[k][0]) and np.array_equal(whole[k][40], first[k][0]), k


def test_tiles3_factor_identity():
    """z = I: draws - mu is L^T, and L L^T = Sigma + eps I."""
    base, allow = tiles3_reference()
    gp, M = model("tiles3"), 130
    q = tiles3_queries(M)
    D = gp.sample_posterior(q, M, z=np.eye(M), jitter=JITTER)
    Lt = D - gp.build_posterior(q, mean_only=True)
    assert np.array_equal(np.tril(Lt, -1), np.zeros((M, M)))
    maxd = float(base["var"].max())
    check("tiles3 M = 130 L L^T", Lt.T @ Lt, base["sigma"] + JITTER * maxd * np.eye(M), allow["sigma"])


# ---- the limits -----------------------------------------------------------------------------------------------------------

def test_max_m_set_inducing_points_equals_a_fresh_object(golden):
    assert_on_its_branch("max_m")
    case, want, allow = expected(golden, "max_m")
    fresh = model("max_m")
    moved = make_gp(case, z=case["z"] + 1e-3)
    moved.set_inducing_points(case["z"])
    a, b = fresh(case["q"]), moved(case["q"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert moved.bound == fresh.bound


def test_one_beyond_the_limits(golden):
    from inference_amd import _lib
    from inference_amd.gp import Matern52, SparseGpRegressor

    case, want, allow = expected(golden, "tiles3")
    gp = model("tiles3")
    eng = gp.engine
    # m = 4097: no object
    x, y, e = sh.dataset(300, 3)
    z = np.random.default_rng(1).uniform(0.0, 1.0, size=(_lib.SGP_MAX_M + 1, 3))
    ptr = C.c_void_p()
    assert eng.h.lib.gpmi_sgp_create(eng.h.ctx, 300, 3, _lib.dptr(x), len(z), _lib.dptr(z), C.byref(ptr)) == GPMI_ERR_ARG
    assert not ptr.value and b"m out of range" in eng.h.lib.gpmi_last_error(eng.h.ctx)
    with pytest.raises(ValueError):
        SparseGpRegressor(x, y, y_err=e, inducing_points=z, kernel=Matern52, hyperpars=np.array([MU, 0.1, -1.0, -1.0, -1.0]))
    ok = C.c_void_p()
    assert eng.h.lib.gpmi_sgp_create(eng.h.ctx, 300, 3, _lib.dptr(x), _lib.SGP_MAX_M, _lib.dptr(z[:-1]), C.byref(ok)) == GPMI_OK
    assert eng.h.lib.gpmi_sgp_destroy(ok) == GPMI_OK
    # panel_rows = 32769 on a live object; the next valid call gives the fixture's numbers
    th, white = gp._split(full_theta(case))
    th = np.ascontiguousarray(th, dtype=float)
    F, info = C.c_double(-7.0), C.c_int(-7)
    rc = eng.h.lib.gpmi_sgp_bound(eng.ptr, gp._kernel_id, _lib.dptr(th), th.size, white, gp.jitter, 32769, C.byref(F), None, None,
                                  C.byref(info))
    assert rc == GPMI_ERR_ARG and F.value == -7.0 and info.value == -7
    assert b"panel_rows out of range" in eng.h.lib.gpmi_last_error(eng.h.ctx)
    with pytest.raises(_lib.GpmiError, match="panel_rows"):
        eng.bound(gp._kernel_id, th, white, gp.jitter, 32769, True, True, want_zgrad=True)
    got = device_bound(gp, case, True)
    check("tiles3 F after the refused calls", got[0], want["F"][0], allow["F"])
    check("tiles3 dF/dZ after the refused calls", got[4], want["gz"], allow["gz"])
    at_limit = device_bound(gp, case, True, panel_rows=32768)  # (one panel of 768 rows here)
    check("tiles3 F at panel_rows 32768", at_limit[0], want["F"][0], allow["F"])
    check("tiles3 dF/dZ at panel_rows 32768", at_limit[4], want["gz"], allow["gz"])


# ---- the selection at 258 workgroups: every thread's strided read of the block partials -----------------------------------

@pytest.mark.parametrize("label", ["weighted", "unweighted"])
def test_selection_at_66000_points(golden, label):
    from inference_amd import _lib
    from inference_amd._engine import select_schedule
    from test_select_gpu import raw_select

    assert select_schedule(sh.SELECT_N) == 258 > 256 >= select_schedule(65536)
    assert select_schedule(sh.SELECT_N + sh.SELECT_EXTRA) == 261
    g = golden("sparse_scale")
    x, theta, w = sh.select_case()
    assert np.array_equal(g["select/x_ends"], x[[0, -1]])
    w = w if label == "weighted" else None
    want = {k: g[f"select/{label}_{k}"] for k in ("index", "trace", "pivot_var")}
    h = _lib.Handle()
    try:
        def run(xx, ww):
            rc, count, index, trace, pivot_var = raw_select(h, xx, theta, _lib.KERNEL_M52, sh.SELECT_M, ww)
            assert rc == GPMI_OK and count == sh.SELECT_M, h.lib.gpmi_last_error(h.ctx).decode()
            return dict(index=index, trace=trace, pivot_var=pivot_var)

        got, again = run(x, w), run(x, w)
        assert got["index"].tolist() == want["index"].tolist()
        check(f"selection {label} trace", got["trace"], want["trace"], 1e-10 * float(want["trace"][0]))
        check(f"selection {label} pivot_var", got["pivot_var"], want["pivot_var"], 1e-10)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)
        extra = np.random.default_rng(12).uniform(0.0, 1.0, size=(sh.SELECT_EXTRA, 2))
        longer = run(np.concatenate([x, extra]), np.concatenate([np.ones(len(x)) if w is None else w, np.zeros(sh.SELECT_EXTRA)]))
        assert longer["index"].tolist() == got["index"].tolist()
        assert longer["pivot_var"].tobytes() == got["pivot_var"].tobytes()
        check(f"selection {label}, 700 rows of weight 0 appended: trace", longer["trace"], got["trace"], 1e-10 * float(got["trace"][0]))
    finally:
        h.close()
