"""GPU tests of the lockstep batches of the sparse model: gpmi_sgp_bound_batch through `SparseEngine.bound_batch` and
through `SparseGpRegressor.marginal_likelihood_batch` / `marginal_likelihood_gradient_batch`, and the lockstep drivers on
a sparse model.  Row sets, mirror values and allowances: tests/sparse_batch_host.py (per row and quantity, 10 x the
largest movement under 48 ripples of 1e-13 on the mirror's K_mm and K_mn, floored at 1e-10 of the quantity's scale).
The fixture conditions behind them are asserted on the CPU, tests/test_sparse_batch_cpu.py.
`pytest -m gpu -s` prints every device error beside its allowance (the README's table, "Lockstep batches").
"""
import ctypes as C
import warnings

import numpy as np
import pytest
from numpy.linalg import LinAlgError
from numpy.random import default_rng
from numpy.testing import assert_array_equal

import ensemble_host as eh
import hmc_host as hh
import sparse_batch_host as bh
import sparse_host as sh
from sparse_batch_host import bits
from sparse_host import check

pytestmark = pytest.mark.gpu


def engine_args(case, rows):
    """(stationary thetas (T, n_theta), white variances (T,), constant means (T,)) of full vectors."""
    parts = [bh.split_row(case, row) for row in rows]
    return np.array([p[1] for p in parts]), np.array([p[2] for p in parts]), np.array([p[0] for p in parts])


def engine_batch(gp, case, rows, want_grad=True, want_alpha=False, max_chunk=0):
    th, white, mu = engine_args(case, rows)
    return gp.engine.bound_batch(gp._kernel_id, th, white, gp.jitter, case["panel"], mu_const=mu, want_grad=want_grad,
                                 want_alpha=want_alpha, max_chunk=max_chunk)


def full_gradient(case, g, sum_alpha):
    """The engine's (T, n_theta + 1) gradient and sum_alpha in the class's layout [mean | kernel | (ln s)]."""
    return np.column_stack([sum_alpha, g if case["white"] > 0.0 else g[:, :-1]])


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(number, jitter=1e-8):
        if (number, jitter) not in cache:
            gp = bh.make_gp(sh.case(number), jitter=jitter)
            gp.engine.set_observations(gp.y, gp._noise_var)
            gp._observations_up = True
            cache[number, jitter] = gp
        return cache[number, jitter]

    return get


# ---- 1. rows against the mirror --------------------------------------------------------------------------------------
@pytest.mark.parametrize("number", bh.BATCH_CASES)
def test_rows_against_the_mirror(models, number):
    case, rows, base, allow = bh.reference(number)
    gp = models(number)
    F, g, sum_alpha, alpha, info = engine_batch(gp, case, rows, want_alpha=number == 1)
    assert_array_equal(info, 0)
    grad = full_gradient(case, g, sum_alpha)
    Fc = gp.marginal_likelihood_batch(rows)
    Fg, gc = gp.marginal_likelihood_gradient_batch(rows)
    assert Fc.shape == (bh.N_ROWS,) and gc.shape == (bh.N_ROWS, gp.n_hyperpars)
    assert bits(Fc) == bits(F) and bits(Fg) == bits(F) and bits(gc) == bits(grad)  # the class adds nothing of its own
    for t in range(bh.N_ROWS):
        check(f"case {number} row {t} F", F[t], base[t]["F"][0], allow[t]["F"])
        check(f"case {number} row {t} gradient", grad[t], base[t]["grad"], allow[t]["grad"])
        if alpha is not None:
            check(f"case {number} row {t} alpha", alpha[t], base[t]["alpha"], allow[t]["alpha"])
    print(f"case {number}: largest error / allowance over the rows: F "
          f"{max(abs(F[t] - base[t]['F'][0]) / allow[t]['F'] for t in range(bh.N_ROWS)):.2e}, gradient "
          f"{max(np.abs(grad[t] - base[t]['grad']).max() / allow[t]['grad'] for t in range(bh.N_ROWS)):.2e}")
    # the single evaluation of row 0 agrees within the same allowances; whether it has the same bits is reported
    F1, g1 = gp.marginal_likelihood_gradient(rows[0])
    check(f"case {number} single F against row 0", F1, F[0], 2.0 * allow[0]["F"])
    check(f"case {number} single gradient against row 0", g1, grad[0], 2.0 * allow[0]["grad"])
    print(f"case {number}: row 0 bit-equal to the single evaluation: F {F1 == F[0]}, kernel gradient "
          f"{bits(g1[1:]) == bits(grad[0, 1:])}")


# ---- 2. bits ---------------------------------------------------------------------------------------------------------
def test_a_row_has_the_same_bits_wherever_it_is_evaluated(models):
    from inference_amd._engine import sgp_batch_schedule

    case, rows, _, _ = bh.reference(1)
    gp = models(1)
    n, d = case["x"].shape
    chunks = [sgp_batch_schedule(n, len(case["z"]), d, bh.N_ROWS, panel_rows=case["panel"], want_grad=True, max_chunk=k)["chunks"]
              for k in (0, 1, 3)]
    assert chunks == [1, 7, 3]

    def row3(out, at):
        F, g, sa, alpha, info = out
        assert info[at] == 0
        return bits(F[at]), bits(g[at]), bits(sa[at]), bits(alpha[at])

    want = row3(engine_batch(gp, case, rows[3:4], want_alpha=True), 0)
    assert row3(engine_batch(gp, case, rows[[3, 5]], want_alpha=True), 0) == want
    for k in (0, 1, 3):
        assert row3(engine_batch(gp, case, rows, want_alpha=True, max_chunk=k), 3) == want, f"max_chunk {k}"
    assert row3(engine_batch(gp, case, rows, want_alpha=True), 3) == want  # the call repeated
    assert row3(engine_batch(gp, case, rows[::-1], want_alpha=True), 3) == want  # (row 3 is its own mirror image)
    values_only = engine_batch(gp, case, rows, want_grad=False)
    assert values_only[1] is None and values_only[2] is None
    assert bits(values_only[0]) == bits(engine_batch(gp, case, rows)[0])


def test_a_batch_call_leaves_the_single_evaluations_and_the_fit_untouched(models):
    case, rows, _, _ = bh.reference(1)
    gp = bh.make_gp(case)
    theta = rows[4]
    mean0, std0 = gp(case["q"])
    F0, g0 = gp.marginal_likelihood_gradient(theta)
    v0 = gp.marginal_likelihood(theta)
    gp.marginal_likelihood_gradient_batch(rows)
    gp.marginal_likelihood_batch(rows[:2])
    mean1, std1 = gp(case["q"])
    v1 = gp.marginal_likelihood(theta)
    F1, g1 = gp.marginal_likelihood_gradient(theta)
    assert bits(mean0) == bits(mean1) and bits(std0) == bits(std1)
    assert v0 == v1 and F0 == F1 and bits(g0) == bits(g1)


# ---- 3. a failing row ------------------------------------------------------------------------------------------------
def test_a_failing_row_is_a_status_of_that_row_alone(models):
    case = sh.case(1)
    rows = bh.failure_rows(case)
    gp = models(1, jitter=0.0)
    at = bh.FAIL_POSITION
    others = [t for t in range(bh.FAIL_ROWS) if t != at]
    # the precondition, on the single evaluation: this row does fail, in the second pivot of K_mm
    th, white = gp._split(rows[at])
    assert gp.engine.bound(gp._kernel_id, th, white, 0.0, case["panel"])[3] == 2
    F, g, sa, alpha, info = engine_batch(gp, case, rows, want_alpha=True)
    assert_array_equal(info, [0, 0, 2, 0, 0])
    Fo, go, sao, alphao, infoo = engine_batch(gp, case, rows[others], want_alpha=True)
    assert_array_equal(infoo, 0)
    assert bits(F[others]) == bits(Fo) and bits(g[others]) == bits(go) and bits(sa[others]) == bits(sao)
    assert bits(alpha[others]) == bits(alphao)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        values = gp.marginal_likelihood_batch(rows)
    assert len(caught) == 1 and values[at] == -1e50 and bits(values[others]) == bits(Fo)
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_gradient_batch(rows)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        Fs, gs = gp.marginal_likelihood_gradient_batch(rows, failed="sentinel")
    assert len(caught) == 1 and Fs[at] == -1e50 and not gs[at].any()
    assert bits(Fs[others]) == bits(Fo) and bits(gs[others]) == bits(full_gradient(case, go, sao))
    # the next valid call is right
    again = engine_batch(gp, case, rows[others], want_alpha=True)
    assert bits(again[0]) == bits(Fo) and bits(again[1]) == bits(go) and bits(again[3]) == bits(alphao)


# ---- 4. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_object_usable(models):
    from inference_amd import _lib
    from inference_amd._engine import SparseEngine

    case, rows, _, _ = bh.reference(1)
    gp = models(1)
    eng = gp.engine
    th, white, mu = engine_args(case, rows[:3])
    good = engine_batch(gp, case, rows[:3])

    def still_right():
        out = engine_batch(gp, case, rows[:3])
        assert bits(out[0]) == bits(good[0]) and bits(out[1]) == bits(good[1])

    mus = np.repeat(mu[:, None], eng.n, axis=1)
    nan_theta = th.copy()
    nan_theta[1, 2] = np.nan
    for kwargs, theta, wv in ((dict(mu_const=mu, mus=mus), th, white), (dict(), th, white), (dict(mu_const=mu), nan_theta, white),
                              (dict(mu_const=mu), th, np.array([0.02, -1e-3, 0.02]))):
        with pytest.raises(_lib.GpmiError, match="status -1"):
            eng.bound_batch(gp._kernel_id, theta, wv, gp.jitter, case["panel"], **kwargs)
        still_right()
    # T < 0, through the library itself
    F, info = np.zeros(3), np.zeros(3, dtype=np.int32)
    rc = eng.h.lib.gpmi_sgp_bound_batch(eng.ptr, gp._kernel_id, -1, _lib.dptr(th), th.shape[1], _lib.dptr(white), _lib.dptr(mu), None,
                                        gp.jitter, case["panel"], 0, _lib.dptr(F), None, None, None,
                                        info.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == -1
    still_right()
    # before gpmi_sgp_set_observations
    fresh = SparseEngine(case["x"], case["z"])
    try:
        with pytest.raises(_lib.GpmiError, match="status -1"):
            fresh.bound_batch(gp._kernel_id, th, white, gp.jitter, case["panel"], mu_const=mu)
        fresh.set_observations(case["y"], bh.noise_var(case))
        out = fresh.bound_batch(gp._kernel_id, th, white, gp.jitter, case["panel"], mu_const=mu, want_grad=True)
        assert bits(out[0]) == bits(good[0]) and bits(out[1]) == bits(good[1])
    finally:
        fresh.close()
    # the class
    bad = rows[:3].copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        gp.marginal_likelihood_batch(bad)
    with pytest.raises(ValueError):
        gp.marginal_likelihood_gradient_batch(rows[:3, :-1])
    with pytest.raises(ValueError):
        gp.marginal_likelihood_gradient_batch(rows[:3], failed="skip")
    still_right()
    # T = 0
    empty = eng.bound_batch(gp._kernel_id, np.zeros((0, th.shape[1])), np.zeros(0), gp.jitter, case["panel"], mu_const=np.zeros(0),
                            want_grad=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, th.shape[1] + 1) and empty[4].shape == (0,)
    assert gp.marginal_likelihood_batch(np.zeros((0, gp.n_hyperpars))).shape == (0,)
    Fe, ge = gp.marginal_likelihood_gradient_batch(np.zeros((0, gp.n_hyperpars)))
    assert Fe.shape == (0,) and ge.shape == (0, gp.n_hyperpars)


# ---- 5. another mean function: the route of one mean vector per row ---------------------------------------------------
def test_linear_mean_rows_against_the_mirror():
    from inference_amd.gp import LinearMean

    case = sh.case(1)
    d = case["x"].shape[1]
    rng = default_rng(41)
    base_rows = bh.row_set(case)[:4]
    rows = np.array([np.concatenate([[r[0]], rng.uniform(-0.3, 0.3, size=d), r[1:]]) for r in base_rows])
    gp = bh.make_gp(case, mean=LinearMean, hyperpars=rows[0])
    F, grad = gp.marginal_likelihood_gradient_batch(rows)
    values = gp.marginal_likelihood_batch(rows)
    assert bits(values) == bits(F)
    centred = case["x"] - case["x"].mean(axis=0)
    features = [np.ones(len(centred))] + list(centred.T)
    for t, row in enumerate(rows):
        mu = row[0] + centred @ row[1:1 + d]
        with bh.one_blas_thread():
            ref, allow = bh.reference_row(case, row, sh.N_RIPPLES, 500000 + 1000 * t, mean_vector=mu, mean_features=features)
        check(f"LinearMean row {t} F", F[t], ref["F"][0], allow["F"])
        check(f"LinearMean row {t} gradient", grad[t], ref["grad"], allow["grad"])


# ---- 6. the lockstep drivers on a sparse model -----------------------------------------------------------------------
def box(gp):
    return np.array([b[0] for b in gp.hp_bounds], dtype=float), np.array([b[1] for b in gp.hp_bounds], dtype=float)


@pytest.fixture(scope="module")
def driven():
    """Case 1 (N = 300, m = 33) with batch-independent single evaluations: what a sampler advanced alone calls."""
    gp = bh.make_gp(sh.case(1))
    gp.batch_independent_values(True)
    return gp, sh.full_theta(sh.case(1))


def test_ensembles_in_lockstep_are_the_samplers_advanced_alone(driven):
    from inference_amd.mcmc import EnsembleSampler, advance_lockstep_ensembles

    gp, start = driven
    lower, upper = box(gp)

    def samplers():
        out = []
        for k, update in enumerate(("serial", "split")):
            u = default_rng(9100 + k).random((2 * start.size + 2, start.size))
            walkers = np.clip(start + 0.1 * (2.0 * u - 1.0), lower + 1e-3, upper - 1e-3)
            out.append(EnsembleSampler(gp.marginal_likelihood, walkers, bounds=(lower, upper), display_progress=False,
                                       update=update, seed=310 + k))
        return out

    alone, together = samplers(), samplers()
    for s in alone:
        s.advance(3)
    rows = advance_lockstep_ensembles(together, 3, gp.marginal_likelihood_batch)
    assert rows == sum(np.array(s.total_proposals).sum() for s in together)
    for k, (a, b) in enumerate(zip(alone, together)):
        sa, sb = eh.state(a), eh.state(b)
        for key in eh.STATE_KEYS:
            assert_array_equal(sa[key], sb[key], err_msg=f"sampler {k} {key}")


def test_hmc_chains_in_lockstep_are_the_chains_advanced_alone(driven):
    from inference_amd.mcmc import HamiltonianChain, advance_lockstep_hmc

    gp, start = driven

    def chains():
        out = []
        for k, T in enumerate((1.0, 1.0, 2.0, 4.0)):
            ch = HamiltonianChain(gp.marginal_likelihood, start, grad=lambda t: gp.marginal_likelihood_gradient(t)[1],
                                  epsilon=0.02, temperature=T, bounds=box(gp), display_progress=False)
            ch.rng = default_rng(520 + k)
            ch.steps = 6
            out.append(ch)
        return out

    alone, together = chains(), chains()
    for ch in alone:
        for _ in range(3):
            ch.take_step()
    advance_lockstep_hmc(together, 3, gp.marginal_likelihood_gradient_batch)
    for a, b in zip(alone, together):
        sa, sb = hh.state(a), hh.state(b)
        for key in sa:
            assert_array_equal(sa[key], sb[key], err_msg=key)


def test_parallel_tempering_of_gibbs_chains_on_a_sparse_model(driven):
    import random

    from inference_amd.mcmc import GibbsChain, ParallelTempering

    gp, start = driven

    def ladder(lockstep):
        chains = []
        for k, T in enumerate((1.0, 3.0)):
            ch = GibbsChain(posterior=gp.marginal_likelihood, start=start, widths=[0.05] * start.size, temperature=T,
                            display_progress=False)
            for i, b in enumerate(gp.hp_bounds):
                ch.set_boundaries(i, b)
            ch.rng = default_rng(7000 + 10 * k)
            for i, par in enumerate(ch.params):
                par.rng = default_rng(7000 + 10 * k + 1 + i)
            chains.append(ch)
        pt = ParallelTempering(chains)
        assert pt.batch_posterior == gp.marginal_likelihood_batch  # found by name: no driver knows the sparse model
        if not lockstep:
            pt.batch_posterior = None  # the chains stepped one by one, each through a batch of one
        pt.rng = default_rng(23)
        return pt

    sequential, lockstep = ladder(False), ladder(True)
    random.seed(4)
    sequential.advance(4, swap_interval=2)
    random.seed(4)
    lockstep.advance(4, swap_interval=2)
    assert lockstep.posterior_evaluations > 0 and sequential.posterior_evaluations == 0
    for a, b in zip(sequential.chains, lockstep.chains):
        assert_array_equal(np.array(a.probs), np.array(b.probs))
        for pa, pb in zip(a.params, b.params):
            assert_array_equal(np.array(pa.samples), np.array(pb.samples))
    assert_array_equal(sequential.successful_swaps, lockstep.successful_swaps)


# ---- 7. the search ---------------------------------------------------------------------------------------------------
def mirror_search(case, gp, starts, ripple):
    """The one-after-another search of `multistart_bfgs` on the mirror: the bounds F* of every start."""
    from scipy.optimize import fmin_l_bfgs_b

    mir = sh.SparseMirror(case["kind"], case["x"], case["z"], jitter=gp.jitter, ripple=ripple)

    def cost(theta):
        try:
            F, g, alpha = mir.bound_and_gradient(theta[1:-1], float(np.exp(2.0 * theta[-1])), case["y"] - theta[0], bh.noise_var(case))
        except LinAlgError:
            return 1e50, np.zeros(theta.size)
        return -F, -np.concatenate([[alpha.sum()], g])

    return np.array([-fmin_l_bfgs_b(func=cost, x0=x0, approx_grad=False, bounds=gp.hp_bounds)[1] for x0 in starts])


def test_lockstep_search():
    """The margin between the lockstep and the one-after-another search on the device is measured on the mirror: the
    search is path-sensitive, so the one-after-another search runs there twice, with and without a 1e-13 ripple, and ten
    times the largest difference of their F* is allowed (floored at 1e-10 of |F*|, as every allowance here)."""
    case = sh.case(1)
    gp = bh.make_gp(case)
    np.random.seed(5)
    best = gp.multistart_bfgs(starts=3, lockstep=True)
    log = gp.search_log
    starts = [x0 for x0, _, _ in log]
    F_lock = np.array([-f for _, _, f in log])
    assert len(log) == 3 and all(x.shape == (gp.n_hyperpars,) and t.shape == (gp.n_hyperpars,) for x, t, _ in log)
    assert np.array_equal(best, log[int(np.argmax(F_lock))][1])
    np.random.seed(5)
    gp.multistart_bfgs(starts=3)
    assert all(np.array_equal(x0, s0) for (x0, _, _), s0 in zip(gp.search_log, starts))
    F_seq = np.array([-f for _, _, f in gp.search_log])
    with bh.one_blas_thread():
        F_plain, F_rippled = mirror_search(case, gp, starts, None), mirror_search(case, gp, starts, sh.rippler(77))
    allow = max(10.0 * float(np.abs(F_plain - F_rippled).max()), 1e-10 * float(np.abs(F_plain).max()))
    print(f"search: F* lockstep {F_lock}, one after another {F_seq}, mirror {F_plain}; mirror against rippled mirror "
          f"{np.abs(F_plain - F_rippled).max():.3e}")
    check("search F*, lockstep against one after another", F_lock, F_seq, allow)
    np.random.seed(5)
    searched = bh.make_gp(case, hyperpars=None, n_starts=3, lockstep_search=True)
    assert np.array_equal(searched.hyperpars, best)
