"""GPU tests of EnsembleSampler on the batched device likelihood (`GpRegressor.marginal_likelihood_batch`): the lockstep
driver against the samplers advanced alone (bit for bit), both modes against the same seeded sampler on the CPU oracle,
the effective sample sizes of `diagnostics_data`, and a proposal whose covariance does not factorise.

Two models, those of test_hmc_gpu.py: the N = 48 problem of test_mcmc_cpu.pt_problem (SE, P = 3) and SE + WhiteNoise on
N = 200, d = 2 (P = 5).  The walkers start scattered around the model's start vector and are bounded by its `hp_bounds`;
P = 3 has 8 walkers and P = 5 has 12, the fewest that split mode takes."""
import warnings

import numpy as np
import pytest
from numpy.random import default_rng
from numpy.testing import assert_allclose, assert_array_equal

import ensemble_host as eh
import workloads as wl
from test_mcmc_cpu import pt_problem

pytestmark = pytest.mark.gpu

MODELS = ["pt48", "wn200"]
WALKERS = {"pt48": 8, "wn200": 12}
# seeds of the oracle comparison, chosen on the CPU oracle alone so that the margins asserted there hold
ORACLE_SEEDS = {("pt48", "serial"): 41, ("pt48", "split"): 42, ("wn200", "serial"): 43, ("wn200", "split"): 44}
ORACLE_ITERATIONS = 5


def model_data(name):
    """(x, y, y_err, start, white_noise) of a model."""
    if name == "pt48":
        x, y, e, start, _ = pt_problem()
        return x, y, e, start, False
    x, y, e = wl.synthetic_dataset(7, 200, 2)
    start = np.array([y.mean(), np.log(y.std()), np.log(0.5), np.log(0.5), np.log(0.1)])
    return x, y, e, start, True


def device_model(name):
    from inference_amd import gp as gp_mod

    x, y, e, start, white_noise = model_data(name)
    kernel = gp_mod.SquaredExponential() + gp_mod.WhiteNoise() if white_noise else gp_mod.SquaredExponential
    return gp_mod.GpRegressor(x, y, y_err=e, hyperpars=start, kernel=kernel), start


def oracle_model(name):
    from oracle import gp_oracle as orc

    x, y, e, start, white_noise = model_data(name)
    return orc.OracleGp(x, y, e, kernel=orc.SE, white_noise=white_noise), start


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = device_model(name)
            cache[name][0].batch_independent_values(True)
        return cache[name]

    return get


def box(hp_bounds):
    return np.array([b[0] for b in hp_bounds], dtype=float), np.array([b[1] for b in hp_bounds], dtype=float)


def scattered(name, start, hp_bounds, seed):
    """The walkers' starting positions: within 0.15 of the start vector in every parameter, inside the bounds."""
    lower, upper = box(hp_bounds)
    u = default_rng(seed).random((WALKERS[name], start.size))
    return np.clip(start + 0.15 * (2.0 * u - 1.0), lower + 1e-3, upper - 1e-3)


def make_sampler(name, start, hp_bounds, update, seed, posterior=None, batch_posterior=None):
    from inference_amd.mcmc import EnsembleSampler

    return EnsembleSampler(posterior, scattered(name, start, hp_bounds, 9000 + seed), bounds=box(hp_bounds),
                           display_progress=False, update=update, batch_posterior=batch_posterior, seed=seed)


def same_state(a, b, what=""):
    sa, sb = eh.state(a), eh.state(b)
    for key in eh.STATE_KEYS:
        assert_array_equal(sa[key], sb[key], err_msg=f"{what} {key}")


@pytest.mark.parametrize("name", MODELS)
def test_ensemble_lockstep_is_the_samplers_advanced_alone(models, name):
    from inference_amd.mcmc import advance_lockstep_ensembles

    gp, start = models(name)

    def posterior(t):  # the sampler's own evaluations: a batch of one
        return float(gp.marginal_likelihood_batch(t[None, :])[0])

    def samplers():
        return [make_sampler(name, start, gp.hp_bounds, update, 300 + k, posterior=posterior)
                for k, update in enumerate(("serial", "split", "serial", "split"))]

    alone, together = samplers(), samplers()
    for s in alone:
        s.advance(5)
    rows = advance_lockstep_ensembles(together, 5, gp.marginal_likelihood_batch)
    assert rows == sum(np.array(s.total_proposals).sum() for s in together)
    for k, (a, b) in enumerate(zip(alone, together)):
        same_state(a, b, f"sampler {k}")
        assert b.n_iterations == 5 and b.chain_length == 5 * WALKERS[name]
    print(f"{name}: {rows} rows for {4 * 5 * WALKERS[name]} updates")


def oracle_run(name, update):
    """The seeded sampler of the comparison on the CPU oracle, advanced, and the recorder of its accept tests."""
    ref, start = oracle_model(name)
    sampler = make_sampler(name, start, ref.hp_bounds, update, ORACLE_SEEDS[name, update], posterior=ref.marginal_likelihood)
    rec = eh.Recorder(sampler)
    sampler.advance(ORACLE_ITERATIONS)
    return ref, sampler, rec


@pytest.mark.parametrize("update", ["serial", "split"])
@pytest.mark.parametrize("name", MODELS)
def test_ensemble_on_device_follows_the_cpu_oracle(models, name, update):
    """A position depends on the posterior only through the accept decisions: where every decision agrees, the device run
    has the oracle run's positions bit for bit, and its log-probabilities within the project's 1e-10.  The oracle run is
    first shown to have no decision that 1e-10 could turn: every accept test with q < 1 + 1e-6 keeps |u - q| >= 1e-6 and
    every |p| is at most 1e3, so that a relative 1e-10 on p and on walker_probs[i] moves q by at most 2e-7 q."""
    gp, start = models(name)
    ref, exact, rec = oracle_run(name, update)
    assert_allclose(np.array(gp.hp_bounds), np.array(ref.hp_bounds), rtol=1e-12)
    margin, largest = rec.margins()
    assert len(rec.tests) == np.array(exact.total_proposals).sum()
    assert margin >= 1e-6 and largest <= 1e3, (margin, largest)  # (else: pick another seed, on the CPU)
    device = make_sampler(name, start, gp.hp_bounds, update, ORACLE_SEEDS[name, update],
                          batch_posterior=gp.marginal_likelihood_batch)
    device.advance(ORACLE_ITERATIONS)
    got, want = eh.state(device), eh.state(exact)
    error = np.abs(got["sample_probs"] / want["sample_probs"] - 1.0).max()
    print(f"{name} {update}: {len(rec.tests)} accept tests, margin {margin:.1e}, max |p| {largest:.3g}, "
          f"sample_probs device vs oracle {error:.1e}")
    for key in ("total_proposals", "failed_updates", "walker_positions", "sample"):
        assert_array_equal(got[key], want[key], err_msg=key)
    assert_allclose(got["sample_probs"], want["sample_probs"], rtol=1e-10)
    assert_allclose(got["walker_probs"], want["walker_probs"], rtol=1e-10)


def test_ensemble_diagnostics_ess_is_one_batch_call():
    from inference_amd.mcmc import EnsembleSampler, effective_sample_size_batch

    sampler = EnsembleSampler(eh.post_b, eh.starts("b"), display_progress=False, seed=5)
    sampler.advance(256)
    series = sampler.sample.reshape(256, 8 * 3)
    data = sampler.diagnostics_data(ess=True)
    assert data["ess"].shape == (8, 3) and data["ess"].dtype == np.int64
    assert_array_equal(data["ess"], effective_sample_size_batch(series).reshape(8, 3))
    assert_array_equal(sampler.diagnostics_data(burn=16, ess=True)["ess"],
                       effective_sample_size_batch(series[16:]).reshape(8, 3))
    assert (data["ess"] >= 1).all() and (data["ess"] <= 256).all()
    assert_array_equal(data["acceptance_rates"], sampler.diagnostics_data()["acceptance_rates"])


@pytest.mark.parametrize("update", ["serial", "split"])
def test_ensemble_retries_a_proposal_that_does_not_factorise(models, update):
    gp, start = models("pt48")
    sampler = make_sampler("pt48", start, gp.hp_bounds, update, 77, batch_posterior=gp.marginal_likelihood_batch)
    calls, seen = [0], []

    def batch(rows):
        """The device batch; the first row of the first call is given an amplitude of exp(800), which overflows."""
        calls[0] += 1
        if calls[0] == 1:
            rows = rows.copy()
            rows[0, 1] = 800.0
        values = gp.marginal_likelihood_batch(rows)
        if calls[0] == 1:
            seen.append(values[0])
        return values

    sampler.batch_posterior = batch
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sampler.advance(3)
    assert seen == [-1e50]
    assert len([w for w in caught if "Cholesky decomposition failure" in str(w.message)]) == 1
    assert sampler.total_proposals[0][0] >= 2  # walker 0: the failed row was rejected, and the walker tried again
    assert sampler.n_iterations == 3 and sum(sampler.failed_updates) == 0
    assert np.isfinite(sampler.sample).all() and (np.abs(sampler.sample_probs) < 1e3).all()
    assert calls[0] == np.array(sampler.total_proposals).sum() if update == "serial" else calls[0] >= 6
