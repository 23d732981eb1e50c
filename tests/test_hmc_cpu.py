"""
CPU tests of HamiltonianChain, its masses, step-size selector and Bounds against traces of the reference
(tests/golden/hmc.npz, written by golden/make_golden_hmc.py from the seeded recipes of tests/hmc_host.py), and of the
lockstep driver `advance_lockstep_hmc` against the chains stepped alone.  The maker asserted that no accept test, number of
leapfrog steps or epsilon review of a trace sits on a rounding error, so the integer logs are compared exactly.
"""
import random
import warnings

import numpy as np
import pytest
from numpy.random import default_rng
from numpy.testing import assert_allclose, assert_array_equal

import hmc_host as hh
from inference_amd.mcmc import (Bounds, GibbsChain, HamiltonianChain, ParallelTempering, advance_ladders,
                                advance_lockstep_hmc)
from inference_amd.mcmc.hmc import MatrixMass, ScalarMass, VectorMass, get_particle_mass


@pytest.fixture(scope="module")
def g(golden):
    return golden("hmc")


def same_state(a, b):
    sa, sb = hh.state(a), hh.state(b)
    for key in sa:
        assert_array_equal(sa[key], sb[key], err_msg=key)


@pytest.mark.parametrize("name", list(hh.CASES))
def test_reference_traces(g, name):
    chain = hh.build(HamiltonianChain, name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        chain.advance(hh.CASES[name][1])
    got = hh.state(chain)
    assert_allclose(got["theta"], g[f"{name}_theta"], rtol=0, atol=1e-9)
    assert_allclose(got["probs"], g[f"{name}_probs"], rtol=1e-10)
    assert_array_equal(got["leapfrog_steps"], g[f"{name}_leapfrog_steps"])
    assert_array_equal(got["epsilon_checks"], g[f"{name}_epsilon_checks"])
    assert_allclose(got["epsilon_values"], g[f"{name}_epsilon_values"], rtol=1e-12)
    assert chain.chain_length == got["theta"].shape[0] == hh.CASES[name][1] + 1
    assert chain.estimate_burn_in() == int(g[f"{name}_burn"])
    assert_array_equal(chain.mode(), g[f"{name}_mode"])


def test_attributes():
    chain = HamiltonianChain(hh.posterior, hh.START, grad=hh.gradient, temperature=4.0, display_progress=False)
    assert (chain.steps, chain.max_attempts, chain.inv_temp, chain.temperature) == (50, 200, 0.25, 4.0)
    assert chain.n_parameters == 3 and chain.chain_length == 1 and chain.leapfrog_steps == [0] and chain.bounds is None
    assert isinstance(chain.mass, ScalarMass) and chain.mass.inv_mass == 1.0
    assert chain.probs == [hh.posterior(hh.START) * 0.25]
    es = chain.ES
    assert (es.epsilon, es.accept_rate, es.chk_int, es.growth_factor) == (0.1, 0.65, 15, 1.4)
    assert es.epsilon_values == [0.1] and es.epsilon_checks == [0.0]
    r = np.array([0.3, -1.0, 2.0])
    assert chain.kinetic_energy(r) == 0.5 * (r @ r)
    assert chain.hamiltonian(hh.START, r) == 0.5 * (r @ r) - hh.posterior(hh.START) * 0.25
    bounded = HamiltonianChain(hh.posterior, hh.START, grad=hh.gradient, bounds=Bounds(hh.LOWER, hh.UPPER))
    assert bounded.run_leapfrog == bounded.bounded_leapfrog and chain.run_leapfrog == chain.standard_leapfrog
    # the finite-difference gradient is that of the TEMPERED posterior (and the leapfrog tempers it again)
    assert_allclose(HamiltonianChain(hh.posterior, hh.START, temperature=4.0).grad(hh.START), 0.25 * hh.gradient(hh.START),
                    rtol=1e-4)


def test_bounds(g):
    bounds = Bounds(lower=hh.LOWER, upper=hh.UPPER)
    assert_array_equal(bounds.width, hh.UPPER - hh.LOWER)
    assert bounds.n_bounds == 3
    for k, p in enumerate(g["bounds_points"]):
        assert_array_equal(bounds.reflect(p), g["bounds_reflect"][k])
        t, reflections = bounds.reflect_momenta(p)
        assert_array_equal(t, g["bounds_reflect_momenta"][k])
        assert_array_equal(reflections, g["bounds_reflections"][k])
        assert bounds.inside(t) and bounds.inside(p) == bool(((p >= hh.LOWER) & (p <= hh.UPPER)).all())
    assert_array_equal(Bounds([0.0, 1.0], [[2.0, 3.0]]).lower, [0.0, 1.0])  # sequences are squeezed
    with pytest.raises(ValueError, match="one-dimensional"):
        Bounds(np.zeros((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match="equal size"):
        Bounds(np.zeros(2), np.ones(3))
    with pytest.raises(ValueError, match="larger than the corresponding lower"):
        Bounds(np.zeros(2), np.array([1.0, 0.0]))
    with pytest.raises(ValueError, match=r"\[ Sampler error \]"):
        Bounds(np.zeros(2), np.zeros(2), error_source="Sampler")
    with pytest.raises(ValueError, match="number of bounds"):
        bounds.validate_start_point(np.zeros(2))
    with pytest.raises(ValueError, match="outside specified bounds"):
        bounds.validate_start_point(np.array([0.0, 0.0, 7.0]))
    bounds.validate_start_point(hh.START)


def test_masses(g):
    for name, inverse_mass, kind in (("scalar", 0.25, ScalarMass), ("vector", hh.S ** 2, VectorMass), ("matrix", hh.FULL, MatrixMass)):
        mass = get_particle_mass(inverse_mass, 3)
        assert type(mass) is kind
        draws = default_rng(hh.SEED + 2)
        momenta = np.array([mass.sample_momentum(draws) for _ in range(4)])
        assert_allclose(momenta, g[f"momentum_{name}"], rtol=1e-13)
        assert_allclose([mass.get_velocity(r) for r in g[f"momentum_{name}"]], g[f"velocity_{name}"], rtol=1e-13)
    assert type(get_particle_mass(2, 3)) is ScalarMass
    with pytest.raises(TypeError, match="numpy.ndarray"):
        get_particle_mass([1.0, 1.0, 1.0], 3)
    with pytest.raises(AssertionError):  # the wrong size trips the assertion, not the ValueError
        get_particle_mass(np.ones(4), 3)
    with pytest.raises(ValueError, match="only positive values"):
        get_particle_mass(np.array([1.0, 0.0, 1.0]), 3)
    with pytest.raises(ValueError, match="valid covariance matrix"):
        get_particle_mass(np.array([[1.0, 0.5], [0.2, 1.0]]), 2)
    with pytest.raises(ValueError, match="valid covariance matrix"):
        get_particle_mass(np.ones((2, 3)), 2)
    with pytest.raises(ValueError, match="do not match"):
        get_particle_mass(np.eye(2), 3)


def test_readouts(g):
    chain = hh.rebuilt_chain(g)
    assert chain.chain_length == hh.LONG + 1
    assert chain.estimate_burn_in() == int(g["long_burn"])
    assert_array_equal(chain.mode(), g["long_mode"])
    assert_array_equal(chain.get_parameter(1, burn=10, thin=3), g["long_parameter"])
    assert_array_equal(chain.get_probabilities(burn=10, thin=3), g["long_probabilities"])
    assert_array_equal(chain.get_sample(burn=10, thin=3), g["long_sample"])
    sample, probs = chain.get_interval(interval=0.9, burn=200, thin=2)
    assert_array_equal(sample, g["long_interval_sample"])
    assert_array_equal(probs, g["long_interval_probs"])
    chain.estimate_mass(burn=200, thin=2, diagonal=True)
    assert type(chain.mass) is VectorMass
    assert_allclose(chain.mass.inv_mass, g["long_mass_diagonal"], rtol=1e-13)
    chain.estimate_mass(burn=200, thin=2, diagonal=False)
    assert type(chain.mass) is MatrixMass
    assert_allclose(chain.mass.inv_mass, g["long_mass_full"], rtol=1e-13)
    # the burn-in estimate is capped at 0.9 of the length
    chain.ES.epsilon_checks[-2] = 1e9
    chain.ES.epsilon_values[-2] = 10 * chain.ES.epsilon
    assert chain.estimate_burn_in() == int(0.9 * chain.chain_length)
    assert chain.get_last() is chain.theta[-1]
    new = np.zeros(3)
    chain.replace_last(new)
    assert chain.theta[-1] is new
    with pytest.raises(NotImplementedError, match="UnimodalPdf"):
        chain.get_marginal(0, unimodal=True)
    with pytest.raises(ValueError, match="burn"):
        chain.matrix_plot(burn=hh.LONG)
    with pytest.raises(ValueError, match="no samples"):
        hh.build(HamiltonianChain).trace_plot()


def five_chains():
    """The three masses, two temperatures, bounded and not."""
    both = (hh.LOWER, hh.UPPER)
    recipes = [dict(epsilon=0.2), dict(inverse_mass=hh.S ** 2, temperature=2.5, bounds=both), dict(inverse_mass=hh.FULL),
               dict(inverse_mass=hh.FULL, temperature=2.5, bounds=both, epsilon=0.3), dict(inverse_mass=0.5, bounds=both)]
    return [hh.build(HamiltonianChain, seed=40 + k, **kw) for k, kw in enumerate(recipes)]


def test_lockstep_is_the_chains_run_alone():
    alone, together = five_chains(), five_chains()
    calls = []

    def batch(thetas):
        calls.append(len(thetas))
        return hh.batch(thetas)

    for ch in alone:
        ch.advance(25)
    evals = advance_lockstep_hmc(together, 25, batch)
    assert evals == sum(calls) == sum(sum(ch.leapfrog_steps) for ch in together) + 5
    assert max(calls) == 5 and calls[0] == 5
    for a, b in zip(alone, together):
        same_state(a, b)
    # a replaced last sample (what a swap does): that chain alone asks for its start again
    moved = np.array([0.5, 1.0, 1.0])
    for ch in (alone[2], together[2]):
        ch.replace_last(moved.copy())
        ch.probs[-1] = hh.posterior(moved) * ch.inv_temp
    before = sum(sum(ch.leapfrog_steps) for ch in together)
    for ch in alone:
        ch.advance(15)
    del calls[:]
    evals = advance_lockstep_hmc(together, 15, batch, max_batch=2)
    assert evals == sum(calls) == sum(sum(ch.leapfrog_steps) for ch in together) - before + 1
    assert max(calls) == 2
    for a, b in zip(alone, together):
        same_state(a, b)
        assert a.rng.random() == b.rng.random()  # the generators have been consumed identically
    assert all(ch.chain_length == 41 for ch in together)
    assert advance_lockstep_hmc(together, 0, batch) == 0 and advance_lockstep_hmc([], 3, batch) == 0


def hmc_ladder(batch):
    chains = [hh.build(HamiltonianChain, seed=300 + k, temperature=T, epsilon=0.2, bounds=(hh.LOWER, hh.UPPER))
              for k, T in enumerate((1.0, 2.0, 4.0, 8.0))]
    ladder = ParallelTempering(chains, batch_value_and_grad=batch)
    ladder.rng = default_rng(17)
    return ladder


def test_parallel_tempering_of_hmc_chains():
    sequential, lockstep = hmc_ladder(None), hmc_ladder(hh.batch)
    assert sequential.batch_posterior is None and sequential.batch_value_and_grad is None
    random.seed(3)
    sequential.advance(12, swap_interval=3)
    random.seed(3)
    lockstep.advance(12, swap_interval=3)
    assert sequential.successful_swaps.sum() >= 1
    assert sequential.posterior_evaluations == 0
    # one row per leapfrog step, one per chain at the start, and one for each chain of a successful swap
    steps = sum(sum(ch.leapfrog_steps) for ch in lockstep.chains)
    swapped_before_the_last_interval = lockstep.posterior_evaluations - steps - 4
    assert 0 <= swapped_before_the_last_interval <= 2 * sequential.successful_swaps.sum()
    for a, b in zip(sequential.chains, lockstep.chains):
        same_state(a, b)
    assert_array_equal(sequential.successful_swaps, lockstep.successful_swaps)
    assert_array_equal(sequential.attempted_swaps, lockstep.attempted_swaps)
    assert sequential.rng.random() == lockstep.rng.random()


def test_validation():
    with pytest.raises(ValueError, match="not a callable"):
        HamiltonianChain(posterior=3.0, start=np.zeros(2))
    with pytest.raises(ValueError, match="float"):
        HamiltonianChain(posterior=lambda t: 1, start=np.zeros(2))
    with pytest.raises(ValueError, match="finite"):
        HamiltonianChain(posterior=lambda t: float("nan"), start=np.zeros(2))
    with pytest.raises(ValueError, match=r"HamiltonianChain error[\s\S]*outside specified bounds"):
        HamiltonianChain(hh.posterior, np.array([0.0, 0.0, 7.0]), grad=hh.gradient, bounds=(hh.LOWER, hh.UPPER))
    with pytest.raises(TypeError):
        HamiltonianChain(hh.posterior, hh.START, grad=hh.gradient, inverse_mass=[1.0, 1.0, 1.0])
    chain = hh.build(HamiltonianChain, "scalar")
    chain.max_attempts = 0
    with pytest.raises(ValueError, match="maximum allowed attempts of 0"):
        chain.take_step()
    with pytest.raises(ValueError, match="maximum allowed attempts of 0"):
        advance_lockstep_hmc([chain], 1, hh.batch)
    assert chain.chain_length == 1
    with pytest.raises(TypeError, match="take_step"):
        advance_lockstep_hmc([hh.build(HamiltonianChain, "scalar"), hh.build(HamiltonianChain, "fdiff")], 1, hh.batch)
    ladder = ParallelTempering([hh.build(HamiltonianChain, "scalar"), hh.build(HamiltonianChain, temperature=2.0)])
    with pytest.raises(TypeError, match="advance_lockstep_hmc"):
        advance_ladders([ladder], 2, batch_posterior=lambda th: np.zeros(len(th)))


def test_a_failed_row_is_a_rejected_attempt():
    """The sentinel of `marginal_likelihood_gradient_batch(failed="sentinel")`, -1e50 and a zero gradient, at the end of a
    trajectory: acceptance probability 0, the attempt is retried."""
    chain = hh.build(HamiltonianChain, "scalar")
    first = hh.build(HamiltonianChain, "scalar")._draw_attempt()[1]  # leapfrog steps of the first trajectory
    calls = []

    def batch(thetas):
        calls.append(len(thetas))
        if len(calls) == 1 + first:  # (one row for the start, then one per step) the last position of that trajectory
            return np.full(1, -1e50), np.zeros((1, 3))
        return hh.batch(thetas)

    advance_lockstep_hmc([chain], 1, batch)
    assert chain.chain_length == 2 and chain.leapfrog_steps[1] > first and np.isfinite(chain.probs[1])
    assert sum(calls) == chain.leapfrog_steps[1] + 1


def test_gibbs_chain_still_reads_out_through_the_shared_base():
    chain = GibbsChain(hh.posterior, hh.START, display_progress=False)
    assert GibbsChain.get_interval is HamiltonianChain.get_interval
    with pytest.raises(NotImplementedError, match="UnimodalPdf"):
        chain.get_marginal(0, unimodal=True)


def test_a_batched_lml_alone_does_not_drive_hmc_chains():
    """`ParallelTempering` detects `GpRegressor.marginal_likelihood` posteriors for the Gibbs driver; chains that need
    gradients are stepped one by one unless `batch_value_and_grad` is given."""
    class Model:
        def marginal_likelihood(self, t):
            return hh.posterior(t)

        def marginal_likelihood_batch(self, thetas):
            raise AssertionError("the Gibbs driver was used for HMC chains")

    model = Model()
    chains = [hh.build(HamiltonianChain, seed=60 + k, temperature=T, posterior=model.marginal_likelihood)
              for k, T in enumerate((1.0, 2.0))]
    ladder = ParallelTempering(chains)
    assert ladder.batch_posterior is None and ladder.batch_value_and_grad is None
    ladder.take_steps(2)
    assert [ch.chain_length for ch in chains] == [3, 3] and ladder.posterior_evaluations == 0
    gibbs = [GibbsChain(model.marginal_likelihood, hh.START, display_progress=False) for _ in range(2)]
    assert ParallelTempering(gibbs).batch_posterior == model.marginal_likelihood_batch
