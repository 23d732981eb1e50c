"""
CPU tests of PcaChain against traces of the reference (tests/golden/pca.npz, written by golden/make_golden_pca.py from the
seeded recipes of tests/pca_host.py), with the covariance of the direction updates taken on the host
(`covariance=lambda s: numpy.cov(s.T)`, what the reference computes), and of the lockstep drivers against the chains stepped
alone.  The maker asserted that no accept test, width review or direction of a trace sits on a rounding error; the
arithmetic is the reference's, operation for operation, so everything is compared bit for bit.
"""
import random
import warnings

import numpy as np
import pytest
from numpy.random import default_rng
from numpy.testing import assert_array_equal

import pca_host as ph
from inference_amd.mcmc import Bounds, GibbsChain, ParallelTempering, PcaChain, advance_ladders, advance_lockstep


@pytest.fixture(scope="module")
def g(golden):
    return golden("pca")


def build(name, **kwargs):
    return ph.build(PcaChain, name, covariance=ph.numpy_covariance, **kwargs)


def same_state(a, b):
    sa, sb = ph.state(a), ph.state(b)
    assert sa.keys() == sb.keys()
    for key in sa:
        assert_array_equal(sa[key], sb[key], err_msg=key)


@pytest.mark.parametrize("name", list(ph.CASES))
def test_reference_traces(g, name):
    chain = build(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        chain.advance(ph.STEPS)
    assert chain.chain_length == ph.STEPS + 1
    got = ph.state(chain)
    for key, value in got.items():
        assert_array_equal(value, g[f"{name}_{key}"], err_msg=key)
    assert list(chain.update_history) == ph.UPDATES
    assert (chain.last_update, chain.dir_update_interval, chain.next_update) == (250, 225, 475)
    assert chain.estimate_burn_in() == int(g[f"{name}_burn"])
    assert_array_equal(chain.mode(), g[f"{name}_mode"])


def test_attributes():
    chain = PcaChain(ph.POSTERIOR3, np.array([1.5, 0.0, 3.0]), temperature=4.0, display_progress=False)
    assert chain.inv_temp == 0.25 and chain.n_parameters == 3 and chain.chain_length == 1 and chain.bounds is None
    assert [p.target_rate for p in chain.params] == [0.5] * 3
    assert [p.sigma for p in chain.params] == [1.5 * 0.05, 1.0, 3.0 * 0.05]
    assert_array_equal(np.array(chain.directions), np.eye(3))
    assert (chain.dir_update_interval, chain.dir_growth_factor, chain.last_update, chain.next_update) == (100, 1.5, 0, 100)
    assert chain.angles_history == [] and chain.update_history == [] and chain.covar is None
    assert chain.probs == [ph.POSTERIOR3(np.array([1.5, 0.0, 3.0])) * 0.25]
    assert isinstance(chain, GibbsChain)


def test_only_the_chains_generator_is_used():
    """One normal per proposal and one uniform per proposal that is not better; `Parameter.proposal` is never called."""
    chain = build("plain")
    rec = ph.Recorder(chain)
    for p in chain.params:
        p.proposal = None
        p.rng = None
    rec.run(20)
    kinds = [k for k, _ in rec.events]
    assert kinds.count("normal") == kinds.count("accept_prob") == rec.proposals[-1]
    better = sum(1 for k, v in rec.events if k == "accept_prob" and v == 1.0)
    assert kinds.count("uniform") == rec.proposals[-1] - better
    assert all(p.try_count == 0 for p in chain.params)


def lockstep_set():
    """Three PcaChains (one bounded and tempered) and a GibbsChain on the same posterior."""
    chains = [build("plain"), build("bounded"), build("plain", seed=21)]
    gibbs = GibbsChain(ph.POSTERIOR3, np.array([1.5, 0.0, 3.0]), widths=[0.5, 0.3, 1.0], display_progress=False)
    gibbs.rng = default_rng(31)
    for k, p in enumerate(gibbs.params):
        p.rng = default_rng(40 + k)
    return chains + [gibbs]


def test_lockstep_equals_the_chains_alone():
    alone, together = lockstep_set(), lockstep_set()
    for chain in alone:
        chain.advance(120)
    sizes = []

    def batch(thetas):
        sizes.append(len(thetas))
        return ph.batch_of(ph.POSTERIOR3)(thetas)

    evals = advance_lockstep(together, 70, batch)
    evals += advance_lockstep(together, 50, batch)  # the direction update at length 100 falls into the second call
    assert evals == sum(sizes) and max(sizes) == 4
    for a, b in zip(alone[:3], together[:3]):
        same_state(a, b)
        assert list(b.update_history) == [100]
    assert_array_equal(alone[3].get_sample(burn=0), together[3].get_sample(burn=0))
    assert_array_equal(alone[3].probs, together[3].probs)
    for pa, pb in zip(alone[3].params, together[3].params):
        assert pa.sigma_values == pb.sigma_values and pa.sigma_checks == pb.sigma_checks


def ladders(count=2, seed=50):
    out = []
    for k in range(count):
        chains = []
        for level, temperature in enumerate((1.0, 2.0, 4.0)):
            chain = build("plain", seed=seed + 10 * k + level, temperature=temperature)
            chains.append(chain)
        lad = ParallelTempering(chains, batch_posterior=ph.batch_of(ph.POSTERIOR3))
        lad.rng = default_rng(seed + 10 * k + 7)
        lad.pair_choice = random.Random(seed + 10 * k + 8).choice
        out.append(lad)
    return out


def test_ladders_equal_parallel_tempering_alone():
    alone, together = ladders(), ladders()
    for lad in alone:
        lad.advance(125, swap_interval=10)
    advance_ladders(together, 125, swap_interval=10)
    for la, lb in zip(alone, together):
        assert_array_equal(la.successful_swaps, lb.successful_swaps)
        assert_array_equal(la.attempted_swaps, lb.attempted_swaps)
        assert la.successful_swaps.sum() > 0
        for a, b in zip(la.chains, lb.chains):
            same_state(a, b)
            assert list(b.update_history) == [100]
    # ... and ParallelTempering's own lockstep is the chains stepped one by one between the swaps
    serial = ladders(1)[0]
    serial.batch_posterior = None
    serial.advance(125, swap_interval=10)
    for a, b in zip(serial.chains, alone[0].chains):
        same_state(a, b)


def test_one_parameter_chain_fails_at_its_first_update():
    chain = PcaChain(ph.POSTERIOR1, np.array([0.7]), widths=[0.3], display_progress=False, covariance=ph.numpy_covariance)
    chain.rng = default_rng(3)
    chain.advance(98)
    assert chain.chain_length == 99
    with pytest.raises(ValueError):
        chain.take_step()  # step 99 brings the chain to length 100
    device_default = PcaChain(ph.POSTERIOR1, np.array([0.7]), widths=[0.3], display_progress=False)
    with pytest.raises(ValueError, match="one-parameter"):
        device_default.update_directions()  # refused before any device call


def test_axis_limits_warn_and_do_nothing():
    chain = build("plain")
    with pytest.warns(UserWarning, match="set_non_negative"):
        chain.set_non_negative(0)
    with pytest.warns(UserWarning, match="set_boundaries"):
        chain.set_boundaries(1, (0.0, 1.0))
    assert not any(p.non_negative or p.bounded for p in chain.params)


def test_bounds():
    lower, upper = np.array([-2.0, -2.0, -4.0]), np.array([4.0, 1.5, 8.0])
    as_pair = build("bounded")
    as_object = ph.build(PcaChain, "bounded", covariance=ph.numpy_covariance, bounds=Bounds(lower, upper))
    assert isinstance(as_pair.bounds, Bounds) and as_pair.process_proposal == as_pair.bounds.reflect
    as_pair.advance(30)
    as_object.advance(30)
    same_state_before_update = [ph.state(c)["sample"] for c in (as_pair, as_object)]
    assert_array_equal(*same_state_before_update)
    assert ((same_state_before_update[0] >= lower) & (same_state_before_update[0] <= upper)).all()
    with pytest.raises(ValueError, match=r"\[ PcaChain error \]"):
        ph.build(PcaChain, "bounded", bounds=(lower, np.array([4.0, 1.5])))
    with pytest.raises(ValueError, match="number of bounds"):
        ph.build(PcaChain, "bounded", bounds=(lower[:2], upper[:2]))
    with pytest.raises(ValueError, match="outside specified bounds"):
        ph.build(PcaChain, "bounded", bounds=(lower, np.array([4.0, 1.5, 2.0])))


def test_directions_diagnostics(g):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    chain = build("p5")
    chain.advance(ph.STEPS)
    updates, angles = chain.directions_diagnostics_data()
    assert updates.shape == (2,) and angles.shape == (2, 5)
    assert_array_equal(updates, g["p5_update_history"])
    assert_array_equal(angles, g["p5_angles_history"])
    fig = chain.directions_diagnostics(show=False)
    lines = fig.axes[0].lines
    assert len(lines) == 6  # one per parameter and the dashed 1e-2 level
    for i in range(5):
        assert_array_equal(lines[i].get_ydata(), angles[:, i])
    assert fig.axes[0].get_yscale() == "log"
    plt.close("all")
    fresh = build("plain")
    assert [a.shape for a in fresh.directions_diagnostics_data()] == [(0,), (0, 3)]


def test_inherited_readouts_without_a_device(g):
    chain = build("plain")
    chain.advance(ph.STEPS)
    assert chain.get_sample().shape == (ph.STEPS, 3) and chain.get_parameter(1, burn=10, thin=3).shape == (97,)
    sample, probs = chain.get_interval(interval=0.9, burn=50)
    assert sample.shape[1] == 3 and probs.size == sample.shape[0]
    assert_array_equal(chain.get_probabilities(burn=0), g["plain_probs"])


def test_sample_covariance_arguments():
    """What is refused before any device call."""
    from inference_amd.mcmc import sample_covariance

    with pytest.raises(ValueError, match="512"):
        sample_covariance(np.zeros((4, 513)))
    with pytest.raises(ValueError, match="two rows"):
        sample_covariance(np.zeros((1, 3)))
    with pytest.raises(ValueError, match="two rows"):
        sample_covariance(np.zeros(1))
    with pytest.raises(ValueError, match="one- or two-dimensional"):
        sample_covariance(np.zeros((2, 2, 2)))


def test_chunk_rows_constant_matches_the_header():
    import os
    import re

    from inference_amd import _lib

    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gpmi.h")
    with open(header) as f:
        found = re.search(r"#define\s+GPMI_COV_CHUNK_ROWS\s+(\d+)", f.read())
    assert found and int(found.group(1)) == _lib.COV_CHUNK_ROWS
    assert "gpmi_cov_columns" in _lib.SIGNATURES
