"""CPU tests of EnsembleSampler and advance_lockstep_ensembles: serial mode against the reference's traces bit for bit
(golden/ensemble.npz, written by golden/make_golden_ensemble.py), the start-up checks, save / load in both directions, split
mode against a walker-by-walker NumPy mirror, the lockstep driver against the samplers advanced alone, and the
distribution that split mode samples.  Recipes, recorder and mirror are in tests/ensemble_host.py."""
import numpy as np
import pytest
from numpy.random import default_rng
from numpy.testing import assert_array_equal

import ensemble_host as eh
from inference_amd.mcmc import Bounds, EnsembleSampler, advance_lockstep_ensembles


def same_state(got, want, what=""):
    got = got if isinstance(got, dict) else eh.state(got)
    want = want if isinstance(want, dict) else eh.state(want)
    for key in eh.STATE_KEYS:
        assert_array_equal(got[key], want[key], err_msg=f"{what} {key}")


def golden_state(g, prefix):
    return {key: g[f"{prefix}_{key}"] for key in eh.STATE_KEYS}


# --------------------------------------------------------------------------------------------- serial mode: the reference
@pytest.mark.parametrize("name", sorted(eh.CASES))
@pytest.mark.parametrize("batched", [False, True])
def test_serial_mode_is_the_reference_bit_for_bit(golden, name, batched):
    g = golden("ensemble")
    case = eh.CASES[name]
    kw = dict(batch_posterior=eh.batch_of(case["post"])) if batched else {}
    sampler = eh.build(EnsembleSampler, name, **kw)
    sampler.advance(case["iterations"])
    same_state(sampler, golden_state(g, name), name)
    assert_array_equal(sampler.mode(), g[f"{name}_mode"])
    assert sampler.n_iterations == case["iterations"]
    assert sampler.chain_length == case["iterations"] * case["walkers"]
    assert (sampler.n_walkers, sampler.n_parameters) == (case["walkers"], case["P"])
    if name == "d":
        assert sampler.max_attempts == 3 and any(sampler.failed_updates)
        assert ((np.array(sampler.total_proposals) == 3).sum(axis=0) >= sampler.failed_updates).all()


def test_seed_keyword_is_a_generator_set_after_construction(golden):
    g = golden("ensemble")
    sampler = EnsembleSampler(eh.post_a, eh.starts("a"), display_progress=False)
    sampler.rng = default_rng(eh.SEED)
    sampler.advance(20)
    sampler.advance(20)  # (two calls: the sample is joined)
    same_state(sampler, golden_state(g, "a"))


def test_readouts_follow_the_reference(golden):
    g = golden("ensemble")
    sampler = eh.build(EnsembleSampler, "b")
    sampler.advance(eh.CASES["b"]["iterations"])
    assert_array_equal(sampler.get_parameter(1, burn=16, thin=3), g["b_parameter"])
    assert_array_equal(sampler.get_probabilities(burn=16, thin=3), g["b_probabilities"])
    assert_array_equal(sampler.get_sample(burn=16, thin=3), g["b_sample_thinned"])
    assert_array_equal(sampler.get_parameter(2), g["b_parameter_default"])  # burn defaults to 0
    assert sampler.get_parameter(2).size == sampler.chain_length
    sample, probs = sampler.get_interval(interval=0.9, burn=16, thin=2)
    assert_array_equal(sample, g["b_interval_sample"])
    assert_array_equal(probs, g["b_interval_probs"])


def test_diagnostics_data_and_plot():
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    sampler = eh.build(EnsembleSampler, "d")
    sampler.advance(30)
    data = sampler.diagnostics_data()
    proposals = np.array(sampler.total_proposals)
    assert_array_equal(data["acceptance_rates"], np.arange(1.0, 31.0) / proposals.cumsum(axis=1))
    assert_array_equal(data["mean_acceptance_rate"], data["acceptance_rates"].mean(axis=0))
    assert_array_equal(data["probs"], sampler.sample_probs.reshape(30, 6))
    assert_array_equal(data["median_probs"], np.median(data["probs"], axis=1))
    assert_array_equal(data["failed_updates"], sampler.failed_updates)
    assert "ess" not in data
    fig = sampler.plot_diagnostics(show=False)
    assert isinstance(fig, plt.Figure) and len(fig.axes) == 2
    assert len(fig.axes[0].lines) == 6 + 1
    plt.close("all")


# --------------------------------------------------------------------------------------------- start-up checks
def test_start_up_checks_raise():
    good = eh.starts("b")
    colinear = good.copy()
    colinear[:, 1] = 2.0 * colinear[:, 0] + 1e-6 * colinear[:, 2]
    flat = good.copy()
    flat[:, 2] = 1.0
    outside = good.copy()
    outside[3, 0] = eh.UPPER_B[0] + 0.1
    bounds = (eh.LOWER_B, eh.UPPER_B)
    broken = good.copy()
    broken[0, 0] = np.inf
    cases = [
        dict(starting_positions=colinear),
        dict(starting_positions=flat),
        dict(starting_positions=np.ones((5, 1))),
        dict(starting_positions=good, bounds=(eh.LOWER_B[:2], eh.UPPER_B[:2])),
        dict(starting_positions=good, bounds=(eh.LOWER_B, eh.UPPER_B[:2])),
        dict(starting_positions=outside, bounds=bounds),
        dict(starting_positions=good, alpha=1.0),
        dict(starting_positions=good, alpha=0.5),
        dict(starting_positions=good.tolist()),
        dict(starting_positions=good[:3]),
        dict(starting_positions=broken),
        dict(starting_positions=good[:, 0].copy()),  # 1D: passes the checks as a column, fails at the unpacking of .shape
        dict(starting_positions=good, bounds=5.0),
        dict(starting_positions=good, update="parallel"),
        dict(starting_positions=good[:7], update="split"),  # 2 (P + 1) - 1 walkers
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            EnsembleSampler(eh.post_b, display_progress=False, **kw)
    assert isinstance(EnsembleSampler(eh.post_b, good, bounds=Bounds(*bounds), update="split").bounds, Bounds)
    with pytest.raises(ValueError, match="EnsembleSampler error"):
        EnsembleSampler(eh.post_b, good, alpha=1.0)


# --------------------------------------------------------------------------------------------- save / load
def test_save_load_and_advance(golden, tmp_path):
    g = golden("ensemble")
    iterations = eh.CASES["b"]["iterations"]
    for update in ("serial", "split"):
        never_saved = eh.build(EnsembleSampler, "b", update=update)
        never_saved.advance(iterations + eh.MORE)
        sampler = eh.build(EnsembleSampler, "b", update=update)
        sampler.advance(iterations)
        path = tmp_path / f"{update}.npz"
        sampler.save(path)
        with np.load(path, allow_pickle=False) as D:
            assert set(g["save_keys"]) <= set(D.keys())
            assert {"failed_updates", "update"} <= set(D.keys())
            for key in g["save_keys"]:
                if update == "serial":
                    assert_array_equal(D[key], g[f"save_b_{key}"], err_msg=key)
                assert D[key].dtype == g[f"save_b_{key}"].dtype and D[key].shape == g[f"save_b_{key}"].shape, key
        loaded = EnsembleSampler.load(path, posterior=eh.post_b)
        same_state(loaded, sampler, update)
        for key in ("n_walkers", "n_parameters", "n_iterations", "chain_length", "max_attempts", "alpha", "update",
                    "display_progress", "x_lwr", "x_width"):
            assert getattr(loaded, key) == getattr(sampler, key), key
        assert_array_equal(loaded.bounds.lower, eh.LOWER_B)
        assert loaded.rng.bit_generator.state == sampler.rng.bit_generator.state
        loaded.advance(eh.MORE)
        same_state(loaded, never_saved, f"{update} after load")


def test_a_file_of_the_reference_loads_and_advances(golden, tmp_path):
    g = golden("ensemble")
    path = tmp_path / "reference.npz"
    np.savez(path, **{str(key): g[f"save_b_{key}"] for key in g["save_keys"]})
    loaded = EnsembleSampler.load(path, posterior=eh.post_b)
    assert loaded.update == "serial" and loaded.failed_updates == [0] * eh.CASES["b"]["iterations"]
    assert loaded.chain_length == g["b_sample_probs"].size
    assert_array_equal(loaded.sample, g["b_sample"])
    loaded.rng = default_rng(eh.SEED + 1)
    loaded.advance(eh.MORE)
    got, want = eh.state(loaded), golden_state(g, "more")
    for key in eh.STATE_KEYS[:-1]:
        assert_array_equal(got[key], want[key], err_msg=key)
    assert_array_equal(got["failed_updates"][-eh.MORE:], want["failed_updates"][-eh.MORE:])


# --------------------------------------------------------------------------------------------- split mode
@pytest.mark.parametrize("max_attempts", [1, 100])
@pytest.mark.parametrize("name,walkers", [("a", 12), ("a", 16), ("a", 13), ("b", 12), ("b", 16), ("b", 9)])
@pytest.mark.parametrize("batched", [False, True])
def test_split_mode_is_the_mirror_bit_for_bit(name, walkers, max_attempts, batched):
    case = eh.CASES[name]
    kw = dict(case["kw"])
    mirror = eh.split_mirror(case["post"], eh.starts(name, walkers), 25, max_attempts=max_attempts, **kw)
    calls = []

    def batch(rows):
        calls.append(len(rows))
        return eh.batch_of(case["post"])(rows)

    sampler = eh.build(EnsembleSampler, name, walkers=walkers, max_attempts=max_attempts, update="split",
                       **(dict(batch_posterior=batch) if batched else {}))
    sampler.advance(25)
    same_state(sampler, mirror, f"{name} {walkers}")
    if batched:
        assert calls[0] == walkers and calls[1] == walkers // 2  # the starting probabilities, then the first round of A
        assert sum(calls[1:]) == np.array(sampler.total_proposals).sum()
    if max_attempts == 1:
        assert (np.array(sampler.total_proposals) == 1).all() and sum(sampler.failed_updates) > 0
        assert len(calls) in (0, 1 + 2 * 25)


def test_split_reflection_is_bounds_reflect_row_by_row():
    sampler = eh.build(EnsembleSampler, "b", update="split")
    rows = eh.LOWER_B + (eh.UPPER_B - eh.LOWER_B) * default_rng(3).uniform(-4.0, 5.0, size=(64, 3))
    assert not all(sampler.bounds.inside(r) for r in rows)
    assert_array_equal(sampler.process_proposal(rows), np.array([sampler.bounds.reflect(r) for r in rows]))


def test_split_mode_needs_two_full_halves():
    with pytest.raises(ValueError):
        eh.build(EnsembleSampler, "a", walkers=2 * (2 + 1) - 1, update="split")
    eh.build(EnsembleSampler, "a", walkers=2 * (2 + 1), update="split")


# --------------------------------------------------------------------------------------------- the lockstep driver
def five_samplers(batch_posterior=None):
    kw = dict(batch_posterior=batch_posterior) if batch_posterior else {}
    tight = (eh.LOWER_B - 0.5, eh.UPPER_B + 0.5)
    return [
        eh.build(EnsembleSampler, "b", seed=1, **kw),
        eh.build(EnsembleSampler, "b", seed=2, walkers=12, update="split", **kw),
        eh.build(EnsembleSampler, "b", seed=3, walkers=9, update="split", alpha=1.5, max_attempts=2, **kw),
        eh.build(EnsembleSampler, "b", seed=4, walkers=5, bounds=None, alpha=2.5, **kw),
        eh.build(EnsembleSampler, "b", seed=5, walkers=16, update="split", bounds=tight, max_attempts=1, **kw),
    ]


@pytest.mark.parametrize("max_batch", [None, 3])
@pytest.mark.parametrize("own_batch", [False, True])
def test_lockstep_is_the_samplers_advanced_alone(max_batch, own_batch):
    batch = eh.batch_of(eh.post_b)
    sizes = []

    def counted(rows):
        sizes.append(len(rows))
        return batch(rows)

    alone, together = five_samplers(batch if own_batch else None), five_samplers()
    for s in alone:
        s.advance(7)
        s.advance(5)
    before = sum(np.array(s.total_proposals).sum() for s in together)
    assert before == 0
    rows = advance_lockstep_ensembles(together, 7, counted, max_batch=max_batch)
    rows += advance_lockstep_ensembles(together, 5, counted, max_batch=max_batch)
    assert rows == sum(np.array(s.total_proposals).sum() for s in together) == sum(sizes)
    for k, (a, b) in enumerate(zip(alone, together)):
        same_state(a, b, f"sampler {k}")
        assert a.n_iterations == b.n_iterations == 12 and b.chain_length == 12 * b.n_walkers
    if max_batch:
        assert max(sizes) <= max_batch
    else:
        assert sizes[0] == 1 + 6 + 4 + 1 + 8  # one row of a serial sampler, the first half of a split one
    assert advance_lockstep_ensembles([], 5, counted) == 0 and advance_lockstep_ensembles(together, 0, counted) == 0


def test_lockstep_refuses_samplers_of_different_sizes():
    with pytest.raises(ValueError):
        advance_lockstep_ensembles([eh.build(EnsembleSampler, "a"), eh.build(EnsembleSampler, "b")], 1, eh.batch_of(eh.post_a))


# --------------------------------------------------------------------------------------------- the sampled distribution
MEAN3 = np.array([1.0, -2.0, 0.5])
COV3 = np.array([[1.0, 0.96, -0.15], [0.96, 1.44, 0.06], [-0.15, 0.06, 0.25]])  # correlations 0.8, -0.3 and 0.1
BUDGET = 12_000  # posterior evaluations of a run


def gaussian_errors(update, seed):
    """A run of 32 walkers on the 3-D Gaussian until it has made BUDGET evaluations (it ends with the iteration in which
    it reaches them: at most 32 x max_attempts more); the first fifth of its iterations is dropped.  Returns the largest
    error of a mean in units of its sigma, of a covariance in units of sqrt(S_kk S_ll), and the evaluations made."""
    precision = np.linalg.inv(COV3)

    def batch(rows):
        d = rows - MEAN3
        return -0.5 * np.einsum("ri,ij,rj->r", d, precision, d)

    start = MEAN3 + default_rng(100 + seed).normal(size=(32, 3))
    sampler = EnsembleSampler(None, start, display_progress=False, update=update, batch_posterior=batch, seed=seed)
    while np.array(sampler.total_proposals).sum() < BUDGET:
        sampler.advance(1)
    sample = sampler.get_sample(burn=32 * (sampler.n_iterations // 5))
    sigma = np.sqrt(np.diag(COV3))
    mean_error = np.abs((sample.mean(axis=0) - MEAN3) / sigma).max()
    cov_error = np.abs((np.cov(sample.T) - COV3) / np.outer(sigma, sigma)).max()
    return mean_error, cov_error, int(np.array(sampler.total_proposals).sum())


def test_split_mode_samples_the_distribution_of_serial_mode():
    """3-D correlated Gaussian, 32 walkers, seeds 0 .. 7, 12 000 evaluations per run in both modes.  The worst error over
    the 8 split runs may be at most 2 x the worst over the 8 serial (reference-parity) runs: both are Monte-Carlo
    estimates of equal cost, and a factor 2 between two worst-of-eight values is far outside their scatter.
    Measured, worst of eight: mean 0.2385 sigma (serial) and 0.1541 (split); covariance 0.6685 (serial) and 0.6628 (split).
    The covariance figures are NOT scatter: every run of either mode lies between 0.51 and 0.67. The reference moves a
    walker to X_i + z (X_j - X_i), which is X_j + (1 - z) (X_i - X_j): the stretch about the partner is 1 - z and not z,
    the factor z^(P - 1) does not balance that move, and the ensemble settles at about half the target's variances (a
    third with max_attempts = 1).  Both modes keep the reference's proposal (README, quirk table), so they agree with each
    other, which is what this test asserts, and differ from the target alike."""
    assert np.linalg.eigvalsh(COV3).min() > 0
    serial = np.array([gaussian_errors("serial", seed) for seed in range(8)])
    split = np.array([gaussian_errors("split", seed) for seed in range(8)])
    print(f"mean: serial {serial[:, 0].max():.4f} split {split[:, 0].max():.4f}; covariance: serial {serial[:, 1].max():.4f} "
          f"split {split[:, 1].max():.4f}; evaluations serial {serial[:, 2].min():.0f} .. {serial[:, 2].max():.0f}, "
          f"split {split[:, 2].min():.0f} .. {split[:, 2].max():.0f}")
    assert np.abs(serial[:, 2] - BUDGET).max() <= 0.01 * BUDGET and np.abs(split[:, 2] - BUDGET).max() <= 0.01 * BUDGET
    assert split[:, 0].max() <= 2.0 * serial[:, 0].max()
    assert split[:, 1].max() <= 2.0 * serial[:, 1].max()
