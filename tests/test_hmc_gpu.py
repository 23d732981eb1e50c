"""GPU tests of HamiltonianChain on the batched device gradient (`GpRegressor.marginal_likelihood_gradient_batch`): the
lockstep driver against the chains stepped alone (bit for bit), against the CPU oracle (within a tolerance that the test
measures on the CPU), ladders of HMC chains, the batch that survives a failed row, and the chain read-outs.

Two models: the N = 48 problem of test_mcmc_cpu.pt_problem (SE, P = 3, padded to one tile) and SE + WhiteNoise on N = 200,
d = 2 (P = 5, two tiles).  Every chain is bounded by the model's `hp_bounds`, starts with epsilon = 0.05 and makes about
8 leapfrog steps per trajectory."""
import random
import warnings

import numpy as np
import pytest
from numpy.random import default_rng
from numpy.testing import assert_allclose, assert_array_equal

import hmc_host as hh
import workloads as wl
from test_mcmc_cpu import pt_problem

pytestmark = pytest.mark.gpu

MODELS = ["pt48", "wn200"]


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


def one_by_one(gp):
    """The chain's own functions, through a batch of one (the single-evaluation kernels sum in another order)."""
    def posterior(t):
        return float(gp.marginal_likelihood_gradient_batch(t[None, :])[0][0])

    def grad(t):
        return gp.marginal_likelihood_gradient_batch(t[None, :])[1][0]

    return posterior, grad


def make_chain(posterior, grad, start, hp_bounds, temperature, seed):
    from inference_amd.mcmc import HamiltonianChain

    bounds = (np.array([b[0] for b in hp_bounds], dtype=float), np.array([b[1] for b in hp_bounds], dtype=float))
    chain = HamiltonianChain(posterior, start, grad=grad, epsilon=0.05, temperature=temperature, bounds=bounds,
                             display_progress=False)
    chain.rng = default_rng(seed)
    chain.steps = 8
    return chain


def same_state(a, b):
    sa, sb = hh.state(a), hh.state(b)
    for key in sa:
        assert_array_equal(sa[key], sb[key], err_msg=key)


@pytest.mark.parametrize("name", MODELS)
def test_hmc_lockstep_is_the_chains_run_alone(models, name):
    from inference_amd.mcmc import advance_lockstep_hmc

    gp, start = models(name)
    posterior, grad = one_by_one(gp)

    def chains():
        return [make_chain(posterior, grad, start, gp.hp_bounds, T, 500 + k) for k, T in enumerate((1, 1, 2, 2, 5, 5))]

    alone, together = chains(), chains()
    for ch in alone:
        for _ in range(6):
            ch.take_step()
    evals = advance_lockstep_hmc(together, 6, gp.marginal_likelihood_gradient_batch)
    assert evals == sum(sum(ch.leapfrog_steps) for ch in together) + 6
    for a, b in zip(alone, together):
        same_state(a, b)
    print(f"{name}: {evals} rows, leapfrog steps per chain {[sum(ch.leapfrog_steps) for ch in together]}")


def oracle_chain(ref, start, temperature, seed, ripple=0.0):
    """The chain on the CPU oracle; with `ripple`, every gradient it sees is multiplied by 1 + ripple cos(k + j), k the
    number of the call and j the component."""
    calls = [0]

    def grad(t):
        g = ref.marginal_likelihood_gradient(t)[1]
        calls[0] += 1
        return g * (1.0 + ripple * np.cos(calls[0] + np.arange(g.size)))

    return make_chain(ref.marginal_likelihood, grad, start, ref.hp_bounds, temperature, seed)


@pytest.mark.parametrize("T", [1.0, 3.0])
@pytest.mark.parametrize("name", MODELS)
def test_hmc_on_device_follows_the_cpu_oracle(models, name, T):
    """Ten steps of a chain on the device against the same chain on the CPU oracle.  A trajectory amplifies differences in
    the last digits of the gradient, so the allowance is measured here: the oracle chain is run again with its gradient
    rippled by 1e-11 (the gradient tolerance the parity tests grant the device), and 10 x the largest difference in theta
    between the two oracle runs is allowed (the factor the UnimodalPdf fit tests give a path-sensitive computation).
    Measured on an MI355X, device against oracle / allowed, in theta: N = 48 4.4e-15 / 8.1e-12 (T = 1) and 3.1e-15 / 1.0e-11
    (T = 3); N = 200 1.4e-13 / 9.3e-11 and 9.9e-14 / 2.1e-11."""
    from inference_amd.mcmc import advance_lockstep_hmc

    gp, start = models(name)
    ref, _ = oracle_model(name)
    assert_allclose(np.array(gp.hp_bounds), np.array(ref.hp_bounds), rtol=1e-12)
    seed = 700 + int(T)
    device = make_chain(*one_by_one(gp), start, gp.hp_bounds, T, seed)
    advance_lockstep_hmc([device], 10, gp.marginal_likelihood_gradient_batch)
    exact = oracle_chain(ref, start, T, seed)
    rec = hh.Recorder(exact)
    rippled = oracle_chain(ref, start, T, seed, ripple=1e-11)
    for ch in (exact, rippled):
        for _ in range(10):
            ch.take_step()
    accept, n_steps, review, _ = rec.margins()
    assert min(accept, review) >= 1e-6 and n_steps >= 1e-9, (accept, n_steps, review)  # (else: pick another seed)
    assert exact.leapfrog_steps == rippled.leapfrog_steps
    spread = np.abs(np.array(exact.theta) - np.array(rippled.theta)).max()
    error = np.abs(np.array(device.theta) - np.array(exact.theta)).max()
    print(f"{name} T = {T}: device vs oracle {error:.2e} in theta, oracle vs rippled oracle {spread:.2e} "
          f"(allowed {10 * spread:.2e}), leapfrog steps {sum(exact.leapfrog_steps)}")
    assert device.leapfrog_steps == exact.leapfrog_steps
    assert error <= 10 * spread
    assert_allclose(np.array(device.probs), np.array(exact.probs), rtol=1e-10)


def test_parallel_tempering_of_hmc_chains_on_device(models):
    from inference_amd.mcmc import ParallelTempering

    gp, start = models("pt48")
    posterior, grad = one_by_one(gp)

    def ladder(batch):
        chains = [make_chain(posterior, grad, start, gp.hp_bounds, T, 900 + k) for k, T in enumerate((1.0, 2.0, 4.0, 8.0))]
        pt = ParallelTempering(chains, batch_value_and_grad=batch)
        pt.rng = default_rng(17)
        return pt

    sequential, lockstep = ladder(None), ladder(gp.marginal_likelihood_gradient_batch)
    assert sequential.batch_posterior is None  # a plain callable: stepped one by one
    random.seed(3)
    sequential.advance(12, swap_interval=3)
    random.seed(3)
    lockstep.advance(12, swap_interval=3)
    assert sequential.successful_swaps.sum() >= 1
    for a, b in zip(sequential.chains, lockstep.chains):
        same_state(a, b)
    assert_array_equal(sequential.successful_swaps, lockstep.successful_swaps)
    assert_array_equal(sequential.attempted_swaps, lockstep.attempted_swaps)
    assert lockstep.posterior_evaluations >= sum(sum(ch.leapfrog_steps) for ch in lockstep.chains) + 4
    print(f"{int(sequential.successful_swaps.sum())} successful swaps, {lockstep.posterior_evaluations} rows")


def test_gradient_batch_sentinel(golden):
    from numpy.linalg import LinAlgError

    from inference_amd import gp as gp_mod

    g = golden("fail")
    gp = gp_mod.GpRegressor(g["x"], g["y"], y_cov=g["y_cov"], hyperpars=g["theta_ok"])
    thetas = np.array([g["theta_ok"], g["theta_bad"], g["theta_ok"]])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        values, grads = gp.marginal_likelihood_gradient_batch(thetas, failed="sentinel")
    assert len([w for w in caught if "Cholesky decomposition failure" in str(w.message)]) == 1
    assert values[1] == -1e50 and not grads[1].any()
    single_value, single_grad = gp.marginal_likelihood_gradient(g["theta_ok"])
    for row in (0, 2):
        assert_allclose(values[row], single_value, rtol=1e-12)
        assert_allclose(grads[row], single_grad, rtol=1e-11, atol=1e-11 * np.abs(single_grad).max())
    assert values[0] == values[2] and np.array_equal(grads[0], grads[2])
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_gradient_batch(thetas)
    with pytest.raises(LinAlgError):
        gp.marginal_likelihood_gradient_batch(thetas, failed="raise")
    with pytest.raises(ValueError):
        gp.marginal_likelihood_gradient_batch(thetas, failed="ignore")
    # nothing failed: no warning, the values of the default
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        quiet = gp.marginal_likelihood_gradient_batch(thetas[::2], failed="sentinel")
    loud = gp.marginal_likelihood_gradient_batch(thetas[::2])
    assert np.array_equal(quiet[0], loud[0]) and np.array_equal(quiet[1], loud[1])


def test_hmc_readouts_on_device(golden):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from inference_amd.pdf import GaussianKDE

    g = golden("hmc")
    chain = hh.rebuilt_chain(g)
    burn = int(g["long_diag_burn"])
    assert (chain.chain_length - burn) % 2 == 0  # an even length: the batch is the reference's number
    data = chain.diagnostics_data(burn=burn)
    assert_array_equal(data["ess"], g["long_diag_ess"])
    assert data["burn"] == burn and data["ess_min"] == int(g["long_diag_ess"].min())
    assert chain.diagnostics_data()["burn"] == int(g["long_burn"])
    assert_array_equal(data["epsilon_steps"], g["long_epsilon_checks"] * 1e-3)
    assert isinstance(chain.get_marginal(0), GaussianKDE)
    assert isinstance(chain.matrix_plot(burn=burn, thin=4), plt.Figure)
    fig = chain.plot_diagnostics(show=False, burn=burn)
    assert isinstance(fig, plt.Figure) and len(fig.axes) == 4
    assert_array_equal([b.get_height() for b in fig.axes[2].patches], g["long_diag_ess"])
    assert [t.get_text() for t in fig.axes[3].texts][1::2] == ["{:.5G}".format(v) for v in (burn, data["ess_mean"], data["ess_min"])]
    plt.close("all")
