"""GPU tests of PcaChain with its default covariance, one `sample_covariance` device call per direction update
(csrc/cov.hip), against the reference's traces in golden/pca.npz (golden/make_golden_pca.py), and of the lockstep driver
over PcaChains on a device GP.

Up to the first update (chain length 100) no covariance has entered the chain: the sample is the reference's bit for bit.
After it the device's covariance differs from NumPy's in the last digits, within (2 n + 16) 2^-53 per entry; the maker
ran every recipe again with a relative ripple of 2^-44 (the next power of two above that bound) on the reference's
covariance and stored the largest deviation of the sample, `<case>_ripple_dev`.  The allowance here is 10 times that - the
project's usual margin over the reference's own spread, because the device's rounding is not the ripple's."""
import numpy as np
import pytest
from numpy.random import default_rng
from numpy.testing import assert_allclose, assert_array_equal

import pca_host as ph
import workloads as wl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("pca")


@pytest.fixture(scope="module")
def traces():
    """Every recipe run once on the default (device) covariance, with the device calls it made."""
    from inference_amd.mcmc import PcaChain
    from inference_amd.pdf import _device

    out = {}
    inner = _device._call
    for name in ph.CASES:
        calls = []

        def spy(h, fn, *args, calls=calls):
            calls.append((fn, tuple(args[1:3])))
            return inner(h, fn, *args)

        _device._call = spy
        try:
            chain = ph.build(PcaChain, name)
            chain.advance(ph.STEPS)
        finally:
            _device._call = inner
        out[name] = (chain, calls)
    return out


@pytest.mark.parametrize("name", list(ph.CASES))
def test_reference_traces_on_the_device_covariance(g, traces, name):
    chain, _ = traces[name]
    got = ph.state(chain)
    tol = 10.0 * float(g[f"{name}_ripple_dev"])
    want = g[f"{name}_sample"]
    assert_array_equal(got["sample"][:100], want[:100])
    assert_array_equal(got["probs"][:100], g[f"{name}_probs"][:100])
    dev = float(np.abs(got["sample"] - want).max())
    rel_covar = float(np.abs(got["covar"] / g[f"{name}_covar"] - 1.0).max())
    print(f"{name}: sample deviation {dev:.2e}, covar {rel_covar:.2e} relative, allowance {tol:.2e}")
    assert_array_equal(got["update_history"], g[f"{name}_update_history"])
    assert_allclose(got["sample"], want, rtol=0, atol=tol)
    assert_allclose(got["covar"], g[f"{name}_covar"], rtol=tol, atol=0)
    for i in range(chain.n_parameters):
        assert_array_equal(got[f"sigma_checks_{i}"], g[f"{name}_sigma_checks_{i}"])


@pytest.mark.parametrize("name", list(ph.CASES))
def test_logged_angles_on_the_device_covariance(g, traces, name):
    """The logged sines sqrt(1 - (v_new . v_old)^2) within the same allowance, relative.  A sine s of a small angle
    carries the rounding of the dot product divided by s^2, which the deviation of the sample knows nothing of; so the
    maker asserts of every fixture that its own rippled runs keep the sines within this allowance (`<case>_ripple_angles`,
    the largest relative deviation over the 49 ripples, printed beside the device's figure)."""
    chain, _ = traces[name]
    got = ph.state(chain)
    tol = 10.0 * float(g[f"{name}_ripple_dev"])
    rel_angles = float(np.abs(got["angles_history"] / g[f"{name}_angles_history"] - 1.0).max())
    print(f"{name}: angles {rel_angles:.2e} relative, allowance {tol:.2e}; under the maker's ripples "
          f"{float(g[f'{name}_ripple_angles']):.2e}; smallest sine {float(g[f'{name}_angles_history'].min()):.2e}")
    assert_allclose(got["angles_history"], g[f"{name}_angles_history"], rtol=tol, atol=0)


@pytest.mark.parametrize("name", list(ph.CASES))
def test_one_device_call_per_update(g, traces, name):
    """300 steps are two updates, each ONE gpmi_cov_columns call over the rows since the update before:
    `get_parameter(i)[last_update:]` keeps its burn of one sample, which makes 99 rows at length 100 and 149 at length 250
    (the counts the reference's own numpy.cov calls saw, recorded by the maker as `<case>_update_rows`)."""
    chain, calls = traces[name]
    P = chain.n_parameters
    assert g[f"{name}_update_rows"].tolist() == ph.UPDATE_ROWS
    assert calls == [("gpmi_cov_columns", (rows, P)) for rows in ph.UPDATE_ROWS]


def test_lockstep_on_the_device():
    """Eight PcaChains on the log-marginal likelihood of a device GP (N = 48, d = 2, SE + WhiteNoise), 120 steps in
    lockstep - one batched evaluation per round of proposals, the direction update of every chain in the middle of the
    call - against the same chains advanced alone through batches of one."""
    from inference_amd import gp as gp_mod
    from inference_amd.mcmc import PcaChain, advance_lockstep

    x, y, e = wl.synthetic_dataset(7, 48, 2)
    start = np.array([y.mean(), np.log(y.std()), np.log(0.5), np.log(0.5), np.log(0.1)])
    gp = gp_mod.GpRegressor(x, y, y_err=e, hyperpars=start, kernel=gp_mod.SquaredExponential() + gp_mod.WhiteNoise())
    gp.batch_independent_values(True)
    assert gp.marginal_likelihood.__self__ is gp
    bounds = (np.array([b[0] for b in gp.hp_bounds], dtype=float), np.array([b[1] for b in gp.hp_bounds], dtype=float))

    def posterior(t):  # gp.marginal_likelihood through a batch of one (the single-evaluation kernels sum in another order)
        return float(gp.marginal_likelihood_batch(t[None, :])[0])

    def chains():
        out = []
        for k, T in enumerate((1, 1, 1, 2, 2, 2, 5, 5)):
            chain = PcaChain(posterior, start, widths=[0.1] * 5, temperature=T, bounds=bounds, display_progress=False)
            chain.rng = default_rng(700 + k)
            out.append(chain)
        return out

    alone, together = chains(), chains()
    for chain in alone:
        chain.advance(120)
    sizes = []

    def batch(thetas):
        sizes.append(len(thetas))
        return gp.marginal_likelihood_batch(thetas)

    evals = advance_lockstep(together, 120, batch)
    assert evals == sum(sizes) and sizes[0] == 8
    for a, b in zip(alone, together):
        sa, sb = ph.state(a), ph.state(b)
        for key in sa:
            assert_array_equal(sa[key], sb[key], err_msg=key)
        assert list(b.update_history) == [100]
    print(f"{evals} evaluations in {len(sizes)} rounds")
