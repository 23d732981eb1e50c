"""CPU tests of the chain diagnostics: the host `effective_sample_size`, `GibbsChain.estimate_burn_in`,
`transition_matrix_plot` and `ParallelTempering.swap_diagnostics_data` against the reference's own outputs in
golden/ess.npz (golden/make_golden_ess.py), and the NumPy lag-sum mirror of tests/ess_host.py - the device's definition -
against the reference's FFT route where the two describe the same numbers (even n)."""
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import ess_host as eh


@pytest.fixture(scope="module")
def g(golden):
    return golden("ess")


@pytest.mark.parametrize("name", eh.EVEN + eh.ODD + ["layout", "tiny_4"])
def test_host_function_gives_the_reference_integer(g, name):
    from inference_amd.mcmc import effective_sample_size

    s = eh.checked_case(g, name)
    got = np.array([effective_sample_size(c) for c in s.T])
    assert_array_equal(got, g[f"{name}_ess"])
    assert all(type(effective_sample_size(c)) is int for c in s.T[:2])


def test_host_function_on_the_chain(g):
    from inference_amd.mcmc import effective_sample_size

    chain = eh.rebuilt_chain(g)
    burn = int(g["chain_burn"])
    assert_array_equal([effective_sample_size(chain.get_parameter(i, burn=burn)) for i in range(3)], g["chain_ess"])


def test_no_negative_lag_is_the_reference_index_error(g):
    from inference_amd.mcmc import effective_sample_size

    with pytest.raises(IndexError):
        effective_sample_size(eh.checked_case(g, "tiny_2")[:, 0])
    const = eh.checked_case(g, "const")
    with pytest.raises(IndexError):
        effective_sample_size(const[:, 0])
    with pytest.raises(IndexError):
        effective_sample_size(const[:, 2])
    assert effective_sample_size(const[:, 1]) > 0


def test_negative_first_element_is_a_value_error(monkeypatch):
    from inference_amd.mcmc import utilities
    from inference_amd.pdf import _messages as msg

    monkeypatch.setattr(utilities, "irfft", lambda power: np.array([-1.0, 0.5, 0.25, 0.1]))
    with pytest.raises(ValueError, match="First element of the autocorrelation is negative"):
        utilities.effective_sample_size(np.arange(4.0))
    assert msg.ess_negative_first() == "First element of the autocorrelation is negative"


@pytest.mark.parametrize("name", eh.EVEN + ["layout", "tiny_4"])
def test_mirror_agrees_with_the_reference_for_even_n(g, name):
    s = eh.checked_case(g, name)
    assert s.shape[0] % 2 == 0
    f0, total, cut, ess = eh.mirror(s)
    assert_array_equal(cut, g[f"{name}_cut"])
    assert_array_equal(ess, g[f"{name}_ess"])
    assert_allclose(f0, g[f"{name}_f0"], rtol=eh.TOL, atol=0)
    assert_allclose(total, g[f"{name}_sum"], rtol=eh.TOL, atol=0)


@pytest.mark.parametrize("name", eh.ODD)
def test_mirror_reproduces_its_stored_numbers_for_odd_n(g, name):
    s = eh.checked_case(g, name)
    assert s.shape[0] % 2 == 1
    f0, total, cut, ess = eh.mirror(s)
    assert_array_equal(cut, g[f"{name}_mirror_cut"])
    assert_array_equal(ess, g[f"{name}_mirror_ess"])
    assert_allclose(f0, g[f"{name}_mirror_f0"], rtol=eh.TOL, atol=0)
    assert_allclose(total, g[f"{name}_mirror_sum"], rtol=eh.TOL, atol=0)


def test_the_odd_length_quirk_is_real(g):
    """The reference's integer and the length-n autocorrelation's differ for a column of ar_4097: the quirk the README
    documents, kept in the host function and not in the batch."""
    assert (g["ar_4097_ess"] != g["ar_4097_mirror_ess"]).any()


def test_cosine_cut_is_its_parameter():
    for c in (3, 511, 512, 513):
        assert eh.mirror_column(eh.cosine(c)[:, 0])[2] == c


def test_estimate_burn_in(g):
    chain = eh.rebuilt_chain(g)
    burn = chain.estimate_burn_in()
    assert type(burn) is int
    assert burn == int(g["chain_burn"])


def test_estimate_burn_in_keeps_the_argmax_quirk(g):
    """A parameter whose width never was 15 % away from its final value contributes its LAST review."""
    chain = eh.rebuilt_chain(g)
    chain.probs = list(np.linspace(0.0, -1.0, len(chain.probs)))  # the best step is the first: the widths decide
    for p in chain.params:
        p.sigma_values = [p.sigma * 1.01, p.sigma * 0.99, p.sigma]
        p.sigma_checks = [0.0, 100, 700]
    assert chain.estimate_burn_in() == 700


def _read(ax):
    pc = ax.collections[0]
    return {"corners": np.array([p.vertices[0] for p in pc.get_paths()]),
            "sizes": np.array([p.vertices[2] - p.vertices[0] for p in pc.get_paths()]),
            "colors": np.array(pc.get_facecolor()),
            "labels": np.array([t.get_text() for t in ax.texts]),
            "label_xy": np.array([t.get_position() for t in ax.texts]),
            "limits": np.array([ax.get_xlim(), ax.get_ylim()])}


def _same(got, g, prefix):
    for key, value in got.items():
        assert_array_equal(value, g[f"{prefix}_{key}"], err_msg=f"{prefix}_{key}")


def test_transition_matrix_plot(g):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from inference_amd.plotting import transition_matrix_plot

    rates = g["tm_matrix"]
    _, ax = plt.subplots()
    assert transition_matrix_plot(axis=ax, matrix=rates) is ax
    _same(_read(ax), g, "tm_full")
    _, ax = plt.subplots()
    transition_matrix_plot(axis=ax, matrix=rates, colormap="plasma", exclude_diagonal=True, upper_triangular=True)
    _same(_read(ax), g, "tm_upper")
    # an unknown colormap warns and draws viridis
    _, ax = plt.subplots()
    with pytest.warns(UserWarning, match="'no_such_map' is not a valid colormap from matplotlib.colormaps"):
        transition_matrix_plot(axis=ax, matrix=rates, colormap="no_such_map")
    _same(_read(ax), g, "tm_full")
    # an axis of its own; no labels from 11 x 11 on
    big = np.random.default_rng(3).random((11, 11))
    ax = transition_matrix_plot(matrix=big)
    assert ax.figure is not None and len(ax.texts) == 0 and len(ax.collections[0].get_paths()) == 121
    plt.close("all")


def test_transition_matrix_plot_errors():
    from inference_amd.plotting import transition_matrix_plot

    with pytest.raises(TypeError, match="given matrix must be a numpy.ndarray"):
        transition_matrix_plot(matrix=[[0.1, 0.2], [0.3, 0.4]])
    with pytest.raises(ValueError, match="given matrix must have exactly two dimensions"):
        transition_matrix_plot(matrix=np.zeros(4))
    with pytest.raises(ValueError, match="given matrix must be square"):
        transition_matrix_plot(matrix=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="given matrix must be at least of size 2x2"):
        transition_matrix_plot(matrix=np.ones((1, 1)))


def test_swap_diagnostics(g):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    ladder = eh.rebuilt_ladder(g)
    rate_matrix, total_swaps = ladder.swap_diagnostics_data()
    assert_array_equal(rate_matrix, g["swap_rate_matrix"])
    assert_array_equal(total_swaps, g["swap_total"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fig = ladder.swap_diagnostics(show=False)
    assert len(fig.axes) == 2
    _same(_read(fig.axes[0]), g, "swap_axis")
    assert_array_equal([b.get_height() for b in fig.axes[1].patches], g["swap_total"])
    assert fig.axes[0].get_title() == "acceptance rate of chain position swaps"
    assert fig.axes[1].get_ylabel() == "total successful position swaps"
    plt.close("all")


def test_imports_do_not_need_matplotlib():
    code = ("import sys; import inference_amd.mcmc.utilities, inference_amd.plotting, inference_amd.mcmc; "
            "assert 'matplotlib' not in sys.modules, 'matplotlib was imported'")
    path = [p for p in sys.path if p]
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path[:0] = {path!r}; {code}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_lag_block_schedule():
    """The schedule of csrc/acf.hip, from the library itself (host-only): blocks of 256, 256, 512, 1024 and then 2048
    lags, below n // 2."""
    from inference_amd.pdf import _device

    assert _device.acf_lag_blocks(2) == [0]
    assert _device.acf_lag_blocks(512) == [0]
    assert _device.acf_lag_blocks(514) == [0, 256]
    assert _device.acf_lag_blocks(4 * 1024) == [0, 256, 512, 1024]
    assert _device.acf_lag_blocks(20000) == [0, 256, 512, 1024, 2048, 4096, 6144, 8192]
    with pytest.raises(ValueError):
        _device.acf_lag_blocks(1)
