"""CPU tests of `sample_hdi_batch`, `hdi_plot_data` / `hdi_plot`, `trace_plot_data` / `trace_plot` and
`GibbsChain.trace_plot` with `_device.hdi_columns` replaced by the NumPy stand-in of tests/hdi_host.py (the product has no
CPU path: without the stand-in and without a GPU the call raises).  Expected values are the reference's, from
golden/hdi.npz (golden/make_golden_hdi.py)."""
import subprocess
import sys
import warnings

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import hdi_host as hh


@pytest.fixture(scope="module")
def g(golden):
    return golden("hdi")


@pytest.fixture
def host(monkeypatch):
    from inference_amd.pdf import _device

    stand_in = hh.HostHdi()
    monkeypatch.setattr(_device, "hdi_columns", stand_in)
    return stand_in


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def test_validation_texts_before_any_device_work(host):
    from inference_amd.pdf import _messages as msg
    from inference_amd.pdf import sample_hdi_batch

    s = np.arange(40.0).reshape(20, 2)
    for bad in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError) as err:
            sample_hdi_batch(s, [0.5, bad])
        assert str(err.value) == msg.hdi_bad_fraction(bad)
    with pytest.raises(ValueError) as err:
        sample_hdi_batch({1.0, 2.0}, [0.5])
    assert str(err.value) == msg.hdi_bad_type(set)
    with pytest.raises(ValueError) as err:
        sample_hdi_batch(np.zeros((3, 3, 3)), [0.5])
    assert str(err.value) == msg.hdi_bad_ndim(3)
    with pytest.raises(ValueError) as err:
        sample_hdi_batch(np.array(1.0), [0.5])
    assert str(err.value) == msg.hdi_bad_ndim(0)
    with pytest.raises(ValueError) as err:
        sample_hdi_batch(np.zeros((1, 4)), [0.5])
    assert str(err.value) == msg.hdi_too_short()
    assert host.calls == []


def test_warnings_once_per_fraction(host):
    from inference_amd.pdf import _messages as msg
    from inference_amd.pdf import sample_hdi_batch

    s = np.random.default_rng(0).normal(size=(100, 3))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        sample_hdi_batch(s, [0.5, 0.85, 0.999, 0.9])
    assert [str(w.message) for w in seen] == [msg.hdi_inaccurate(), msg.hdi_inaccurate(), msg.hdi_inaccurate()]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        sample_hdi_batch(s, [0.5, 0.8])
    assert seen == []
    # and the same warnings as sample_hdi itself gives, fraction by fraction
    from inference_amd.pdf import sample_hdi

    for f in (0.5, 0.81, 0.85, 0.999):
        with warnings.catch_warnings(record=True) as one:
            warnings.simplefilter("always")
            sample_hdi(s, f)
        with warnings.catch_warnings(record=True) as many:
            warnings.simplefilter("always")
            sample_hdi_batch(s, [f])
        assert [str(w.message) for w in one] == [str(w.message) for w in many]


def test_window_lengths_are_python_ints_of_the_product(host):
    from inference_amd.pdf import sample_hdi_batch

    s = np.random.default_rng(1).normal(size=100)
    quiet(sample_hdi_batch, s, [0.29, 0.57, 0.58, 0.07])
    assert host.calls == [((100, 1), (28, 56, 57, 7))]  # int(0.29 * 100) = 28 and int(0.57 * 100) = 56, as in the reference
    assert int(0.29 * 100) == 28 and int(0.57 * 100) == 56


def test_shapes_and_values(g, host):
    from inference_amd.pdf import sample_hdi, sample_hdi_batch

    s = g["tiny_257_sample"]
    out = quiet(sample_hdi_batch, s, hh.TINY_FRACTIONS)
    assert out.shape == (3, 2, 4)
    assert_array_equal(out, g["tiny_257_hdi"])
    one = quiet(sample_hdi_batch, s[:, 2], hh.TINY_FRACTIONS)
    assert one.shape == (3, 2)
    assert_array_equal(one, g["tiny_257_hdi"][:, :, 2])
    assert quiet(sample_hdi_batch, list(s[:, 1]), (0.5,)).shape == (1, 2)
    assert quiet(sample_hdi_batch, s, ()).shape == (0, 2, 4)
    # integers stay exact, and a generator of fractions is taken once
    ints = np.random.default_rng(3).integers(-2 ** 40, 2 ** 40, size=(50, 2))
    got = quiet(sample_hdi_batch, ints, (f for f in (0.3, 0.6)))
    assert_array_equal(got, np.stack([quiet(sample_hdi, ints, f) for f in (0.3, 0.6)]))
    assert len(host.calls) == 4  # (no fractions: no call)


def test_flagged_columns_are_recomputed_on_the_host(g, host):
    from inference_amd.pdf import sample_hdi_batch

    s = g["nf_small_sample"]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = sample_hdi_batch(s, hh.FRACTIONS)
    assert len(seen) == 2  # 40 - 26 and 40 - 38 are below 20: once per fraction, not once per recomputed column
    assert_array_equal(out, g["nf_small_hdi"])  # (the stand-in leaves -12345 in the flagged columns)
    assert len(host.calls) == 1


def test_hdi_plot_data(g, host):
    from inference_amd.pdf import _messages as msg
    from inference_amd.plotting import hdi_plot_data

    x = np.linspace(0.0, 1.0, 60)
    for name in ("band_a", "band_b"):
        s = hh.checked_case(g, name)
        for sample in (s, np.ascontiguousarray(s.T)):
            host.calls.clear()
            data = hdi_plot_data(x, sample, intervals=hh.BAND_INTERVALS)
            assert host.calls == [((400, 60), (380, 260, 140))]  # exactly one device call, highest interval first
            assert_array_equal(data["intervals"], [0.95, 0.65, 0.35])
            assert data["lower"].shape == data["upper"].shape == (3, 60)
            assert_array_equal(data["lower"], g[f"{name}_lower"])
            assert_array_equal(data["upper"], g[f"{name}_upper"])
    host.calls.clear()
    with pytest.raises(ValueError) as err:
        hdi_plot_data(x[:59], s, intervals=(0.5,))
    assert str(err.value) == msg.hdi_plot_dimensions() == '"x" and "sample" have incompatible dimensions'
    for bad in ((0.5, 1.0), (0.0, 0.5), (-0.1,), (1.2, 0.3)):
        with pytest.raises(ValueError) as err:
            hdi_plot_data(x, s, intervals=bad)
        assert str(err.value) == msg.hdi_plot_intervals()
    assert host.calls == []
    # a square sample is taken as (n, len(x))
    sq = np.random.default_rng(5).normal(size=(60, 60))
    data = hdi_plot_data(x, sq, intervals=(0.5,))
    assert_array_equal(data["lower"][0], quiet(hh.HostHdi(), sq, [30])[0][0, 0])


def test_trace_plot_data(g, host):
    from inference_amd.plotting import trace_plot_data

    S = hh.checked_case(g, "trace")
    data = trace_plot_data([row for row in S])
    assert host.calls == [((3000, 5), (2970, 300))]  # equal lengths: one call, both fractions
    assert data["limits"].shape == (5, 2) and data["ticks"].shape == (5, 3)
    assert_array_equal(data["limits"], g["trace_limits"])
    assert_array_equal(data["ticks"], g["trace_ticks"])
    host.calls.clear()
    data = trace_plot_data([list(s) for s in hh.checked_case(g, "ragged")])
    assert host.calls == [((n, 1), (int(0.99 * n), int(0.10 * n))) for n in hh.RAGGED]  # ragged: one call per sample
    assert_array_equal(data["limits"], g["ragged_limits"])
    assert_array_equal(data["ticks"], g["ragged_ticks"])


def test_trace_plot_labels(g, host):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from inference_amd.pdf import _messages as msg
    from inference_amd.plotting import trace_plot

    S = hh.checked_case(g, "trace")
    samples = [row for row in S]
    with pytest.raises(ValueError) as err:
        trace_plot(samples, labels=["a", "b"], show=False)
    assert str(err.value) == msg.trace_plot_labels() == "number of labels must match the number of plotted parameters"
    assert host.calls == []
    fig = trace_plot(samples, show=False)
    assert [ax.get_ylabel() for ax in fig.axes] == list(g["trace_labels"]) == [f"param {i}" for i in range(5)]
    assert_array_equal(np.array([ax.get_ylim() for ax in fig.axes]), g["trace_limits"])
    assert_array_equal(np.array([ax.get_yticks() for ax in fig.axes]), g["trace_ticks"])
    # the reference's layout: n = ceil(sqrt(N / 2)) columns, ceil(N / n) rows; the bottom row carries the x label
    assert [ax.get_subplotspec().get_gridspec().get_geometry() for ax in fig.axes] == [(3, 2)] * 5
    assert [ax.get_xlabel() for ax in fig.axes] == ["", "", "", "", "chain step #"]
    fig = trace_plot(samples * 2, show=False)
    assert [ax.get_ylabel() for ax in fig.axes] == [f"p{i}" for i in range(10)]
    fig = trace_plot(samples[:2], labels=["alpha", "beta"], show=False)
    assert [ax.get_ylabel() for ax in fig.axes] == ["alpha", "beta"]
    plt.close("all")


def test_hdi_plot_colormap_fallback_and_labels(g, host):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib import colormaps

    from inference_amd.pdf import _messages as msg
    from inference_amd.plotting import hdi_plot

    s = hh.checked_case(g, "band_a")
    x = np.linspace(0.0, 1.0, 60)
    _, ax = plt.subplots()
    with pytest.warns(UserWarning) as seen:
        assert hdi_plot(x, s, intervals=hh.BAND_INTERVALS, colormap="no such map", axis=ax) is ax
    assert [str(w.message) for w in seen] == [msg.matrix_plot_colormap("no such map")]
    assert [p.get_label() for p in ax.collections] == list(g["band_a_labels"]) == ["95% HDI", "65% HDI", "35% HDI"]
    levels = 255 * (0.8 * (1 - np.array([0.95, 0.65, 0.35])) + 0.2)
    for poly, level, lower, upper in zip(ax.collections, levels, g["band_a_lower"], g["band_a_upper"]):
        assert tuple(poly.get_facecolor()[0]) == colormaps["Blues"](int(level))
        v = poly.get_paths()[0].vertices
        assert_array_equal(v[1:61, 1], lower)
        assert_array_equal(v[62:122, 1][::-1], upper)
    ax2 = hdi_plot(x, s, intervals=(0.5, 0.9), colormap="Reds", label_intervals=False, color_levels=[10, 200])
    assert ax2 is not ax
    assert [tuple(p.get_facecolor()[0]) for p in ax2.collections] == [colormaps["Reds"](10), colormaps["Reds"](200)]
    assert all(p.get_label().startswith("_") for p in ax2.collections)
    plt.close("all")


def test_modules_import_without_matplotlib():
    code = ("import sys; sys.modules['matplotlib'] = None; sys.path[:0] = %r\n"
            "import inference_amd.plotting as p, inference_amd.pdf as d, inference_amd.mcmc as c\n"
            "assert callable(p.hdi_plot) and callable(p.trace_plot) and callable(d.sample_hdi_batch)\n"
            "assert 'matplotlib.pyplot' not in sys.modules\n"
            "print('ok')") % [p for p in sys.path if p.endswith("inference-tools_amd")]
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_chain_trace_plot_checks(g, host):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from inference_amd.mcmc import GibbsChain
    from inference_amd.pdf import _messages as msg

    chain = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(5), display_progress=False)
    with pytest.raises(ValueError) as err:
        chain.trace_plot(show=False)
    assert str(err.value) == msg.plot_no_samples("GibbsChain", "trace", chain.chain_length)
    S = hh.checked_case(g, "trace")
    for p, column in zip(chain.params, S):
        p.samples = list(column)
    chain.probs = list(-0.5 * np.sum(S ** 2, axis=0))
    chain.chain_length = S.shape[1]
    with pytest.raises(ValueError) as err:
        chain.trace_plot(burn=2999, thin=5, show=False)
    assert str(err.value) == msg.plot_burn_thin("GibbsChain", "trace", 1)
    assert host.calls == []
    fig = chain.trace_plot(show=False)
    assert_array_equal(np.array([ax.get_ylim() for ax in fig.axes]), g["trace_limits"])
    fig = chain.trace_plot(params=[4, 0], burn=1000, thin=4, show=False)
    assert host.calls[-1] == ((500, 2), (495, 50))
    assert len(fig.axes) == 2
    plt.close("all")


def test_no_silent_cpu_path():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from inference_amd import _lib
    from inference_amd.pdf import sample_hdi_batch
    from inference_amd.plotting import hdi_plot_data, trace_plot_data

    s = np.random.default_rng(0).normal(size=(50, 4))
    with pytest.raises(_lib.GpmiUnavailable):
        sample_hdi_batch(s, [0.5])
    with pytest.raises(_lib.GpmiUnavailable):
        hdi_plot_data(np.arange(4.0), s)
    with pytest.raises(_lib.GpmiUnavailable):
        trace_plot_data([s[:, 0], s[:, 1]])
