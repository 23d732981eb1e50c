"""
Host logic of inference_amd.pdf.KDE2D, inference_amd.plotting and GibbsChain.matrix_plot without a GPU: the class runs with
its raw-sum seam filled by NumPy (tests/kde2d_host.py), against the reference's values (tests/golden/kde2d.npz, written
by golden/make_golden_kde2d.py).
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import kde2d_host as kh

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DENSITY_CASES = ["corr", "banana", "tiny", "ties", "shift"]


def note(what, err):
    print(f"[kde2d cpu] worst {what}: {float(err):.3e}")


@pytest.fixture
def host_plotting(monkeypatch):
    """inference_amd.plotting with both estimators on NumPy sums."""
    from inference_amd import plotting
    from inference_amd.pdf import _device

    monkeypatch.setattr(plotting, "KDE2D", kh.HostKDE2D)
    monkeypatch.setattr(_device, "DeviceDensity", kh.HostDensity1D)
    return plotting


@pytest.mark.parametrize("prefix", DENSITY_CASES)
def test_scales_bit_equal_and_densities(golden, prefix):
    g = golden("kde2d")
    pdf = kh.HostKDE2D(g[f"{prefix}_x"], g[f"{prefix}_y"])
    assert pdf.q_x == g[f"{prefix}_q_x"] and pdf.q_y == g[f"{prefix}_q_y"] and pdf.norm == g[f"{prefix}_norm"]
    s_x, s_y = pdf.estimate_bandwidth(pdf.x, pdf.y)
    assert 1.0 / (np.sqrt(2) * s_x) == pdf.q_x and 1.0 / (np.sqrt(2) * s_y) == pdf.q_y
    n = pdf.x.size
    # the host logic around the seam reproduces the reference (the NumPy sums are the reference's own arithmetic)
    kh.density_close(pdf(g[f"{prefix}_px"], g[f"{prefix}_py"]), g[f"{prefix}_pdf"], n, pdf.norm, "scattered", note)
    kh.density_close(pdf.grid(g[f"{prefix}_gx"], g[f"{prefix}_gy"]), g[f"{prefix}_grid"], n, pdf.norm, "grid", note)
    kh.density_close(pdf.at_samples(), g[f"{prefix}_self"], n, pdf.norm, "at samples", note)


def test_call_forms(golden):
    g = golden("kde2d")
    pdf = kh.HostKDE2D(g["corr_x"], g["corr_y"])
    px, py = g["corr_px"], g["corr_py"]
    one = pdf(float(px[3]), float(py[3]))
    assert np.ndim(one) == 0 and isinstance(one, float)
    kh.density_close(one, g["calls_scalar"], 3000, pdf.norm, "scalar call", note)
    assert pdf.density(float(px[3]), float(py[3])) == one
    kh.HostKDE2D.calls = 0
    many = pdf(list(px[:7]), list(py[:7]))
    assert kh.HostKDE2D.calls == 1  # one call of the seam per __call__, not one per point
    assert isinstance(many, list) and len(many) == 7 and all(isinstance(v, float) for v in many)
    kh.density_close(many, g["calls_list"], 3000, pdf.norm, "list call", note)
    short = pdf(px[:9], py[:5])
    assert isinstance(short, list) and len(short) == 5
    kh.density_close(short, g["calls_unequal"], 3000, pdf.norm, "zip truncation", note)
    assert pdf(iter(px[:3]), (v for v in py[:3])) == many[:3]  # any iterables
    assert pdf([], []) == [] and pdf(px[:4], []) == []
    assert pdf.grid(px[:3], py[:2]).shape == (2, 3) and pdf.grid([], py[:2]).shape == (2, 0)
    X, Y = np.meshgrid(px[:3], py[:2])
    assert np.array_equal(pdf.grid(px[:3], py[:2]), np.array(pdf(X.flatten(), Y.flatten())).reshape(2, 3))
    assert np.array_equal(pdf.at_samples()[:50], np.array(pdf(pdf.x[:50], pdf.y[:50])))


def test_degenerate_is_nan_without_the_device(golden, monkeypatch):
    from inference_amd.pdf import KDE2D, _device

    def forbidden(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_device, "DeviceDensity2D", forbidden)
    monkeypatch.setattr(_device, "handle", forbidden)
    g = golden("kde2d")
    xd = g["degenerate_x"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pdf = KDE2D(xd, 2 * xd)  # the product class itself
    got = np.array([pdf.q_x, pdf.q_y, pdf.norm])
    assert np.array_equal(got, g["degenerate_scales"], equal_nan=True) and pdf.degenerate
    vals = pdf(xd[:20] + 0.1, 2 * xd[:20])
    assert isinstance(vals, list) and len(vals) == 20 and np.isnan(vals).all()
    assert np.isnan(pdf(0.1, 0.3)) and np.isnan(pdf.density(0.1, 0.3)) and np.isnan(g["degenerate_scalar"])
    assert pdf.grid(xd[:4], xd[:3]).shape == (3, 4) and np.isnan(pdf.grid(xd[:4], xd[:3])).all()
    assert pdf.at_samples().shape == xd.shape and np.isnan(pdf.at_samples()).all()


def test_value_errors():
    x = np.linspace(0.0, 1.0, 10)
    for bad in ((x, x[:9]), (x.reshape(2, 5), x.reshape(2, 5)), (x[:1], x[:1]), (3.0, 4.0), (x, x.reshape(10, 1)), ([], [])):
        with pytest.raises(ValueError, match="KDE2D error"):
            kh.HostKDE2D(*bad)
    pdf = kh.HostKDE2D(x, x**2)
    with pytest.raises(ValueError, match="KDE2D error"):
        pdf.grid(x.reshape(2, 5), x)
    with pytest.raises(ValueError, match="KDE2D error"):
        pdf(x[:3], 0.5)  # one iterable only: not a single point
    with pytest.raises(ValueError, match="KDE2D error"):
        pdf.density(x[:3], x[:3])


def test_no_device_means_unavailable():
    """Without a GPU the product class fails loudly at construction, as GaussianKDE does."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from inference_amd import _lib
    from inference_amd.pdf import KDE2D

    rng = np.random.default_rng(0)
    with pytest.raises(_lib.GpmiUnavailable):
        KDE2D(rng.normal(size=10), rng.normal(size=10))


@pytest.mark.parametrize("style", ["contour", "hdi"])
def test_matrix_plot_data_against_reference(golden, host_plotting, style):
    g = golden("kde2d")
    data = host_plotting.matrix_plot_data(list(g["mp_samples"]), plot_style=style,
                                          hdi_fractions=tuple(g["mp_hdi_fractions"]))
    kh.check_matrix_plot_data(data, g, style, note)


def test_matrix_plot_data_without_densities(golden, host_plotting):
    g = golden("kde2d")
    for style in ("histogram", "scatter"):
        data = host_plotting.matrix_plot_data(list(g["mp_samples"][:2]), plot_style=style)
        assert data["pairs"] == {} and data["marginals"].shape == (2, 200)
    with pytest.raises(ValueError):
        host_plotting.matrix_plot_data(list(g["mp_samples"][:2]), plot_style="violin")
    with pytest.raises(ValueError, match="hdi_fractions"):
        host_plotting.matrix_plot_data(list(g["mp_samples"][:2]), hdi_fractions=(0.5, 1.0))


def test_plotting_imports_without_matplotlib():
    code = ("import sys; sys.modules['matplotlib'] = None; sys.modules['matplotlib.pyplot'] = None\n"
            "import inference_amd, inference_amd.plotting, inference_amd.mcmc, inference_amd.pdf\n"
            "assert callable(inference_amd.plotting.matrix_plot) and callable(inference_amd.plotting.matrix_plot_data)\n"
            "print('ok')")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "inference-tools_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_matrix_plot_argument_checks(host_plotting):
    """The checks that come before any figure: they need neither matplotlib nor a density."""
    rng = np.random.default_rng(1)
    samples = [rng.normal(size=300) for _ in range(3)]
    mp = host_plotting.matrix_plot
    with pytest.raises(ValueError, match="number of labels"):
        mp(samples, labels=["a", "b"], show=False)
    with pytest.raises(ValueError, match="number of reference values"):
        mp(samples, reference=[0.0, 1.0], show=False)
    for bad in (0.5, (0.5, 1.0), (0.0, 0.5), [1.5]):
        with pytest.raises(ValueError, match="hdi_fractions"):
            mp(samples, hdi_fractions=bad, show=False)


def test_matrix_plot_warns_and_falls_back(host_plotting):
    pytest.importorskip("matplotlib")
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    rng = np.random.default_rng(2)
    samples = [rng.normal(size=300), rng.normal(size=300) ** 2]
    with pytest.warns(UserWarning, match="'plot_style' must be set as either"):
        fig = host_plotting.matrix_plot(samples, plot_style="violin", show=False)
    assert len(fig.axes) == 3
    plt.close(fig)
    with pytest.warns(UserWarning, match="'NoSuchMap' is not a valid colormap"):
        fig = host_plotting.matrix_plot(samples, colormap="NoSuchMap", plot_style="scatter", show=False)
    plt.close(fig)
    for style in ("contour", "hdi", "histogram", "scatter"):
        fig = host_plotting.matrix_plot(samples, labels=["u", "v"], reference=[0.0, 1.0], plot_style=style, show=False,
                                        show_ticks=(style == "hdi"))
        assert len(fig.axes) == 3
        assert sorted(ax.get_xlabel() for ax in fig.axes) == ["", "u", "v"]
        assert sorted(ax.get_ylabel() for ax in fig.axes) == ["", "", "v"]
        plt.close(fig)


def test_chain_matrix_plot_checks():
    """GibbsChain.matrix_plot: the burn / thin checks of the reference (mcmc/base.py:218-237) come before any plotting."""
    from inference_amd.mcmc import GibbsChain

    chain = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(3),
                       display_progress=False)
    with pytest.raises(ValueError, match="no samples have"):
        chain.matrix_plot(show=False)
    S = np.random.default_rng(4).normal(size=(100, 3))
    for i, p in enumerate(chain.params):
        p.samples = list(S[:, i])
    chain.probs = list(-0.5 * np.sum(S**2, axis=1))
    chain.chain_length = 100
    with pytest.raises(ValueError, match="Number of samples after burn / thin is 1"):
        chain.matrix_plot(burn=99, show=False)
    with pytest.raises(ValueError, match="leave insufficient"):
        chain.matrix_plot(thin=100, show=False)
