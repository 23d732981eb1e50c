"""
CPU tests of UnimodalPdf's host logic (inference_amd.pdf.unimodal) against the reference's values
(tests/golden/unimodal.npz, written by golden/make_golden_unimodal.py): the quadrature nodes, guesses, bounds and sample
moments, the model curve and its normalisation, the Nelder-Mead driving fed the recorded log-probabilities (teacher
forcing), the estimate built around the reference's MAP (`from_fit`: pdf, cdf, moments, intervals), the error texts, the
new C-ABI symbols and `plot_summary`.  No device call is made.  Every test prints the worst error it reached.
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ["gauss", "gamma", "t3", "logn", "big", "tiny"]
WORST = {}


def note(what, err):
    WORST[what] = max(WORST.get(what, 0.0), float(err))
    print(f"[unimodal] worst {what}: {WORST[what]:.3e}")


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    excess = np.abs(a - b) - (atol + rtol * np.abs(b))
    rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    note(what, rel[np.abs(b) > atol / max(rtol, 1e-300)].max(initial=0.0))
    assert (excess <= 0).all(), f"{what}: worst excess {excess.max():.3e} (rtol {rtol}, atol {atol})"


def samples():
    """The recipe of golden/make_golden_unimodal.py."""
    rng = np.random.default_rng(20261017)
    return {
        "gauss": rng.normal(1.0, 2.0, 1500),
        "gamma": rng.gamma(3.0, 1.0, 2000),
        "t3": rng.standard_t(3, 1800),
        "logn": rng.lognormal(0.0, 0.5, 5000),
        "big": rng.normal(-2.0, 0.7, 100_000),
        "tiny": rng.normal(0.0, 1.0, 30),
    }


def sample_of(g, prefix):
    s = g[f"{prefix}_sample"] if f"{prefix}_sample" in g else samples()[prefix]
    assert s.size == g[f"{prefix}_n"]
    np.testing.assert_array_equal(np.concatenate([s[:8], s[-8:]]), g[f"{prefix}_ends"])
    return s


def test_samples_regenerate(golden):
    g = golden("unimodal")
    drawn = samples()
    for prefix in CASES:
        s = sample_of(g, prefix)
        np.testing.assert_array_equal(drawn[prefix], s)
    assert "big_sample" not in g and g["big_skip"] == 50 and g["logn_skip"] == 2
    assert not g["t3_success"]


@pytest.mark.parametrize("prefix", CASES)
def test_guesses_bounds_moments_nodes(golden, prefix):
    from inference_amd.pdf.unimodal import chebyshev_nodes, guesses_and_bounds, sample_moments

    g = golden("unimodal")
    s = sample_of(g, prefix)
    fitted = s[:: int(g[f"{prefix}_skip"])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        guesses, bounds = guesses_and_bounds(s, fitted)
    assert len(guesses) == 72
    np.testing.assert_array_equal(np.array(guesses), g[f"{prefix}_guesses"])
    np.testing.assert_array_equal(np.array(bounds), g[f"{prefix}_bounds"])
    np.testing.assert_array_equal(np.array(sample_moments(fitted)), g[f"{prefix}_moments3"])
    u, w = chebyshev_nodes(128, 0.2)
    np.testing.assert_array_equal(u, g[f"{prefix}_u"])
    np.testing.assert_array_equal(w, g[f"{prefix}_w"])


@pytest.mark.parametrize("prefix", CASES)
def test_model_and_norm(golden, prefix):
    from inference_amd.pdf.unimodal import chebyshev_nodes, log_pdf_model, model_norm

    g = golden("unimodal")
    s = sample_of(g, prefix)
    u, w = chebyshev_nodes(128, 0.2)
    theta, stride = g[f"{prefix}_rec_theta"], g[f"{prefix}_rec_stride"]
    picks = np.unique(np.concatenate([np.arange(72), np.linspace(0, theta.shape[0] - 1, 60).astype(int)]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sums = [log_pdf_model(s[:: stride[i]], theta[i]).sum() for i in picks]
        norms = [model_norm(theta[i], u, w, 0.2) for i in picks]
    close(sums, g[f"{prefix}_rec_sum"][picks], 1e-12, 0.0, "sum of log_pdf_model")
    close(norms, g[f"{prefix}_rec_norm"][picks], 1e-12, 0.0, "norm")
    close(np.log(model_norm(g[f"{prefix}_MAP"], u, w, 0.2)), g[f"{prefix}_map_lognorm"], 1e-12, 0.0, "map_lognorm")
    assert log_pdf_model(theta[0][0], theta[0]) == 0.0  # z = 0: |0|^q = 0, the term is 0


def teacher(theta_rec, post_rec):
    """An objective that checks each request against the recorded sequence and answers with the recorded value."""
    calls = []
    pos = [0]

    def objective(thetas):
        calls.append(len(thetas))
        out = []
        for t in thetas:
            k = pos[0]
            assert k < theta_rec.shape[0], "more requests than the reference made"
            assert np.array_equal(np.asarray(t), theta_rec[k]), (k, t, theta_rec[k])
            out.append(post_rec[k])
            pos[0] += 1
        return out

    return objective, calls, pos


@pytest.mark.parametrize("prefix", CASES)
def test_fit_teacher_forced(golden, prefix):
    """The optimiser driving, the bounds and the two-pass logic against this machine's SciPy: the same requests, bit for
    bit, in the same number, and the same MAP."""
    from inference_amd.pdf.unimodal import fit

    g = golden("unimodal")
    objective, calls, pos = teacher(g[f"{prefix}_rec_theta"], g[f"{prefix}_rec_post"])
    switched = []
    skip = int(g[f"{prefix}_skip"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # SciPy's warning about a guess outside the bounds
        result = fit(list(g[f"{prefix}_guesses"]), [tuple(b) for b in g[f"{prefix}_bounds"]], skip, objective,
                     lambda: switched.append(pos[0]))
    assert pos[0] == g[f"{prefix}_rec_theta"].shape[0]
    assert calls[0] == 72 and set(calls[1:]) == {1}  # the guesses arrive as one batch
    np.testing.assert_array_equal(result.x, g[f"{prefix}_MAP"])
    assert bool(result.success) == bool(g[f"{prefix}_success"])
    stride = g[f"{prefix}_rec_stride"]
    if skip > 1:  # the second pass starts where the recorded requests switch to the full sample
        assert switched == [int(np.argmax(stride == 1))] and (stride[: switched[0]] == skip).all()
    else:
        assert switched == [] and (stride == 1).all()


def test_clipped_guess_warns(golden):
    """A guess for f outside (-3, 3) is clipped by SciPy with its warning (the reference's behaviour)."""
    from inference_amd.pdf.unimodal import fit

    guess = np.array([0.0, 1.0, 0.25, 4.5, 1.0, 2.0])
    bounds = [(-1.0, 1.0), (0.1, 10.0), (0.0, 5.0), (-3.0, 3.0), (1e-2, 20.0), (1.0, 6.0)]
    seen = []

    def objective(thetas):
        seen.extend(np.array(t) for t in thetas)
        return [-float(np.sum((np.asarray(t) - 0.5) ** 2)) for t in thetas]

    with pytest.warns(Warning, match="bounds"):
        fit([guess], bounds, 1, objective)
    assert seen[0][3] == 4.5 and all(t[3] <= 3.0 for t in seen[1:])


@pytest.mark.parametrize("prefix", CASES)
def test_from_fit_against_reference(golden, prefix):
    from inference_amd.pdf import UnimodalPdf

    g = golden("unimodal")
    s = sample_of(g, prefix)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pdf = UnimodalPdf.from_fit(s, g[f"{prefix}_MAP"])
    assert pdf._density is None and pdf.min_result is None
    np.testing.assert_array_equal(pdf.MAP, g[f"{prefix}_MAP"])
    assert pdf.mode == g[f"{prefix}_MAP"][0] and pdf.n_samps == s.size and pdf.skip == g[f"{prefix}_skip"]
    assert (pdf.sd, pdf.n_nodes, pdf.cutoff) == (0.2, 128, 2000)
    np.testing.assert_array_equal(np.array(pdf.bounds), g[f"{prefix}_bounds"])
    close(pdf.map_lognorm, g[f"{prefix}_map_lognorm"], 1e-12, 0.0, "map_lognorm")
    close([pdf.lwr_limit, pdf.upr_limit], g[f"{prefix}_limits"], 1e-12, 0.0, "limits")
    x = g[f"{prefix}_x"]
    assert x[0] < pdf.lwr_limit and x[-1] > pdf.upr_limit
    close(pdf(x), g[f"{prefix}_pdf"], 1e-12, 1e-300, "pdf")
    close(pdf.cdf(x), g[f"{prefix}_cdf"], 1e-12, 1e-15, "cdf")
    close(pdf.evaluate_model(x, pdf.MAP), g[f"{prefix}_pdf"], 1e-12, 1e-300, "evaluate_model")
    m, rm = np.array(pdf.moments()), g[f"{prefix}_moments"]
    err = (np.abs(m - rm) / np.maximum(np.abs(rm), 1.0)).max()
    note("moments", err)
    assert err <= 1e-10
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for f, (lo, hi) in zip(g[f"{prefix}_fractions"], g[f"{prefix}_intervals"]):
            a, b = pdf.interval(f)
            err = max(abs(a - lo), abs(b - hi)) / (hi - lo)
            note("interval / width", err)
            assert err <= 1e-8, (f, a, b, lo, hi)
    # scalar in, scalar out
    xs, ps, cs = g[f"{prefix}_scalar"]
    assert np.ndim(pdf(float(xs))) == 0 and np.ndim(pdf.cdf(float(xs))) == 0
    close(pdf(float(xs)), ps, 1e-12, 1e-300, "pdf of a scalar")
    close(pdf.cdf(float(xs)), cs, 1e-12, 1e-15, "cdf of a scalar")


def test_cdf_quirk_first_interval(golden):
    """The first interval of a batch is 0 below lwr_limit, the later ones integrate the true curve: the cdf of a batch
    that starts below lwr_limit is short of a single point's by the mass between its smallest point and lwr_limit."""
    from inference_amd.pdf import UnimodalPdf

    g = golden("unimodal")
    pdf = UnimodalPdf.from_fit(g["gamma_sample"], g["gamma_MAP"])
    below = pdf.lwr_limit - 1.0
    assert pdf.cdf(below) == 0.0
    x = np.array([below, pdf.mode])
    batch = pdf.cdf(x)
    assert batch[0] == 0.0 and batch[1] > pdf.cdf(pdf.mode)
    assert np.array_equal(pdf.cdf(x[::-1]), batch[::-1])  # the caller's order is restored


def test_error_texts(golden):
    from inference_amd.pdf import UnimodalPdf
    from inference_amd.pdf import _messages as msg

    g = golden("unimodal")
    pdf = UnimodalPdf.from_fit(g["gauss_sample"], g["gauss_MAP"])
    for fraction in (1.5, 0.0, -0.1):
        with pytest.raises(ValueError) as err:
            pdf.interval(fraction)
        assert str(err.value) == ("\n\n                \r[ UnimodalPdf error ]\n                \r>> The 'fraction' argument must "
                                  "have a value greater than\n                \r>> zero and less than one, but the value given "
                                  f"was {fraction}.\n                ")
    text = msg.marginal_unimodal()
    assert "UnimodalPdf(chain.get_parameter(index, burn, thin))" in text


def test_unimodal_abi_declared_and_bound():
    import re

    from inference_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    names = ["gpmi_unimodal_create", "gpmi_unimodal_destroy", "gpmi_unimodal_logpdf_sums"]
    assert "typedef struct gpmi_unimodal gpmi_unimodal;" in header
    assert "UnimodalPdf, inference/pdf/unimodal.py" in header
    for name in names:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_no_cpu_fallback():
    """Without a GPU the constructor raises GpmiUnavailable, and so does a posterior asked of a `from_fit` estimate."""
    from inference_amd import _lib
    from inference_amd.pdf import UnimodalPdf

    if _lib.device_count() == 0:
        s = np.random.default_rng(0).normal(size=200)
        with pytest.raises(_lib.GpmiUnavailable):
            UnimodalPdf(s)
        pdf = UnimodalPdf.from_fit(s, [0.0, 1.0, 1.0, 0.0, 1.0, 2.0])
        with pytest.raises(_lib.GpmiUnavailable):
            pdf.posterior(pdf.MAP)


def test_imports_without_matplotlib():
    code = ("import sys; sys.modules['matplotlib'] = None; sys.modules['matplotlib.pyplot'] = None\n"
            "import inference_amd.pdf as p\n"
            "assert p.UnimodalPdf.plot_summary is p.DensityEstimator.plot_summary\n"
            "assert p.GaussianKDE.plot_summary is p.DensityEstimator.plot_summary\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "inference-tools_amd")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_plot_summary_on_a_stub(tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from inference_amd.pdf import DensityEstimator
    from scipy.special import erf

    class Normal(DensityEstimator):
        sample = np.random.default_rng(4).normal(size=4000)
        mode = 0.0

        def __call__(self, x):
            return np.exp(-0.5 * np.asarray(x, float) ** 2) / np.sqrt(2 * np.pi)

        def cdf(self, x):
            return 0.5 * (1 + erf(np.asarray(x, float) / np.sqrt(2)))

        def moments(self):
            return 0.0, 1.0, 0.0, 0.0

    out = tmp_path / "summary.png"
    fig, ax = Normal().plot_summary(filename=str(out), show=False, label="x")
    assert isinstance(fig, plt.Figure) and len(ax) == 2 and out.stat().st_size > 0
    assert ax[0].get_xlabel() == "x" and ax[0].get_ylabel() == "probability density"
    texts = [t.get_text() for t in ax[1].texts]
    assert {"Basics", "Highest-density intervals", "Higher moments", "1-sigma:", "2-sigma:", "Kurtosis:"} <= set(texts)
    lo, hi = ax[0].lines[0].get_xdata()[[0, -1]]
    assert lo < -2.5 and hi > 2.5  # beyond the 2-sigma interval, out to 0.5 % of the peak
    plt.close(fig)
