"""
CPU tests of the density estimators' host logic (inference_amd.pdf) and of the GibbsChain read-out, against the
reference's values (tests/golden/kde.npz, written by golden/make_golden_kde.py): region tables and the region of every
evaluation point, the rule-of-thumb bandwidth, the bandwidth grid search fed the recorded log-probabilities (teacher
forcing), the cross-validation subsample and the generator state, sample_hdi, the chain's get_interval and mode, the
error texts, and the new C-ABI symbols.  No device call is made.
"""
import warnings

import numpy as np
import pytest

CASES_TABLE = ["bi", "bi_rt", "n3", "n8", "tie", "t2", "bw"]
SAMPLE_OF = {"bi_rt": "bi", "bw": "bi"}


def sample(g, prefix):
    return np.sort(g[f"{SAMPLE_OF.get(prefix, prefix)}_sample"])


@pytest.mark.parametrize("prefix", CASES_TABLE)
def test_region_table_and_lookup(golden, prefix):
    from inference_amd.pdf.kde import region_of, region_table

    g = golden("kde")
    s = sample(g, prefix)
    layers, edges, regions, lwr, upr = region_table(s, g[f"{prefix}_h"])
    np.testing.assert_array_equal(edges, g[f"{prefix}_edges"])
    np.testing.assert_array_equal(lwr, g[f"{prefix}_lwr"])
    np.testing.assert_array_equal(upr, g[f"{prefix}_upr"])
    assert edges.size == 2**layers + 1
    x = g[f"{prefix}_x"]
    assert np.isin(g[f"{prefix}_edges"], x).sum() >= min(edges.size, 150)  # points exactly on edges are covered
    np.testing.assert_array_equal(region_of(edges, regions, x), g[f"{prefix}_regions"])


def test_many_regions(golden):
    g = golden("kde")
    assert g["t2_lwr"].size >= 256


@pytest.mark.parametrize("prefix", ["bi_rt", "n3", "n8", "t2"])
def test_rule_of_thumb_bandwidth(golden, prefix):
    from inference_amd.pdf.kde import rule_of_thumb_bandwidth

    g = golden("kde")
    assert rule_of_thumb_bandwidth(sample(g, prefix)) == g[f"{prefix}_h"]


def teacher(widths_rec, logp_rec):
    """An objective that checks each request against the recorded sequence and answers with the recorded value."""
    calls = []
    pos = [0]

    def objective(widths):
        calls.append(len(widths))
        out = []
        for w in widths:
            k = pos[0]
            assert k < widths_rec.size, "more requests than the reference made"
            assert w == widths_rec[k] or (np.isinf(w) and np.isinf(widths_rec[k])), (k, w, widths_rec[k])
            out.append(logp_rec[k])
            pos[0] += 1
        return out

    return objective, calls, pos


@pytest.mark.parametrize("prefix", ["bi", "tie", "big"])
def test_grid_search_teacher_forced(golden, prefix):
    from inference_amd.pdf.kde import cv_bandwidth_search, rule_of_thumb_bandwidth

    g = golden("kde")
    s = sample(g, prefix)
    objective, calls, pos = teacher(g[f"{prefix}_cv_widths"], g[f"{prefix}_cv_logp"])
    h = cv_bandwidth_search(rule_of_thumb_bandwidth(s), objective)
    assert pos[0] == g[f"{prefix}_cv_widths"].size
    assert calls[0] == 5 and calls[-6:] == [2] * 6 and set(calls[1:-6]) <= {1}
    assert h == g[f"{prefix}_h"]


def test_grid_search_overflow_case(golden):
    """Two clusters 1e4 apart: every width is inf, the log-probabilities NaN, the search returns inf after 22
    requests, and building the region table raises the reference's OverflowError."""
    from inference_amd.pdf import GaussianKDE
    from inference_amd.pdf.kde import cv_bandwidth_search, region_table, rule_of_thumb_bandwidth

    g = golden("kde")
    s = np.sort(g["ovf_sample"])
    assert g["ovf_cv_widths"].size == 22 and np.isnan(g["ovf_cv_logp"]).all()
    objective, calls, pos = teacher(g["ovf_cv_widths"], g["ovf_cv_logp"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = cv_bandwidth_search(rule_of_thumb_bandwidth(s), objective)
        assert np.isinf(h) and pos[0] == 22
        with pytest.raises(OverflowError, match=str(g["ovf_error"])):
            region_table(s, h)
        # the whole class: inf widths are answered without the device, so this holds with or without a GPU
        with pytest.raises(OverflowError, match=str(g["ovf_error"])):
            GaussianKDE(g["ovf_sample"], cross_validation=True)


def test_grid_search_quirks():
    """A maximum at the left edge makes the refinement read log_h[-1]; one at the right edge raises IndexError."""
    from inference_amd.pdf.kde import cv_bandwidth_search

    seen = []

    def left(widths):
        seen.extend(np.log(widths))
        return [-np.log(w) for w in widths]  # increasing towards small widths: the maximum stays at the left edge

    cv_bandwidth_search(0.0, left)
    first_refine = seen[10]
    assert first_refine == pytest.approx(0.5 * (1.0 + (-3.5)))  # 0.5 * (log_h[-1] + log_h[0]): the grid is [-3.5 .. 1]
    with pytest.raises(IndexError):
        cv_bandwidth_search(0.0, lambda widths: list(np.log(widths)))


def test_subsample_and_generator_state(golden):
    from inference_amd.pdf.kde import cv_bandwidth_search, cv_subsample, rule_of_thumb_bandwidth

    g = golden("kde")
    np.random.seed(7)
    big = np.concatenate([np.random.normal(0.0, 1.0, 12000), np.random.normal(4.0, 0.5, 8000)])
    np.testing.assert_array_equal(big, g["big_sample"])
    s = np.sort(big)
    sub = cv_subsample(s, 5000)
    np.testing.assert_array_equal(sub, s[g["big_subsample"]])
    objective, _, _ = teacher(g["big_cv_widths"], g["big_cv_logp"])
    assert cv_bandwidth_search(rule_of_thumb_bandwidth(s), objective) == g["big_h"]
    np.testing.assert_array_equal(np.random.random(3), g["big_draws"])
    assert cv_subsample(s, 20000) is s


def test_sample_hdi(golden):
    from inference_amd.pdf import sample_hdi

    g = golden("kde")
    np.testing.assert_array_equal(sample_hdi(g["chain_samples"], 0.68), g["hdi_2d"])
    np.testing.assert_array_equal(sample_hdi(list(g["chain_samples"][:, 1]), 0.9), g["hdi_1d"])


def test_sample_hdi_warnings_and_errors():
    from inference_amd.pdf import sample_hdi
    from inference_amd.pdf import _messages as msg

    with pytest.warns(UserWarning) as rec:
        sample_hdi(np.arange(10.0), 0.95)
    assert str(rec[0].message) == ("\n\n            \r[ sample_hdi warning ]\n            \r>> n_samples * (1 - fraction) "
                                   "is small - calculated interval may be inaccurate.\n            ")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sample_hdi(np.arange(100.0), 0.5)  # no warning
    cases = [
        ((np.zeros(5), 1.5), "\n\n            \r[ sample_hdi error ]\n            \r>> The 'fraction' argument must be a float "
                             "between 0 and 1,\n            \r>> but the value given was 1.5.\n            "),
        ((5.0, 0.5), "\n\n            \r[ sample_hdi error ]\n            \r>> The 'sample' argument should be a numpy.ndarray "
                     "or a\n            \r>> Sequence which can be converted to an array, but\n            \r>> instead has "
                     "type <class 'float'>.\n            "),
        ((np.zeros((2, 2, 2)), 0.5), "\n\n            \r[ sample_hdi error ]\n            \r>> The 'sample' argument should "
                                     "be a numpy.ndarray\n            \r>> with either one or two dimensions, but the given\n"
                                     "            \r>> array has dimensionality 3.\n            "),
        ((np.zeros(1), 0.5), "\n\n            \r[ sample_hdi error ]\n            \r>> The first dimension of the given 'sample' "
                             "array must \n            \r>> have have a length of at least 2.\n            "),
    ]
    for args, text in cases:
        with pytest.raises(ValueError) as err:
            sample_hdi(*args)
        assert str(err.value) == text
    assert "insufficient" in msg.hdi_insufficient()


def test_error_texts():
    from inference_amd.pdf import DensityEstimator, GaussianKDE

    with pytest.raises(ValueError) as err:
        GaussianKDE([1.0, 2.0])
    assert str(err.value) == ("\n\n                \r[ GaussianKDE error ]\n                \r>> Not enough samples were given "
                              "to estimate the PDF.\n                \r>> At least 3 samples are required.\n                ")

    class Flat(DensityEstimator):
        sample = np.linspace(0.0, 1.0, 100)
        mode = 0.5

        def __call__(self, x):
            return np.ones_like(np.asarray(x, float))

        def cdf(self, x):
            return np.clip(np.asarray(x, float), 0.0, 1.0)

        def moments(self):
            return 0.5, 1 / 12, 0.0, -1.2

    with pytest.raises(ValueError) as err:
        Flat().interval(1.5)
    assert str(err.value) == ("\n\n                \r[ Flat error ]\n                \r>> The 'fraction' argument must have a "
                              "value greater than\n                \r>> zero and less than one, but the value given was 1.5."
                              "\n                ")
    lo, hi = Flat().interval(0.5)  # the host search on a uniform density: any interval of width 0.5 inside [0, 1]
    assert hi - lo == pytest.approx(0.5, abs=1e-3) and -1e-3 <= lo and hi <= 1 + 1e-3


def make_chain(g):
    from inference_amd.mcmc import GibbsChain

    chain = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(3))
    S, P = g["chain_samples"], g["chain_probs"]
    for i, p in enumerate(chain.params):
        p.samples = list(S[:, i])
    chain.probs = list(P)
    chain.chain_length = len(P)
    return chain


def test_chain_get_interval_and_mode(golden):
    g = golden("kde")
    chain = make_chain(g)
    np.testing.assert_array_equal(chain.mode(), g["chain_mode"])
    k = 0
    while f"chain_iv{k}_args" in g:
        iv, burn, thin, samples = g[f"chain_iv{k}_args"]
        np.random.seed(100 + k)
        smp, prb = chain.get_interval(interval=iv, burn=int(burn), thin=int(thin),
                                      samples=None if samples < 0 else int(samples))
        np.testing.assert_array_equal(smp, g[f"chain_iv{k}_sample"])
        np.testing.assert_array_equal(prb, g[f"chain_iv{k}_probs"])
        np.testing.assert_array_equal(np.random.random(2), g[f"chain_iv{k}_draw"])
        k += 1
    assert k == 5


def test_chain_marginal_unimodal_not_provided(golden):
    chain = make_chain(golden("kde"))
    with pytest.raises(NotImplementedError, match="UnimodalPdf"):
        chain.get_marginal(0, unimodal=True)


def test_kde_abi_declared_and_bound():
    import ctypes
    import os
    import re

    from inference_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gpmi.h")).read()
    names = ["gpmi_kde_create", "gpmi_kde_destroy", "gpmi_kde_eval", "gpmi_kde_cv_logprob"]
    assert "typedef struct gpmi_kde gpmi_kde;" in header
    for name in names:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ctypes.CDLL(_lib.LIB_PATH).gpmi_version() == 100


def test_no_cpu_fallback():
    """Without a GPU a density that needs the device raises GpmiUnavailable; the checks before it run anyway."""
    from inference_amd import _lib
    from inference_amd.pdf import GaussianKDE

    with pytest.raises(ValueError):
        GaussianKDE(np.zeros(2))
    if _lib.device_count() == 0:
        with pytest.raises(_lib.GpmiUnavailable):
            GaussianKDE(np.linspace(0.0, 1.0, 50))
        with pytest.raises(_lib.GpmiUnavailable):
            GaussianKDE(np.linspace(0.0, 1.0, 50), cross_validation=True)


def test_one_handle_per_device(monkeypatch):
    """`device=None` resolves to the default device before the lookup: GaussianKDE(s) and GaussianKDE(s, device=d) for
    that d share one handle, and every handle carries the lock that serialises its density calls."""
    from inference_amd import _lib
    from inference_amd.pdf import _device

    made = []

    class FakeHandle:
        def __init__(self, device):
            made.append(device)
            self.ctx = 1

    monkeypatch.setattr(_lib, "Handle", FakeHandle)
    monkeypatch.setattr(_device, "_handles", {})
    monkeypatch.setenv("GPMI_DEVICE", "0")
    d = _device.resolve_device(None)
    assert d == _lib.default_device() == 0
    h = _device.handle()
    assert _device.handle(0) is h and _device.handle(None) is h and made == [0]
    assert hasattr(h.kde_lock, "acquire")
    h.ctx = 0  # closed: the next lookup opens a new handle
    assert _device.handle(0) is not h and made == [0, 0]
