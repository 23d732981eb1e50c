"""
GPU tests of the device density estimator (inference_amd.pdf.GaussianKDE over csrc/kde.hip) against the reference's
values (tests/golden/kde.npz, written by golden/make_golden_kde.py), against NumPy sums over the same slices, run
against run, and through the GibbsChain read-out.  Every test prints the worst error it reached per quantity.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import erf

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WORST = {}


def note(what, err):
    WORST[what] = max(WORST.get(what, 0.0), float(err))
    print(f"[kde] worst {what}: {WORST[what]:.3e}")


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    excess = np.abs(a - b) - (atol + rtol * np.abs(b))
    rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    note(what, rel[np.abs(b) > atol / max(rtol, 1e-300)].max(initial=0.0))
    assert (excess <= 0).all(), f"{what}: worst excess {excess.max():.3e} (rtol {rtol}, atol {atol})"


CASES = {  # prefix -> (sample key, constructor keywords)
    "bi": ("bi", dict(cross_validation=True)),
    "bi_rt": ("bi", {}),
    "n3": ("n3", {}),
    "n8": ("n8", {}),
    "tie": ("tie", dict(cross_validation=True)),
    "t2": ("t2", {}),
    "bw": ("bi", dict(bandwidth=0.37)),
}


def numpy_sums(s, lo, hi, q, x, r):
    pdf = np.empty(x.size)
    cdf = np.empty(x.size)
    for i, (xi, ri) in enumerate(zip(x, r)):
        t = (xi - s[lo[ri]:hi[ri]]) * q
        pdf[i] = np.exp(-(t * t)).sum()
        cdf[i] = (1 + erf(t)).sum()
    return pdf, cdf


@pytest.mark.parametrize("prefix", list(CASES))
def test_against_reference(golden, prefix):
    from inference_amd.pdf import GaussianKDE

    g = golden("kde")
    key, kw = CASES[prefix]
    kde = GaussianKDE(g[f"{key}_sample"], **kw)
    assert kde.h == g[f"{prefix}_h"]  # bit-equal, after cross-validation too
    x = g[f"{prefix}_x"]
    close(kde(x), g[f"{prefix}_pdf"], 1e-12, 1e-300, "pdf")
    close(kde.cdf(x), g[f"{prefix}_cdf"], 1e-12, 1e-15, "cdf")
    span = kde.sample[-1] - kde.sample[0]
    err = abs(kde.mode - g[f"{prefix}_mode"]) / span
    note("mode / sample range", err)
    assert err <= 1e-9
    m, rm = np.array(kde.moments()), g[f"{prefix}_moments"]
    err = (np.abs(m - rm) / np.maximum(np.abs(rm), 1.0)).max()
    note("moments", err)
    assert err <= 1e-10
    for f, (lo, hi) in zip(g[f"{prefix}_fractions"], g[f"{prefix}_intervals"]):
        a, b = kde.interval(f)
        err = max(abs(a - lo), abs(b - hi)) / (hi - lo)
        note("interval / width", err)
        assert err <= 1e-8, (f, a, b, lo, hi)
    # scalar in, scalar out
    assert np.ndim(kde(float(x[7]))) == 0 and kde(float(x[7])) == kde(x)[7]
    assert np.ndim(kde.cdf(float(x[7]))) == 0


@pytest.mark.parametrize("prefix", ["bi", "tie", "big"])
def test_cv_logprobs(golden, prefix):
    from inference_amd.pdf import _device

    g = golden("kde")
    s = np.sort(g[f"{prefix}_sample"])
    if prefix == "big":
        s = s[g["big_subsample"]]
    w, lp = g[f"{prefix}_cv_widths"], g[f"{prefix}_cv_logp"]
    got = _device.cv_logprob(s, w)
    close(got, lp, 1e-11, 0.0, "CV log-prob")
    # one width at a time gives the same bits as the batch (the grid search asks for 5, 1 and 2 at a time)
    for k in (0, 7, w.size - 1):
        assert _device.cv_logprob(s, w[k:k + 1])[0] == got[k]


def test_cv_seeded_subsample(golden):
    from inference_amd.pdf import GaussianKDE

    g = golden("kde")
    np.random.seed(7)
    big = np.concatenate([np.random.normal(0.0, 1.0, 12000), np.random.normal(4.0, 0.5, 8000)])
    kde = GaussianKDE(big, cross_validation=True)
    assert kde.h == g["big_h"]
    np.testing.assert_array_equal(np.random.random(3), g["big_draws"])
    err = abs(kde.mode - g["big_mode"]) / (kde.sample[-1] - kde.sample[0])
    note("mode / sample range", err)
    assert err <= 1e-9


def test_million_samples_against_numpy():
    from inference_amd.pdf import GaussianKDE

    rng = np.random.default_rng(12345)
    s = np.concatenate([rng.normal(0.0, 1.0, 600_000), rng.normal(3.0, 0.4, 400_000)])
    kde = GaussianKDE(s)
    x = np.concatenate([rng.uniform(kde.sample[0] - 1, kde.sample[-1] + 1, 250), kde.edges[::97][:50]])
    r = kde.regions[np.searchsorted(kde.edges, x)]
    pdf, cdf = numpy_sums(kde.sample, kde.lwr_inds, kde.upr_inds, kde.q, x, r)
    close(kde(x), pdf * kde.norm, 1e-12, 1e-300, "pdf n=1e6 vs NumPy")
    close(kde.cdf(x), (0.5 / s.size) * cdf + kde.cdf_offsets[r], 1e-12, 1e-15, "cdf n=1e6 vs NumPy")
    # run against run, batch against single points, pdf + cdf together against apart
    x2 = rng.uniform(-3, 5, 10_000)
    p1, c1 = kde(x2), kde.cdf(x2)
    assert np.array_equal(p1, kde(x2)) and np.array_equal(c1, kde.cdf(x2))
    P, F = kde._pdf_and_cdf(x2)
    assert np.array_equal(P, p1) and np.array_equal(F, c1)
    for k in (0, 4321, 9999):
        assert kde(x2[k]) == p1[k] and kde.cdf(x2[k]) == c1[k]


def test_cv_repeatable():
    from inference_amd.pdf import _device

    s = np.random.default_rng(3).normal(size=30_000)
    w = [0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2, 6.4, 12.8]  # more than one launch of 8 widths
    a = _device.cv_logprob(s, w)
    assert np.array_equal(a, _device.cv_logprob(s, w))
    assert np.array_equal(a, _device.cv_logprob(s[::-1].copy(), w))  # the device sorts its copy
    # against a NumPy evaluation of the same formula on a subset
    t = s[:3000]
    d = t[:, None] - t[None, :]
    for h, got in zip(w[:3], _device.cv_logprob(t, w[:3])):
        S = np.exp(-0.5 * (d / h) ** 2).sum(axis=1)
        ref = np.sum(np.log(S) - np.log(h * t.size * np.sqrt(2 * np.pi)) + np.log(1 - 0.99 / S))
        close(got, ref, 1e-11, 0.0, "CV log-prob vs NumPy")


def test_tiny_and_many_regions():
    from inference_amd.pdf import GaussianKDE

    kde = GaussianKDE([0.0, 1.0, 5.0])
    x = np.linspace(-3, 8, 101)
    r = kde.regions[np.searchsorted(kde.edges, x)]
    pdf, cdf = numpy_sums(kde.sample, kde.lwr_inds, kde.upr_inds, kde.q, x, r)
    close(kde(x), pdf * kde.norm, 1e-12, 1e-300, "pdf n=3")
    close(kde.cdf(x), (0.5 / 3) * cdf + kde.cdf_offsets[r], 1e-12, 1e-15, "cdf n=3")
    # Cauchy: a long tail, thousands of regions
    s = np.random.default_rng(5).standard_cauchy(200_000)
    kde = GaussianKDE(s)
    assert kde.lwr_inds.size >= 4096
    x = np.concatenate([np.random.default_rng(6).normal(0, 3, 300), kde.edges[:: kde.edges.size // 100]])
    r = kde.regions[np.searchsorted(kde.edges, x)]
    pdf, cdf = numpy_sums(kde.sample, kde.lwr_inds, kde.upr_inds, kde.q, x, r)
    close(kde(x), pdf * kde.norm, 1e-12, 1e-300, "pdf many regions")
    close(kde.cdf(x), (0.5 / s.size) * cdf + kde.cdf_offsets[r], 1e-12, 1e-15, "cdf many regions")


def test_abi_error_returns():
    from inference_amd import _lib
    from inference_amd.pdf import _device

    h = _device.handle()
    lib = h.lib
    ERR = -1
    s = np.linspace(0.0, 1.0, 10)
    lo = np.array([0, 2], dtype=np.int64)
    hi = np.array([5, 10], dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    out = C.c_void_p()
    assert lib.gpmi_kde_create(h.ctx, 10, None, 2, i64(lo), i64(hi), C.byref(out)) == ERR
    assert lib.gpmi_kde_create(h.ctx, 0, _lib.dptr(s), 2, i64(lo), i64(hi), C.byref(out)) == ERR
    assert lib.gpmi_kde_create(h.ctx, 10, _lib.dptr(s), 0, i64(lo), i64(hi), C.byref(out)) == ERR
    bad = np.array([5, 11], dtype=np.int64)
    assert lib.gpmi_kde_create(h.ctx, 10, _lib.dptr(s), 2, i64(lo), i64(bad), C.byref(out)) == ERR
    assert lib.gpmi_kde_create(h.ctx, 10, _lib.dptr(s), 2, i64(hi), i64(lo), C.byref(out)) == ERR
    assert lib.gpmi_kde_create(None, 10, _lib.dptr(s), 2, i64(lo), i64(hi), C.byref(out)) == ERR
    assert lib.gpmi_kde_create(h.ctx, 10, _lib.dptr(s), 2, i64(lo), i64(hi), C.byref(out)) == 0
    x = np.array([0.5, 0.7])
    r = np.array([0, 1], dtype=np.int64)
    ps, cs = np.empty(2), np.empty(2)
    assert lib.gpmi_kde_eval(out, 2, _lib.dptr(x), i64(r), 2.0, None, None) == ERR
    assert lib.gpmi_kde_eval(out, 2, None, i64(r), 2.0, _lib.dptr(ps), None) == ERR
    assert lib.gpmi_kde_eval(out, -1, _lib.dptr(x), i64(r), 2.0, _lib.dptr(ps), None) == ERR
    for q in (0.0, -1.0, np.inf, np.nan):
        assert lib.gpmi_kde_eval(out, 2, _lib.dptr(x), i64(r), q, _lib.dptr(ps), None) == ERR
    rbad = np.array([0, 2], dtype=np.int64)
    assert lib.gpmi_kde_eval(out, 2, _lib.dptr(x), i64(rbad), 2.0, _lib.dptr(ps), None) == ERR
    assert lib.gpmi_kde_eval(None, 2, _lib.dptr(x), i64(r), 2.0, _lib.dptr(ps), None) == ERR
    assert lib.gpmi_kde_eval(out, 2, _lib.dptr(x), i64(r), 2.0, _lib.dptr(ps), _lib.dptr(cs)) == 0
    ref_p, ref_c = numpy_sums(s, lo, hi, 2.0, x, r)
    close(ps, ref_p, 1e-12, 1e-300, "pdf ABI")
    close(cs, ref_c, 1e-12, 1e-15, "cdf ABI")
    assert lib.gpmi_kde_destroy(out) == 0
    assert lib.gpmi_kde_destroy(None) == ERR
    lp = np.empty(2)
    for w in ([0.1, np.inf], [0.1, -1.0], [0.1, 0.0], [np.nan, 0.1]):
        w = np.array(w)
        assert lib.gpmi_kde_cv_logprob(h.ctx, 10, _lib.dptr(s), 2, _lib.dptr(w), 0.99, _lib.dptr(lp)) == ERR
    w = np.array([0.1, 0.2])
    assert lib.gpmi_kde_cv_logprob(h.ctx, 0, _lib.dptr(s), 2, _lib.dptr(w), 0.99, _lib.dptr(lp)) == ERR
    assert lib.gpmi_kde_cv_logprob(h.ctx, 10, None, 2, _lib.dptr(w), 0.99, _lib.dptr(lp)) == ERR
    assert lib.gpmi_kde_cv_logprob(h.ctx, 10, _lib.dptr(s), 0, _lib.dptr(w), 0.99, _lib.dptr(lp)) == ERR
    assert lib.gpmi_kde_cv_logprob(h.ctx, 10, _lib.dptr(s), 2, _lib.dptr(w), 1.5, _lib.dptr(lp)) == ERR
    assert lib.gpmi_kde_cv_logprob(h.ctx, 10, _lib.dptr(s), 2, _lib.dptr(w), 0.99, None) == ERR
    assert lib.gpmi_kde_cv_logprob(h.ctx, 10, _lib.dptr(s), 2, _lib.dptr(w), 0.99, _lib.dptr(lp)) == 0


def test_handle_owns_densities():
    """A closed handle has released its densities: their finalisers must not call into freed memory, and the module
    opens a new handle for the next density."""
    import gc

    from inference_amd import _lib
    from inference_amd.pdf import GaussianKDE, _device

    kdes = [GaussianKDE(np.random.default_rng(k).normal(size=500)) for k in range(3)]
    old = _device.handle()
    assert all(k._density.h is old for k in kdes)
    old.close()
    with pytest.raises(_lib.GpmiUnavailable):
        kdes[0](0.0)
    del kdes
    gc.collect()
    kde = GaussianKDE(np.random.default_rng(9).normal(size=500))
    assert kde._density.h is not old and kde._density.h.ctx
    assert np.isfinite(kde(0.0))


def test_threads_share_the_handle_safely():
    """KDEs built and evaluated on several threads at once (on the one module handle) give the bits of a
    single-threaded run."""
    from concurrent.futures import ThreadPoolExecutor

    from inference_amd.pdf import GaussianKDE, _device

    rng = np.random.default_rng(77)
    samples = [np.concatenate([rng.normal(k, 1.0, 2000 + 400 * k), rng.normal(-k, 0.3, 1000)]) for k in range(6)]
    assert max(s.size for s in samples) <= 5000  # the cross-validation uses every sample: no draw from the generator
    x = np.linspace(-8, 8, 3000)

    def work(k):
        kde = GaussianKDE(samples[k], cross_validation=(k % 2 == 0))  # n <= 5000: no random subsample
        out = (kde.h, kde.mode, kde(x), kde.cdf(x), kde.interval(0.9), _device.cv_logprob(samples[k], [0.1, 0.3]))
        del kde  # releases its density object while the other threads run
        return out

    serial = [work(k) for k in range(len(samples))]
    for _ in range(2):
        with ThreadPoolExecutor(max_workers=6) as pool:
            threaded = list(pool.map(work, range(len(samples))))
        for a, b in zip(serial, threaded):
            assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
            for u, v in zip(a[2:4] + a[5:], b[2:4] + b[5:]):
                assert np.array_equal(u, v)
    assert len({id(h) for h in _device._handles.values()}) == len(_device._handles)


def test_default_device_shares_the_handle():
    from inference_amd.pdf import GaussianKDE, _device

    s = np.random.default_rng(8).normal(size=1000)
    a = GaussianKDE(s)
    b = GaussianKDE(s, device=_device.resolve_device(None))
    assert a._density.h is b._density.h
    assert np.array_equal(a(np.linspace(-3, 3, 50)), b(np.linspace(-3, 3, 50)))


def test_get_marginal_from_parallel_tempering():
    from inference_amd.mcmc import GibbsChain, ParallelTempering
    from inference_amd.pdf import GaussianKDE

    def posterior(t):
        return float(-0.5 * ((t[0] - 1.0) ** 2 / 0.25 + (t[1] + 2.0) ** 2))

    chains = []
    for k, temp in enumerate((1.0, 2.0, 4.0)):
        ch = GibbsChain(posterior=posterior, start=np.array([0.5, -1.5]), widths=[0.2, 0.3], temperature=temp)
        ch.rng = np.random.default_rng(10 + k)
        for i, p in enumerate(ch.params):
            p.rng = np.random.default_rng(100 * k + i)
        chains.append(ch)
    pt = ParallelTempering(chains)
    pt.rng = np.random.default_rng(1)
    pt.advance(300, swap_interval=10)
    for c in pt.return_chains():
        for i in range(2):
            m = c.get_marginal(i, burn=20, thin=2)
            ref = GaussianKDE(c.get_parameter(i, burn=20, thin=2))
            assert m.h == ref.h and m.mode == ref.mode
            x = np.linspace(ref.lwr_limit, ref.upr_limit, 200)
            assert np.array_equal(m(x), ref(x)) and np.array_equal(m.cdf(x), ref.cdf(x))
        assert np.array_equal(c.mode(), c.get_sample(burn=0)[int(np.argmax(c.probs))])


def test_kde_bench_tool_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kde_bench.py"), "--tiny"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pairs/s" in r.stdout
