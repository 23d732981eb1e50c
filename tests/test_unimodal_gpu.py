"""
GPU tests of the device sums behind UnimodalPdf (inference_amd.pdf.UnimodalPdf over csrc/unimodal.hip) against the
reference's values (tests/golden/unimodal.npz, written by golden/make_golden_unimodal.py), against a NumPy evaluation of
the same formula at n = 10^6, run against run, one theta against a batch, across threads, and end to end against the
reference's fit within the reference's own response to rounding-level noise.  Every test prints the worst error it
reached per quantity.
"""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ["gauss", "gamma", "t3", "logn", "big", "tiny"]
# The one case excused from the MAP comparison of the end-to-end test: at n = 10^5 the likelihood is nearly flat in k (the
# reference's own MAP moves by 1e-2 in k under noise of 1e-12), so MAP is not a stable read-out there.  Its pdf and its
# posterior are compared like every other case's.
MAP_EXCUSED = "big"
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


def numpy_sum(s, theta):
    from inference_amd.pdf.unimodal import log_pdf_model

    with np.errstate(all="ignore"):
        return log_pdf_model(s, theta).sum()


@pytest.mark.parametrize("prefix", CASES)
def test_sums_at_every_recorded_theta(golden, prefix):
    """The arithmetic: the device sums at every theta the reference's fit asked for, with its stride, against the
    reference's own sums, and the posterior (sum - n_fit log norm) against the value the reference returned."""
    from inference_amd.pdf import UnimodalPdf, _device

    g = golden("unimodal")
    s = sample_of(g, prefix)
    theta, stride = g[f"{prefix}_rec_theta"], g[f"{prefix}_rec_stride"]
    dev = _device.DeviceUnimodal(s)
    got = np.empty(theta.shape[0])
    for st in np.unique(stride):
        sel = stride == st
        got[sel] = dev.sums(theta[sel], stride=int(st))
    close(got, g[f"{prefix}_rec_sum"], 1e-12, 0.0, f"sums ({prefix})")
    # the class's posterior: the two terms may cancel, so its error is held relative to the larger of them
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pdf = UnimodalPdf.from_fit(s, g[f"{prefix}_MAP"])
    full = stride == 1
    post = np.array(pdf.posterior_batch(theta[full]))
    n_log_norm = s.size * np.log(g[f"{prefix}_rec_norm"][full])
    scale = np.maximum(np.abs(g[f"{prefix}_rec_sum"][full]), np.abs(n_log_norm))
    err = (np.abs(post - g[f"{prefix}_rec_post"][full]) / scale).max()
    note("posterior / larger term", err)
    assert err <= 1e-12
    assert pdf.posterior(theta[-1]) == post[-1]


def test_bits_single_batch_and_repeat(golden):
    from inference_amd.pdf import _device

    g = golden("unimodal")
    for prefix, stride in (("gamma", 1), ("logn", 2), ("big", 50), ("big", 1), ("tiny", 1)):
        dev = _device.DeviceUnimodal(sample_of(g, prefix))
        batch = g[f"{prefix}_rec_theta"][:72]
        a = dev.sums(batch, stride=stride)
        assert np.array_equal(a, dev.sums(batch, stride=stride))  # run against run
        for k in (0, 17, 35, 71):  # one theta alone against the same theta in a batch
            assert dev.sums(batch[k:k + 1], stride=stride)[0] == a[k]
        many = np.concatenate([batch, batch, batch[:7]])  # more than one launch
        b = dev.sums(many, stride=stride)
        assert np.array_equal(b[:72], a) and np.array_equal(b[72:144], a) and np.array_equal(b[144:], a[:7])


def test_threads_share_the_handle_safely(golden):
    """Sums asked for on several threads at once (on the one module handle) give the bits of a single-threaded run."""
    from concurrent.futures import ThreadPoolExecutor

    from inference_amd.pdf import _device

    g = golden("unimodal")
    jobs = [(p, sample_of(g, p), g[f"{p}_rec_theta"][:200], int(g[f"{p}_skip"])) for p in ("gauss", "gamma", "t3", "logn", "big", "tiny")]

    def work(k):
        _, s, theta, skip = jobs[k]
        dev = _device.DeviceUnimodal(s)
        out = [dev.sums(theta[:72], stride=skip)] + [dev.sums(theta[i:i + 1], stride=1) for i in range(72, 200)]
        del dev  # releases its object while the other threads run
        return np.concatenate(out)

    serial = [work(k) for k in range(len(jobs))]
    for _ in range(2):
        with ThreadPoolExecutor(max_workers=6) as pool:
            threaded = list(pool.map(work, range(len(jobs))))
        for a, b in zip(serial, threaded):
            assert np.array_equal(a, b, equal_nan=True)


def test_million_samples_against_numpy():
    from inference_amd.pdf import _device

    rng = np.random.default_rng(424242)
    s = rng.gamma(4.0, 0.5, 1_000_000)
    theta = np.array([
        [1.5, 1.0, 1.0, 0.3, 2.0, 2.0],
        [1.2, 0.7, 0.25, 0.8, 1.0, 2.0],
        [2.0, 2.0, 2.0, -0.5, 8.0, 2.5],
        [1.7, 0.9, 4.0, 1.5, 0.5, 1.0],
        [1.0, 0.4, 0.0, 0.0, 4.0, 6.0],
        [3.0, 1.3, 5.0, -3.0, 20.0, 3.7],
        [0.5, 0.2, 0.5, 3.0, 0.01, 1.3],
        [float(s[500]), 1.0, 1.0, 0.4, 3.0, 2.0],  # a sample sits exactly on x0: z = 0, a zero term
    ])
    dev = _device.DeviceUnimodal(s)
    for stride in (1, 500):
        got = dev.sums(theta, stride=stride)
        ref = np.array([numpy_sum(s[::stride], t) for t in theta])
        assert np.isfinite(ref).all()
        close(got, ref, 1e-12, 0.0, f"sums n=1e6 stride {stride} vs NumPy")
        assert np.array_equal(got, dev.sums(theta, stride=stride))
        assert dev.sums(theta[3:4], stride=stride)[0] == got[3]
    # NaN in theta: NaN out, no error, and the other rows of the batch keep their bits
    bad = theta.copy()
    bad[2, 3] = np.nan
    bad[5, 0] = np.inf  # every z is -inf: the sum is -inf, as NumPy's
    out = dev.sums(bad, stride=1)
    assert np.isnan(out[2]) and out[5] == numpy_sum(s, bad[5]) == -np.inf
    keep = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(out[keep], dev.sums(theta, stride=1)[keep])
    # out-of-range values are not an argument error either: what IEEE arithmetic gives, as NumPy does
    odd = np.array([[1.5, -1.0, 1.0, 0.3, 2.0, 2.0], [1.5, 1.0, 800.0, 0.3, 2.0, 2.0]])
    got = dev.sums(odd, stride=500)
    ref = np.array([numpy_sum(s[::500], t) for t in odd])
    close(got[:1], ref[:1], 1e-12, 0.0, "sums with s0 < 0 vs NumPy")
    assert np.isnan(got[1]) == np.isnan(ref[1]) and (np.isnan(ref[1]) or got[1] == ref[1])


@pytest.mark.parametrize("prefix", CASES)
def test_end_to_end_against_reference_fit(golden, prefix):
    """UnimodalPdf(sample) on the device against the reference's fit.  The fit is path-sensitive (a Nelder-Mead run of
    1100 - 2300 comparisons), so the tolerance is 10 x the reference's own spread under noise of 1e-12 in its
    objective, read from the fixture; where that spread is 0, the project's standing 1e-10."""
    from inference_amd.pdf import UnimodalPdf

    g = golden("unimodal")
    s = sample_of(g, prefix)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pdf = UnimodalPdf(s)
    assert pdf._density is not None and pdf.min_result is not None
    x, ref_pdf, ref_map = g[f"{prefix}_x"], g[f"{prefix}_pdf"], g[f"{prefix}_MAP"]
    sp_pdf, sp_map, sp_post = float(g[f"{prefix}_spread_pdf"]), g[f"{prefix}_spread_MAP"], float(g[f"{prefix}_spread_post"])

    err_pdf = np.abs(pdf(x) - ref_pdf).max() / ref_pdf.max()
    tol_pdf = 10 * sp_pdf if sp_pdf > 0 else 1e-10
    print(f"[unimodal] {prefix}: pdf / max pdf {err_pdf:.3e} (reference's spread {sp_pdf:.3e}, tolerance {tol_pdf:.3e})")

    err_map = np.abs(pdf.MAP - ref_map)
    tol_map = np.where(sp_map > 0, 10 * sp_map, 1e-10 * np.maximum(1.0, np.abs(ref_map)))
    print(f"[unimodal] {prefix}: MAP {np.array2string(err_map, precision=3)} (reference's spread "
          f"{np.array2string(sp_map, precision=3)}){' - excused' if prefix == MAP_EXCUSED else ''}")

    host_post = numpy_sum(s, pdf.MAP) - s.size * np.log(pdf.norm(pdf.MAP))
    err_post = abs(host_post - float(g[f"{prefix}_post_map"]))
    tol_post = 10 * sp_post if sp_post > 0 else 1e-10 * abs(float(g[f"{prefix}_post_map"]))
    print(f"[unimodal] {prefix}: posterior at MAP {err_post:.3e} (reference's spread {sp_post:.3e}, tolerance {tol_post:.3e})")

    assert err_pdf <= tol_pdf
    if prefix != MAP_EXCUSED:
        assert (err_map <= tol_map).all(), (err_map, tol_map)
    assert err_post <= tol_post
    # the read-out of the fitted curve is host arithmetic on MAP
    assert pdf.mode == pdf.MAP[0] and pdf.map_lognorm == np.log(pdf.norm(pdf.MAP))
    assert 0.9 < pdf.cdf(pdf.upr_limit + 10 * (pdf.upr_limit - pdf.lwr_limit)) < 1.0 + 1e-6
    lo, hi = pdf.interval(0.9)
    assert lo < pdf.mode < hi


def test_abi_error_returns(golden):
    from inference_amd import _lib
    from inference_amd.pdf import _device

    h = _device.handle()
    lib = h.lib
    ERR = -1
    s = np.linspace(0.0, 1.0, 10)
    theta = np.array([[0.5, 0.3, 1.0, 0.2, 1.0, 2.0]])
    out = np.empty(1)
    obj = C.c_void_p()
    with h.kde_lock:
        assert lib.gpmi_unimodal_create(h.ctx, 10, None, C.byref(obj)) == ERR
        assert lib.gpmi_unimodal_create(h.ctx, 0, _lib.dptr(s), C.byref(obj)) == ERR
        assert lib.gpmi_unimodal_create(h.ctx, -3, _lib.dptr(s), C.byref(obj)) == ERR
        assert lib.gpmi_unimodal_create(h.ctx, 10, _lib.dptr(s), None) == ERR
        assert lib.gpmi_unimodal_create(None, 10, _lib.dptr(s), C.byref(obj)) == ERR
        assert lib.gpmi_unimodal_create(h.ctx, 10, _lib.dptr(s), C.byref(obj)) == 0
        args = (h.ctx, obj, 1, 1, _lib.dptr(theta), _lib.dptr(out))
        for k, bad in ((0, None), (1, None), (2, 0), (2, -1), (3, 0), (3, -2), (4, None), (5, None)):
            a = list(args)
            a[k] = bad
            assert lib.gpmi_unimodal_logpdf_sums(*a) == ERR, k
        assert "gpmi_unimodal_logpdf_sums" in lib.gpmi_last_error(h.ctx).decode()
        assert lib.gpmi_unimodal_logpdf_sums(*args) == 0
        close(out, [numpy_sum(s, theta[0])], 1e-12, 0.0, "sums ABI")
        assert lib.gpmi_unimodal_logpdf_sums(h.ctx, obj, 100, 1, _lib.dptr(theta), _lib.dptr(out)) == 0  # stride > n: one sample
        close(out, [numpy_sum(s[:1], theta[0])], 1e-12, 0.0, "sums ABI")
        assert lib.gpmi_unimodal_destroy(None, obj) == ERR
        assert lib.gpmi_unimodal_destroy(h.ctx, None) == ERR
        assert lib.gpmi_unimodal_destroy(h.ctx, obj) == 0
        assert lib.gpmi_unimodal_destroy(h.ctx, obj) == ERR  # no longer a live object of the handle
        assert lib.gpmi_unimodal_logpdf_sums(*args) == ERR


def test_handle_owns_unimodal_objects(golden):
    """A closed handle has released its objects: their finalisers must not call into freed memory, and the module
    opens a new handle for the next one."""
    import gc

    from inference_amd import _lib
    from inference_amd.pdf import UnimodalPdf, _device

    g = golden("unimodal")
    theta = g["gauss_MAP"]
    pdfs = [UnimodalPdf.from_fit(np.random.default_rng(k).normal(size=500), theta) for k in range(3)]
    values = [p.posterior(theta) for p in pdfs]
    assert np.isfinite(values).all()
    old = _device.handle()
    assert all(p._density.h is old for p in pdfs)
    old.close()
    with pytest.raises(_lib.GpmiUnavailable):
        pdfs[0].posterior(theta)
    assert np.isfinite(pdfs[0](0.3))  # the fitted curve is host arithmetic
    del pdfs
    gc.collect()
    pdf = UnimodalPdf.from_fit(np.random.default_rng(0).normal(size=500), theta)
    assert pdf.posterior(theta) == values[0]
    assert pdf._density.h is not old and pdf._density.h.ctx


def test_unimodal_bench_tool_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "unimodal_bench.py"), "--tiny"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "sums_1" in r.stdout and "fit" in r.stdout
