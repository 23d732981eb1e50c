"""
GPU tests of the 2-D density estimator (inference_amd.pdf.KDE2D over csrc/kde2d.hip), of matrix_plot_data and of
GibbsChain.matrix_plot: against the reference's values (tests/golden/kde2d.npz, written by golden/make_golden_kde2d.py),
against NumPy sums computed here (tests/kde2d_host.py), and run against run.  Every test prints the worst error it
reached per quantity.

Densities from all three entry points are held to rtol 1e-12 (the figure test_kde_gpu.py holds the 1-D pdf to) plus an
absolute term of n x 2.3e-308 x norm: a term flushed to zero, or a factor pair that underflows, loses at most the
smallest normal double, n times over.
"""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import kde2d_host as kh

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WORST = {}
DENSITY_CASES = ["corr", "banana", "tiny", "ties", "shift"]


def note(what, err):
    WORST[what] = max(WORST.get(what, 0.0), float(err))
    print(f"[kde2d] worst {what}: {WORST[what]:.3e}")


@pytest.mark.parametrize("prefix", DENSITY_CASES)
def test_against_reference(golden, prefix):
    from inference_amd.pdf import KDE2D

    g = golden("kde2d")
    pdf = KDE2D(g[f"{prefix}_x"], g[f"{prefix}_y"])
    assert pdf.q_x == g[f"{prefix}_q_x"] and pdf.q_y == g[f"{prefix}_q_y"] and pdf.norm == g[f"{prefix}_norm"]  # bit-equal
    n, norm = pdf.x.size, pdf.norm
    px, py, gx, gy = (g[f"{prefix}_{k}"] for k in ("px", "py", "gx", "gy"))
    got = pdf(px, py)
    assert isinstance(got, list) and len(got) == px.size
    kh.density_close(got, g[f"{prefix}_pdf"], n, norm, "scattered vs reference", note)
    kh.density_close(pdf.at_samples(), g[f"{prefix}_self"], n, norm, "at_samples vs reference", note)
    grid = pdf.grid(gx, gy)
    kh.density_close(grid, g[f"{prefix}_grid"], n, norm, "grid vs reference", note)
    # grid() against __call__ on the meshgrid, whichever kernel it was routed to
    X, Y = np.meshgrid(gx, gy)
    kh.density_close(grid, np.array(pdf(X.flatten(), Y.flatten())).reshape(grid.shape), n, norm, "grid vs __call__", note)
    # the factorised kernel and the direct sum called directly, whatever the routing prefers
    fact = pdf._density.grid_sums(gx, gy, pdf.q_x, pdf.q_y) * norm
    kh.density_close(fact, g[f"{prefix}_grid"], n, norm, "factorised grid vs reference", note)
    direct = pdf._density.sums(X.ravel(), Y.ravel(), pdf.q_x, pdf.q_y).reshape(grid.shape) * norm
    kh.density_close(direct, g[f"{prefix}_grid"], n, norm, "direct grid vs reference", note)
    if prefix == "corr":
        assert (g["corr_pdf"] == 0.0).any() and (np.array(got)[g["corr_pdf"] == 0.0] <= n * 2.3e-308 * norm).all()


def test_call_forms(golden):
    from inference_amd.pdf import KDE2D

    g = golden("kde2d")
    pdf = KDE2D(g["corr_x"], g["corr_y"])
    px, py = g["corr_px"], g["corr_py"]
    one = pdf(float(px[3]), float(py[3]))
    assert np.ndim(one) == 0
    kh.density_close(one, g["calls_scalar"], 3000, pdf.norm, "scalar call", note)
    many = pdf(list(px[:7]), list(py[:7]))
    assert isinstance(many, list) and len(many) == 7
    kh.density_close(many, g["calls_list"], 3000, pdf.norm, "list call", note)
    short = pdf(px[:9], py[:5])
    assert isinstance(short, list) and len(short) == 5
    kh.density_close(short, g["calls_unequal"], 3000, pdf.norm, "zip truncation", note)
    assert pdf([], []) == [] and pdf.density(float(px[3]), float(py[3])) == one == many[3]


def test_degenerate_is_nan(golden):
    from inference_amd.pdf import KDE2D

    xd = golden("kde2d")["degenerate_x"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pdf = KDE2D(xd, 2 * xd)
    assert pdf._density is None
    assert np.isnan(pdf(xd[:20] + 0.1, 2 * xd[:20])).all() and np.isnan(pdf(0.1, 0.3))
    assert np.isnan(pdf.grid(xd[:4], xd[:3])).all() and np.isnan(pdf.at_samples()).all()


@pytest.mark.parametrize("style", ["contour", "hdi"])
def test_matrix_plot_data_against_reference(golden, style):
    from inference_amd.plotting import matrix_plot_data

    g = golden("kde2d")
    data = matrix_plot_data(list(g["mp_samples"]), plot_style=style, hdi_fractions=tuple(g["mp_hdi_fractions"]))
    kh.check_matrix_plot_data(data, g, style, note)


def two_clusters(n, seed):
    """Two well separated, differently correlated clusters: most tile pairs of the self sum are out of reach."""
    rng = np.random.default_rng(seed)
    k = n // 2
    z = rng.normal(size=(4, n))
    x = np.concatenate([z[0, :k], 12.0 + 0.5 * z[0, k:]])
    y = np.concatenate([0.6 * z[0, :k] + 0.8 * z[1, :k], -9.0 + z[1, k:]])
    p = rng.permutation(n)
    return x[p], y[p]


def test_run_against_run_and_batch_independence(golden):
    from inference_amd.pdf import KDE2D

    g = golden("kde2d")
    pdf = KDE2D(g["banana_x"], g["banana_y"])
    px, py = g["banana_px"][:1000], g["banana_py"][:1000]
    a = np.array(pdf(px, py))
    assert np.array_equal(a, np.array(pdf(px, py)))
    for k in (0, 1, 255, 256, 617, 999):  # one point alone has the bits it has inside the batch of 1000
        assert pdf(float(px[k]), float(py[k])) == a[k], k
        assert pdf(px[k:k + 1], py[k:k + 1])[0] == a[k]
    assert np.array_equal(a[300:700], np.array(pdf(px[300:700], py[300:700])))
    s1 = pdf.at_samples()
    assert np.array_equal(s1, pdf.at_samples())
    gx, gy = g["banana_gx"], g["banana_gy"]
    d = pdf._density
    f1 = d.grid_sums(gx, gy, pdf.q_x, pdf.q_y)
    assert np.array_equal(f1, d.grid_sums(gx, gy, pdf.q_x, pdf.q_y))
    assert np.array_equal(pdf.grid(gx, gy), pdf.grid(gx, gy))
    # a second object of the same sample, and a larger sample where the ranges are many
    x, y = two_clusters(60_000, 5)
    big, big2 = KDE2D(x, y), KDE2D(x, y)
    qx, qy = x[:777] + 0.01, y[:777] - 0.02
    b = np.array(big(qx, qy))
    assert np.array_equal(b, np.array(big2(qx, qy))) and big(float(qx[500]), float(qy[500])) == b[500]
    assert np.array_equal(big.at_samples(), big2.at_samples())
    assert np.array_equal(big.grid(gx, gy), big2.grid(gx, gy))
    assert np.array_equal(big._density.grid_sums(gx, gy, big.q_x, big.q_y), big2._density.grid_sums(gx, gy, big.q_x, big.q_y))


def test_scattered_large_against_numpy():
    from inference_amd.pdf import KDE2D

    rng = np.random.default_rng(11)
    n = 200_000
    t = rng.normal(size=n)
    x, y = t + 0.2 * rng.normal(size=n), np.sin(2 * t) + 0.3 * rng.normal(size=n)
    pdf = KDE2D(x, y)
    own = rng.integers(0, n, 200)
    a = np.concatenate([rng.normal(0, 1.5, 1500), rng.uniform(-12, 12, 300), x[own]])
    b = np.concatenate([rng.normal(0, 1.0, 1500), rng.uniform(-8, 8, 300), y[own]])
    ref = kh.raw_sums(x, y, pdf.q_x, pdf.q_y, a, b) * pdf.norm
    kh.density_close(pdf(a, b), ref, n, pdf.norm, "scattered n=2e5 vs NumPy", note)


@pytest.mark.parametrize("g", [64, 200])
def test_grid_large_against_numpy(g):
    from inference_amd.pdf import KDE2D

    rng = np.random.default_rng(12 + g)
    n = 200_000
    t = rng.normal(size=n)
    x, y = t + 0.2 * rng.normal(size=n), np.sin(2 * t) + 0.3 * rng.normal(size=n)
    pdf = KDE2D(x, y)
    gx, gy = np.linspace(-5.0, 5.0, g), np.linspace(-3.0, 3.5, g - 3)  # not square, not a multiple of the block
    grid = pdf.grid(gx, gy)
    fact = pdf._density.grid_sums(gx, gy, pdf.q_x, pdf.q_y) * pdf.norm
    assert grid.shape == fact.shape == (g - 3, g)
    cells = rng.choice(grid.size, 500, replace=False)
    cells[:4] = [0, g - 1, grid.size - g, grid.size - 1]  # the corners
    iy, ix = np.unravel_index(cells, grid.shape)
    ref = kh.raw_sums(x, y, pdf.q_x, pdf.q_y, gx[ix], gy[iy]) * pdf.norm
    kh.density_close(grid[iy, ix], ref, n, pdf.norm, f"grid {g} n=2e5 vs NumPy", note)
    kh.density_close(fact[iy, ix], ref, n, pdf.norm, f"factorised grid {g} n=2e5 vs NumPy", note)
    direct = np.array(pdf(gx[ix], gy[iy]))
    kh.density_close(direct, ref, n, pdf.norm, f"direct grid {g} n=2e5 vs NumPy", note)


def test_at_samples_skip_rule_against_numpy():
    """The test of the skip rule: two clusters, most tile pairs skipped, every value still that of the full sum."""
    from inference_amd.pdf import KDE2D

    n = 100_000
    x, y = two_clusters(n, 21)
    pdf = KDE2D(x, y)
    got = pdf.at_samples()
    sums, (done, total) = pdf._density.self_sums(pdf.q_x, pdf.q_y, count_tiles=True)
    print(f"[kde2d] at_samples n = {n}: {done} of {total} tile pairs computed ({done / total:.3f})")
    assert total == ((n + 255) // 256) ** 2 and 0 < done < 0.5 * total
    assert np.array_equal(sums * pdf.norm, got)
    idx = np.random.default_rng(22).choice(n, 500, replace=False)
    ref = kh.raw_sums(x, y, pdf.q_x, pdf.q_y, x[idx], y[idx]) * pdf.norm
    kh.density_close(got[idx], ref, n, pdf.norm, "at_samples n=1e5 vs NumPy", note)
    kh.density_close(np.array(pdf(x[idx], y[idx])), ref, n, pdf.norm, "scattered at samples n=1e5 vs NumPy", note)
    assert (sums >= 1.0).all()


def test_abi_error_returns():
    from inference_amd import _lib
    from inference_amd.pdf import _device

    h = _device.handle()
    lib = h.lib
    ERR = -1
    rng = np.random.default_rng(3)
    x, y = rng.normal(size=10), rng.normal(size=10)
    dp = _lib.dptr
    out = C.c_void_p()

    def text():
        return lib.gpmi_last_error(h.ctx).decode()

    assert lib.gpmi_kde2d_create(None, 10, dp(x), dp(y), C.byref(out)) == ERR
    for args in ((10, None, dp(y)), (10, dp(x), None), (0, dp(x), dp(y)), (-3, dp(x), dp(y)), (2**31, dp(x), dp(y))):
        assert lib.gpmi_kde2d_create(h.ctx, *args, C.byref(out)) == ERR and "gpmi_kde2d_create" in text()
    assert lib.gpmi_kde2d_create(h.ctx, 10, dp(x), dp(y), None) == ERR
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[4] = bad
        assert lib.gpmi_kde2d_create(h.ctx, 10, dp(xb), dp(y), C.byref(out)) == ERR and "finite" in text()
        assert lib.gpmi_kde2d_create(h.ctx, 10, dp(x), dp(xb), C.byref(out)) == ERR
    assert lib.gpmi_kde2d_create(h.ctx, 10, dp(x), dp(y), C.byref(out)) == 0

    a, b, s = np.array([0.1, 0.2]), np.array([0.0, -0.3]), np.empty(2)
    big = np.empty(10)
    tiles = np.zeros(2, dtype=np.int64)
    i64 = tiles.ctypes.data_as(C.POINTER(C.c_int64))
    ax, ay, gs = np.linspace(-1, 1, 3), np.linspace(-1, 1, 2), np.empty(6)
    for qx, qy in ((0.0, 1.0), (1.0, 0.0), (np.inf, 1.0), (1.0, np.inf), (-1.0, 1.0), (np.nan, 1.0)):
        assert lib.gpmi_kde2d_eval(h.ctx, out, 2, dp(a), dp(b), qx, qy, dp(s)) == ERR and "q_x" in text()
        assert lib.gpmi_kde2d_self(h.ctx, out, qx, qy, dp(big), i64) == ERR
        assert lib.gpmi_kde2d_grid(h.ctx, out, 3, dp(ax), 2, dp(ay), qx, qy, dp(gs)) == ERR
    assert lib.gpmi_kde2d_eval(h.ctx, out, 2, None, dp(b), 1.0, 1.0, dp(s)) == ERR
    assert lib.gpmi_kde2d_eval(h.ctx, out, 2, dp(a), None, 1.0, 1.0, dp(s)) == ERR
    assert lib.gpmi_kde2d_eval(h.ctx, out, 2, dp(a), dp(b), 1.0, 1.0, None) == ERR
    assert lib.gpmi_kde2d_eval(h.ctx, out, -1, dp(a), dp(b), 1.0, 1.0, dp(s)) == ERR
    assert lib.gpmi_kde2d_eval(h.ctx, None, 2, dp(a), dp(b), 1.0, 1.0, dp(s)) == ERR
    assert lib.gpmi_kde2d_eval(None, out, 2, dp(a), dp(b), 1.0, 1.0, dp(s)) == ERR
    assert lib.gpmi_kde2d_eval(h.ctx, out, 0, None, None, 1.0, 1.0, None) == 0  # m = 0 returns at once
    assert lib.gpmi_kde2d_self(h.ctx, out, 1.0, 1.0, None, None) == ERR
    assert lib.gpmi_kde2d_self(h.ctx, None, 1.0, 1.0, dp(big), None) == ERR
    assert lib.gpmi_kde2d_grid(h.ctx, out, 3, None, 2, dp(ay), 1.0, 1.0, dp(gs)) == ERR
    assert lib.gpmi_kde2d_grid(h.ctx, out, 3, dp(ax), 2, dp(ay), 1.0, 1.0, None) == ERR
    assert lib.gpmi_kde2d_grid(h.ctx, out, -1, dp(ax), 2, dp(ay), 1.0, 1.0, dp(gs)) == ERR
    assert lib.gpmi_kde2d_grid(h.ctx, out, 0, None, 2, dp(ay), 1.0, 1.0, None) == 0
    # the good calls, against NumPy
    assert lib.gpmi_kde2d_eval(h.ctx, out, 2, dp(a), dp(b), 0.7, 1.3, dp(s)) == 0
    kh.density_close(s, kh.raw_sums(x, y, 0.7, 1.3, a, b), 10, 1.0, "eval ABI", note)
    assert lib.gpmi_kde2d_self(h.ctx, out, 0.7, 1.3, dp(big), i64) == 0 and list(tiles) == [1, 1]
    kh.density_close(big, kh.raw_sums(x, y, 0.7, 1.3, x, y), 10, 1.0, "self ABI", note)
    assert lib.gpmi_kde2d_grid(h.ctx, out, 3, dp(ax), 2, dp(ay), 0.7, 1.3, dp(gs)) == 0
    X, Y = np.meshgrid(ax, ay)
    kh.density_close(gs, kh.raw_sums(x, y, 0.7, 1.3, X.ravel(), Y.ravel()), 10, 1.0, "grid ABI", note)
    # an object used after its release
    assert lib.gpmi_kde2d_destroy(h.ctx, out) == 0
    assert lib.gpmi_kde2d_eval(h.ctx, out, 2, dp(a), dp(b), 1.0, 1.0, dp(s)) == ERR and "not a live" in text()
    assert lib.gpmi_kde2d_self(h.ctx, out, 1.0, 1.0, dp(big), None) == ERR
    assert lib.gpmi_kde2d_grid(h.ctx, out, 3, dp(ax), 2, dp(ay), 1.0, 1.0, dp(gs)) == ERR
    assert lib.gpmi_kde2d_destroy(h.ctx, out) == ERR and lib.gpmi_kde2d_destroy(h.ctx, None) == ERR
    assert lib.gpmi_kde2d_destroy(None, out) == ERR


def test_handle_owns_densities():
    """Closing a handle releases its live 2-D objects (100 of them), their finalisers then leave the freed memory alone,
    and the module opens a new handle for the next density."""
    import gc

    from inference_amd import _lib
    from inference_amd.pdf import KDE2D, _device

    rng = np.random.default_rng(1)
    pdfs = [KDE2D(rng.normal(size=300), rng.normal(size=300)) for _ in range(100)]
    old = _device.handle()
    assert all(p._density.h is old for p in pdfs)
    old.close()
    with pytest.raises(_lib.GpmiUnavailable):
        pdfs[0](0.0, 0.0)
    del pdfs
    gc.collect()
    pdf = KDE2D(rng.normal(size=300), rng.normal(size=300))
    assert pdf._density.h is not old and np.isfinite(pdf(0.0, 0.0))


def injected_chain(n_par=3, length=600):
    from inference_amd.mcmc import GibbsChain

    chain = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(n_par),
                       display_progress=False)
    S = np.random.default_rng(4).normal(size=(length, n_par)) * np.array([1.0, 2.0, 0.5])[:n_par]
    S[:, 1] += 0.8 * S[:, 0]
    for i, p in enumerate(chain.params):
        p.samples = list(S[:, i])
    chain.probs = list(-0.5 * np.sum(S**2, axis=1))
    chain.chain_length = length
    return chain


@pytest.mark.parametrize("style", ["contour", "hdi", "histogram", "scatter"])
def test_chain_matrix_plot(style):
    pytest.importorskip("matplotlib")
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    chain = injected_chain()
    fig = chain.matrix_plot(burn=50, thin=2, plot_style=style, show=False, labels=["a", "b", "c"], reference=[0.0, 0.0, 0.0])
    assert len(fig.axes) == 6
    plt.close(fig)
    fig = chain.matrix_plot(params=[2, 0], plot_style=style, show=False)
    assert len(fig.axes) == 3
    plt.close(fig)


def test_chain_matrix_plot_checks():
    chain = injected_chain()
    with pytest.raises(ValueError, match="leave insufficient"):
        chain.matrix_plot(burn=599, show=False)
    with pytest.raises(ValueError, match="Number of samples after burn / thin is 1"):
        chain.matrix_plot(thin=600, show=False)
    from inference_amd.mcmc import GibbsChain

    fresh = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(2), display_progress=False)
    with pytest.raises(ValueError, match="no samples have"):
        fresh.matrix_plot(show=False)


def test_kde2d_bench_tool_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kde2d_bench.py"), "--tiny"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pairs/s" in r.stdout and "matrix_6" in r.stdout
