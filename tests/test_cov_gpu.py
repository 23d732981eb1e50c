"""GPU tests of the sample covariance on the fp64 matrix cores (csrc/cov.hip, gpmi_cov_columns, `sample_covariance`).

Shapes: n in {2, 3, 5, R - 1, R, R + 1, 2 R + 3} (R = GPMI_COV_CHUNK_ROWS) times m in {1, 2, 15, 16, 17, 63, 64, 65} - the
edges of the MFMA's 16 columns and K = 4 rows, of a 64-column tile and of a row chunk - and m = 512 at n = 37.

Exact: integers in [-1000, 1000] with column sums that are multiples of n (the first row is adjusted) have an exact mean,
exact centred products and exact sums (|S| < 2^53), so the device must give numpy.cov's doubles, bit for bit, in every layout.
Bounded: for real data the device is compared with the covariance computed in numpy.longdouble; the bound
(2 n + 16) 2^-53 sqrt(C_ii C_jj) is a derived worst case (n products and their sums, the centring, the final scaling), not
a measurement; numpy.cov itself stays within 1.1 n 2^-53 sqrt(C_ii C_jj) on such inputs."""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import pca_host as ph

pytestmark = pytest.mark.gpu

M_EDGES = [1, 2, 15, 16, 17, 63, 64, 65]


def chunk_rows():
    from inference_amd.pdf import _device

    return _device.COV_CHUNK_ROWS


def n_edges():
    R = chunk_rows()
    return [2, 3, 5, R - 1, R, R + 1, 2 * R + 3]


def columns(sample, **kwargs):
    from inference_amd.pdf import _device

    return _device.cov_columns(sample, **kwargs)


def layouts(x):
    """The sample in C order, transposed, and both with padded leading dimensions (ld = m + 3 and ld = n + 5)."""
    n, m = x.shape
    wide = np.full((n, m + 3), np.nan)
    wide[:, :m] = x
    tall = np.full((m, n + 5), np.nan)
    tall[:, :n] = x.T
    return {"C": x, "T": np.ascontiguousarray(x.T).T, "C ld = m + 3": wide[:, :m], "T ld = n + 5": tall[:, :n].T}


def check_exact(x):
    n, m = x.shape
    want = np.cov(x.T).reshape(m, m)
    want_mean = x.sum(axis=0) / n
    assert (want_mean == np.round(want_mean)).all()
    for name, a in layouts(x).items():
        mean, cov, flags = columns(a)
        assert not flags.any(), (n, m, name)
        assert_array_equal(mean, want_mean, err_msg=f"mean, n = {n}, m = {m}, {name}")
        assert_array_equal(cov, want, err_msg=f"cov, n = {n}, m = {m}, {name}")


@pytest.mark.parametrize("k", range(7))
def test_exact_integers(k):
    n = n_edges()[k]
    rng = np.random.default_rng(100 + k)
    for m in M_EDGES:
        check_exact(ph.exact_integers(rng, n, m))


def test_exact_integers_at_the_column_limit():
    check_exact(ph.exact_integers(np.random.default_rng(7), 37, 512))


def real_data(rng, n, m):
    return rng.standard_normal((n, m)) * rng.uniform(0.1, 10.0, m) + rng.uniform(-3.0, 3.0, m)


def check_bounded(x):
    n, m = x.shape
    xl = x.astype(np.longdouble)
    yl = xl - xl.sum(axis=0) / n
    exact = (yl.T @ yl) / (n - 1)
    scale = np.sqrt(np.outer(np.diag(exact), np.diag(exact)))
    bound = (2 * n + 16) * 2.0 ** -53 * scale
    mean, cov, flags = columns(x)
    assert not flags.any()
    err = np.abs(cov.astype(np.longdouble) - exact)
    worst = float((err / scale).max() / 2.0 ** -53)
    print(f"n = {n}, m = {m}: worst error {worst:.2f} x 2^-53 sqrt(C_ii C_jj), bound {2 * n + 16}")
    assert (err <= bound).all(), (n, m, worst)
    assert np.abs(mean.astype(np.longdouble) - xl.sum(axis=0) / n).max() <= (n + 2) * 2.0 ** -53 * np.abs(xl).max()


@pytest.mark.parametrize("k", range(7))
def test_bounded_against_long_double(k):
    n = n_edges()[k]
    rng = np.random.default_rng(200 + k)
    for m in M_EDGES:
        check_bounded(real_data(rng, n, m))


def test_bounded_at_the_column_limit():
    check_bounded(real_data(np.random.default_rng(8), 37, 512))


@pytest.fixture(scope="module")
def wide():
    """2 R + 3 rows of 65 columns, and its covariance: computed once, never changed."""
    x = real_data(np.random.default_rng(9), 2 * chunk_rows() + 3, 65)
    x.setflags(write=False)
    mean, cov, flags = columns(x)
    assert not flags.any()
    cov.setflags(write=False)
    return x, mean, cov


def test_symmetry_and_repetition(wide):
    x, mean, cov = wide
    assert_array_equal(cov, cov.T)
    again = columns(x)
    assert_array_equal(again[0], mean)
    assert_array_equal(again[1], cov)


@pytest.mark.parametrize("k", [1, 17, 64])
def test_leading_columns_alone(wide, k):
    x, mean, cov = wide
    alone = columns(np.ascontiguousarray(x[:, :k]))
    assert_array_equal(alone[1], cov[:k, :k])
    assert_array_equal(alone[0], mean[:k])


def test_two_columns_alone_and_a_permutation(wide):
    x, mean, cov = wide
    pair = columns(np.ascontiguousarray(x[:, [40, 3]]))[1]
    assert_array_equal(pair, cov[np.ix_([40, 3], [40, 3])])
    perm = np.random.default_rng(10).permutation(65)
    moved = columns(np.ascontiguousarray(x[:, perm]))
    assert_array_equal(moved[1], cov[np.ix_(perm, perm)])
    assert_array_equal(moved[0], mean[perm])


def test_layouts_and_workspace_caps(wide):
    x, mean, cov = wide
    for name, a in layouts(np.array(x)).items():
        got = columns(a)
        assert_array_equal(got[1], cov, err_msg=name)
        assert_array_equal(got[0], mean, err_msg=name)
    # 65 columns are two tiles, three tile pairs: 3 x 32768 bytes per chunk of rows; three chunks
    per_chunk = 3 * 32768
    for cap in (per_chunk, 2 * per_chunk + 100, 3 * per_chunk):  # three groups, two (2 + 1), one
        assert_array_equal(columns(x, ws_bytes=cap)[1], cov, err_msg=f"ws_bytes = {cap}")
        assert_array_equal(columns(np.ascontiguousarray(x.T).T, ws_bytes=cap)[1], cov, err_msg=f"transposed, ws_bytes = {cap}")


def test_impossible_cap(wide):
    from inference_amd import _lib

    with pytest.raises(_lib.GpmiError, match="one chunk"):
        columns(wide[0], ws_bytes=3 * 32768 - 8)
    assert_array_equal(columns(wide[0])[1], wide[2])


def test_views_are_read_in_place(monkeypatch):
    from inference_amd.pdf import _device

    a = real_data(np.random.default_rng(11), 258, 129)
    ref = columns(a)[1]
    seen = []
    inner = _device._call

    def spy(h, name, ctx, n, m, row_stride, col_stride, pointer, *rest):
        seen.append((name, n, m, row_stride, col_stride, C.cast(pointer, C.c_void_p).value))
        return inner(h, name, ctx, n, m, row_stride, col_stride, pointer, *rest)

    monkeypatch.setattr(_device, "_call", spy)
    v = a[:, 3:40]
    assert_array_equal(columns(v)[1], ref[3:40, 3:40])
    assert seen[-1] == ("gpmi_cov_columns", 258, 37, 129, 1, v.ctypes.data)
    b = np.ascontiguousarray(a.T)
    assert_array_equal(columns(b.T)[1], ref)
    assert seen[-1] == ("gpmi_cov_columns", 258, 129, 1, 258, b.ctypes.data)
    assert_array_equal(columns(b[5:70].T)[1], ref[5:70, 5:70])
    w = a[:, ::2]  # dense in neither order: through a C-contiguous copy
    assert_array_equal(columns(w)[1], ref[::2, ::2])
    assert seen[-1][1:5] == (258, 65, 65, 1) and seen[-1][5] != w.ctypes.data
    one = columns(a[:, 7:8])  # one column of a C array, read in place
    assert seen[-1] == ("gpmi_cov_columns", 258, 1, 129, 1, a[:, 7:8].ctypes.data)
    assert_array_equal(one[1], ref[7:8, 7:8])


def test_sample_covariance_surface():
    from inference_amd.mcmc import sample_covariance

    x = real_data(np.random.default_rng(12), 300, 6)
    cov = sample_covariance(x)
    assert cov.shape == (6, 6) and cov.dtype == np.float64
    assert_array_equal(cov, columns(x)[1])
    both = sample_covariance(x, return_mean=True)
    assert_array_equal(both[0], cov)
    assert_array_equal(both[1], columns(x)[0])
    np.testing.assert_allclose(cov, np.cov(x.T), rtol=1e-12, atol=0)
    line = sample_covariance(x[:, 2])  # a 1-D sample is one column
    assert line.shape == (1, 1)
    assert_array_equal(line, cov[2:3, 2:3])
    f32 = x.astype(np.float32)
    assert_array_equal(sample_covariance(f32), sample_covariance(f32.astype(np.float64)))


def test_flags_and_errors():
    from inference_amd import _lib
    from inference_amd.mcmc import sample_covariance
    from inference_amd.pdf import _device

    R = chunk_rows()
    x = real_data(np.random.default_rng(13), R + 40, 70)
    clean = columns(x)[1]
    bad = x.copy()
    bad[R + 7, 5] = np.nan    # in the second chunk
    bad[3, 66] = -np.inf      # in the second tile
    for a in (bad, np.ascontiguousarray(bad.T).T):
        mean, cov, flags = columns(a)
        assert np.flatnonzero(flags).tolist() == [5, 66] and set(flags.tolist()) == {0, 1}
        keep = np.setdiff1d(np.arange(70), [5, 66])
        assert_array_equal(cov[np.ix_(keep, keep)], clean[np.ix_(keep, keep)])  # the other columns are not affected
    with np.errstate(invalid="ignore"):
        want = np.cov(bad.T)
        got, got_mean = sample_covariance(bad, return_mean=True)
        assert_array_equal(got, want)  # NumPy's array, NaNs in the same places
        assert_array_equal(np.isnan(got), np.isnan(want))
        assert_array_equal(got_mean, bad.mean(axis=0))
    assert np.isnan(got[5]).all() and np.isnan(got[:, 66]).all() and np.isfinite(got[np.ix_(keep, keep)]).all()

    # n = 1, m = 0, m = 513 and bad strides are GPMI_ERR_ARG with a text
    h = _device.handle()
    z = np.zeros((8, 4))
    out = [np.zeros(4), np.zeros((4, 4)), np.zeros(4, dtype=np.int32)]
    ptrs = (_lib.dptr(out[0]), _lib.dptr(out[1]), out[2].ctypes.data_as(C.POINTER(C.c_int32)))
    for n, m, rs, cs, text in ((8, 4, 3, 1, "strides"), (8, 4, 1, 7, "strides"), (8, 4, 2, 2, "strides"),
                               (1, 4, 4, 1, "n out of range"), (8, 0, 4, 1, "m out of range"),
                               (8, 513, 513, 1, "m out of range")):
        with pytest.raises(_lib.GpmiError, match=f"status -1.*{text}"):
            _device._call(h, "gpmi_cov_columns", h.ctx, n, m, rs, cs, _lib.dptr(z), 0, *ptrs)
    with pytest.raises(_lib.GpmiError, match="status -1.*ws_bytes"):
        _device._call(h, "gpmi_cov_columns", h.ctx, 8, 4, 4, 1, _lib.dptr(z), -1, *ptrs)
    # and the handle is fine afterwards
    assert_array_equal(columns(x)[1], clean)


def test_cov_bench_tool_runs():
    import os
    import subprocess
    import sys

    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "cov_bench.py"), "--tiny", "--reps", "1"], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "device" in r.stdout and "numpy" in r.stdout
