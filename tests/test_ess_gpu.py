"""GPU tests of the batched effective sample sizes (csrc/acf.hip, gpmi_acf_columns, `effective_sample_size_batch`) and of
the chain diagnostics built on them, against the reference's own outputs in golden/ess.npz (golden/make_golden_ess.py).

`cut` and the integer are compared with `assert_array_equal`; `f0` and `sum` to 1e-10 relative (the project's parity class:
the device sums the lags directly, the reference takes them from an FFT - the two routes measured 4e-16 of f0 apart in
NumPy).  The generator asserted of every even-n column that no lag up to the cut is closer to zero than 1e-7 f0 and that
n / tau is no closer than 1e-7 (relative) to an integer, 500 times that tolerance, so neither integer can flip inside it.
For odd n the reference's numbers are not an autocorrelation of the sample; there the device is compared with the stored
numbers of the NumPy lag-sum mirror (tests/ess_host.py), under the same rule."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import ess_host as eh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("ess")


def batch(sample, **kwargs):
    from inference_amd.mcmc import effective_sample_size_batch

    return effective_sample_size_batch(sample, details=True, **kwargs)


def columns(sample, **kwargs):
    from inference_amd.pdf import _device

    return _device.acf_columns(sample, **kwargs)


def same_bits(a, b):
    for x, y in zip(a, b):
        assert_array_equal(x, y)


def against(got, g, name, prefix=""):
    ess, f0, total, cut = got
    assert ess.dtype == np.int64 and cut.dtype == np.int64
    assert_array_equal(cut, g[f"{name}_{prefix}cut"])
    assert_array_equal(ess, g[f"{name}_{prefix}ess"])
    assert_allclose(f0, g[f"{name}_{prefix}f0"], rtol=eh.TOL, atol=0)
    assert_allclose(total, g[f"{name}_{prefix}sum"], rtol=eh.TOL, atol=0)


@pytest.mark.parametrize("name", eh.EVEN + ["tiny_4"])
def test_even_n_against_the_reference(g, name):
    against(batch(eh.checked_case(g, name)), g, name)


@pytest.mark.parametrize("name", eh.ODD)
def test_odd_n_against_the_lag_sum_mirror(g, name):
    s = eh.checked_case(g, name)
    assert s.shape[0] % 2 == 1
    against(batch(s), g, name, prefix="mirror_")


def test_one_dimensional_sample(g):
    from inference_amd.mcmc import effective_sample_size_batch

    s = eh.checked_case(g, "ramp_4096")
    got = effective_sample_size_batch(s[:, 0])
    assert got.shape == (1,) and got.dtype == np.int64
    assert_array_equal(got, g["ramp_4096_ess"])


def test_lag_block_boundaries():
    """Cosine columns whose first negative lag is the last lag of a block, the first of the next and the one after, for the
    first three block boundaries, against the product's own host function (which the CPU tests pin to the reference)."""
    from inference_amd.mcmc import effective_sample_size
    from inference_amd.pdf import _device

    seen = []
    for b in (256, 512, 1024):
        starts = _device.acf_lag_blocks(4 * b)
        assert b in starts, (b, starts)
        seen.append(starts.index(b))
        for c in (b - 1, b, b + 1):
            s = eh.cosine(c)
            ess, f0, total, cut = batch(s)
            assert cut[0] == c
            assert ess[0] == effective_sample_size(s[:, 0])
    assert seen == [1, 2, 3]  # the first three boundaries of the schedule


def test_independence_and_determinism(g):
    s = eh.checked_case(g, "ar_4096")
    whole = columns(s)
    assert not whole[3].any()
    alone = columns(s[:, 17].copy().reshape(-1, 1))
    few = columns(np.ascontiguousarray(s[:, 16:19]))
    for k in range(3):
        assert_array_equal(alone[k][0], whole[k][17])
        assert_array_equal(few[k][1], whole[k][17])
    same_bits(columns(s), whole)
    # a workspace cap that forces three column blocks (100 + 100 + 56), by the cost per column that include/gpmi.h states
    per_col = 8 * 4096 + 8 * (4096 + 2048) + 8 * 2 * 1024 + 36
    same_bits(columns(s, ws_bytes=2304 + 100 * per_col + per_col // 2), whole)
    # ... and the other layout, whose columns cost 8 n less: other blocks, the same bits
    same_bits(columns(np.ascontiguousarray(s.T).T, ws_bytes=2304 + 100 * per_col + per_col // 2), whole)


def test_impossible_cap(g):
    from inference_amd import _lib

    with pytest.raises(_lib.GpmiError, match="one column"):
        columns(eh.checked_case(g, "ramp_4096"), ws_bytes=8 * 4096)


def test_columns_finishing_in_different_rounds(g):
    """ar_4096 has cuts from 2 to 1192, so every round of the batch runs on fewer columns than the one before: each
    column's numbers are those of its own single-column call."""
    from inference_amd.pdf import _device

    s = eh.checked_case(g, "ar_4096")
    whole = columns(s)
    blocks = np.array(_device.acf_lag_blocks(4096))
    rounds = np.searchsorted(blocks, whole[2], side="right")
    assert sorted(set(rounds.tolist())) == [1, 2, 3, 4]  # columns leave after each of the four rounds
    for c in range(s.shape[1]):
        alone = columns(s[:, c].copy().reshape(-1, 1))
        for k in range(3):
            assert_array_equal(alone[k][0], whole[k][c], err_msg=f"column {c}, output {k}")


@pytest.mark.parametrize("m", eh.LAYOUT_M)
def test_column_counts(g, m):
    a = eh.checked_case(g, "layout")
    ess, f0, total, cut = batch(np.ascontiguousarray(a[:, :m]))
    assert_array_equal(cut, g["layout_cut"][:m])
    assert_array_equal(ess, g["layout_ess"][:m])
    assert_allclose(f0, g["layout_f0"][:m], rtol=eh.TOL, atol=0)
    assert_allclose(total, g["layout_sum"][:m], rtol=eh.TOL, atol=0)


def test_views(g, monkeypatch):
    import ctypes

    from inference_amd.pdf import _device

    a = eh.checked_case(g, "layout")
    ref = columns(a)
    against(batch(a), g, "layout")
    seen = []
    inner = _device._call

    def spy(h, name, ctx, n, m, row_stride, col_stride, pointer, *rest):
        seen.append((name, n, m, row_stride, col_stride, ctypes.cast(pointer, ctypes.c_void_p).value))
        return inner(h, name, ctx, n, m, row_stride, col_stride, pointer, *rest)

    monkeypatch.setattr(_device, "_call", spy)
    # a C-order view with ld > m: read in place
    v = a[:, 3:40]
    same_bits(columns(v), [r[3:40] for r in ref])
    assert seen[-1] == ("gpmi_acf_columns", 258, 37, 129, 1, v.ctypes.data)
    # the column-contiguous layout: the transpose of a C array, read in place
    b = np.ascontiguousarray(a.T)
    same_bits(columns(b.T), ref)
    assert seen[-1] == ("gpmi_acf_columns", 258, 129, 1, 258, b.ctypes.data)
    same_bits(columns(b[5:70].T), [r[5:70] for r in ref])
    first_rows = columns(b[:, :200].T)  # ld > n
    assert seen[-1][1:5] == (200, 129, 1, 258)
    same_bits([r[:3] for r in first_rows], columns(np.ascontiguousarray(a[:200, :3])))
    # a view that is dense in neither order goes through a C-contiguous copy and gives the same numbers
    w = a[:, ::2]
    same_bits(columns(w), [r[::2] for r in ref])
    assert seen[-1][1:5] == (258, 65, 65, 1) and seen[-1][5] != w.ctypes.data
    # float32 input is widened to float64
    f32 = a[:, :5].astype(np.float32)
    same_bits(batch(f32), batch(f32.astype(np.float64)))


def test_flags_and_errors(g):
    from inference_amd import _lib
    from inference_amd.mcmc import effective_sample_size_batch
    from inference_amd.pdf import _device

    const = eh.checked_case(g, "const")
    f0, total, cut, flags = columns(const)
    assert flags.tolist() == [2, 0, 1]
    assert cut[1] >= 1 and f0[1] > 0
    assert columns(np.ascontiguousarray(const.T).T)[3].tolist() == [2, 0, 1]
    with pytest.raises(IndexError):
        effective_sample_size_batch(const)
    with pytest.raises(IndexError):
        effective_sample_size_batch(const[:, 2])
    assert effective_sample_size_batch(const[:, 1]).tolist() == [int(64 / (total[1] / f0[1]))]
    with pytest.raises(IndexError):
        effective_sample_size_batch(eh.checked_case(g, "tiny_2"))
    assert columns(eh.case("tiny_2"))[3].tolist() == [2]
    assert columns(np.arange(3.0).reshape(3, 1))[3].tolist() == [2]  # n < 4: no lag in [1, n // 2)
    assert_array_equal(effective_sample_size_batch(eh.checked_case(g, "tiny_4")), g["tiny_4_ess"])

    # bad strides, n < 2 and m < 1 are GPMI_ERR_ARG
    h = _device.handle()
    import ctypes as C

    x = np.zeros((8, 4))
    out = [np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int32)]
    ptrs = (_lib.dptr(out[0]), _lib.dptr(out[1]), out[2].ctypes.data_as(C.POINTER(C.c_int64)),
            out[3].ctypes.data_as(C.POINTER(C.c_int32)))
    for n, m, rs, cs, text in ((8, 4, 3, 1, "strides"), (8, 4, 1, 7, "strides"), (8, 4, 2, 2, "strides"), (1, 4, 4, 1, "n out of range"),
                               (8, 0, 4, 1, "m out of range")):
        with pytest.raises(_lib.GpmiError, match=f"status -1.*{text}"):
            _device._call(h, "gpmi_acf_columns", h.ctx, n, m, rs, cs, _lib.dptr(x), 0, *ptrs)
    # and the handle is fine afterwards
    assert_array_equal(effective_sample_size_batch(eh.case("tiny_4")), g["tiny_4_ess"])


def test_chain_diagnostics(g, monkeypatch):
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from inference_amd.pdf import _device

    chain = eh.rebuilt_chain(g)
    calls = []
    inner = _device._call

    def spy(h, name, *args):
        calls.append((name, args[1:3]))
        return inner(h, name, *args)

    monkeypatch.setattr(_device, "_call", spy)
    data = chain.diagnostics_data()
    burn = int(g["chain_burn"])
    assert data["burn"] == burn
    rows = chain.chain_length - burn
    assert calls == [("gpmi_acf_columns", (rows, 3))]  # one device call for all parameters
    branch = "the reference's integers (even length)" if rows % 2 == 0 else "the mirror's integers (odd length)"
    print(f"chain_length - burn = {rows}: compared with {branch}")
    assert_array_equal(data["ess"], g["chain_ess"] if rows % 2 == 0 else g["chain_mirror_ess"])
    assert data["ess_mean"] == int(np.mean(data["ess"])) and data["ess_min"] == int(min(data["ess"]))
    assert type(data["ess_mean"]) is int and type(data["ess_min"]) is int
    assert_array_equal(data["probs"], g["chain_probs"])
    assert_array_equal(data["step_axis"], np.arange(chain.chain_length) * 1e-3)
    half = g["chain_probs"][chain.chain_length // 2:].min()
    assert data["prob_ylims"] == [half, g["chain_probs"].max() * 1.1 - 0.1 * half]
    for k in range(3):
        v = g[f"chain_sigma_values_{k}"]
        assert_array_equal(data["width_steps"][k], g[f"chain_sigma_checks_{k}"][1:] * 1e-3)
        assert_array_equal(data["width_percent_change"][k], 1e2 * np.diff(v) / v[:-1])
    # a burn of the caller's choosing
    assert chain.diagnostics_data(burn=burn + 1)["burn"] == burn + 1
    assert calls[-1] == ("gpmi_acf_columns", (rows - 1, 3))

    fig = chain.plot_diagnostics(show=False)
    assert len(fig.axes) == 4
    assert [t.get_text() for t in fig.axes[3].texts][1::2] == ["{:.5G}".format(v) for v in (burn, data["ess_mean"], data["ess_min"])]
    assert_array_equal([b.get_height() for b in fig.axes[2].patches], data["ess"])
    plt.close("all")


def test_ess_bench_tool_runs():
    import os
    import subprocess
    import sys

    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ess_bench.py"), "--tiny", "--reps", "1"], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "batch" in r.stdout and "host" in r.stdout
