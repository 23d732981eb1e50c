"""Shared pieces of the highest-density-interval tests (test infrastructure only: the product has no CPU path).

`case(name)` rebuilds the seeded inputs of golden/hdi.npz (golden/make_golden_hdi.py draws them from here too, and stores
the first and last 8 values of every drawn array, which `checked_case` compares); `HostHdi` is a NumPy stand-in for
`_device.hdi_columns` that counts its calls, so that `sample_hdi_batch` and the plot data can run without a GPU."""
import numpy as np

FRACTIONS = (0.10, 0.65, 0.95)
TINY_FRACTIONS = (0.001, 0.5, 0.999)  # int(f * n) = 0 and n - 1 at the ends, for every n of TINY_N
TIE_FRACTIONS = (0.10, 0.5, 0.65, 0.95)
BAND_INTERVALS = (0.95, 0.35, 0.65)
EDGE_N = [2 ** k + d for k in range(10, 16) for d in (-1, 0, 1)]
TINY_N = [2, 3, 5, 63, 64, 65, 257]
RUNS = [(3 * 2 ** 14 + 5, 2), (5 * 2 ** 13 + 1, 2), (100003, 2), (1000003, 1)]
LAYOUT_M = [1, 2, 15, 16, 17, 31, 33, 63, 65, 129]
RAGGED = [500, 700, 900, 1100, 1300]


def _ties(n, seed, n_int):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 5, size=(n, n_int)).astype(float)
    two = np.where(rng.random(n) < 0.4, -1.5, 2.25)
    return np.column_stack([a, np.full(n, 3.25), two])


def _nonfinite(n, seed):
    a = np.random.default_rng(seed).normal(size=(n, 6))
    a[n // 3, 1] = np.nan
    a[n // 2, 3] = np.inf
    a[n // 4, 4] = -np.inf
    a[n - 2, 4] = np.inf
    return a


def _curves(n, k, seed):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, k)
    return np.sin(6.0 * x)[None, :] * rng.normal(1.0, 0.2, size=(n, 1)) + rng.normal(0.0, 0.3, size=(n, k)) * (0.5 + x)[None, :]


def case(name):
    """The input of a golden case, drawn again from its seed."""
    kind, _, arg = name.partition("_")
    if kind == "edge":
        return np.random.default_rng(2000 + int(arg)).normal(size=(int(arg), 3))
    if kind == "tiny":
        return np.random.default_rng(3000 + int(arg)).normal(size=(int(arg), 4))
    if kind == "runs":
        n = int(arg)
        return np.random.default_rng(4000 + n % 1000).standard_t(3, size=(n, dict(RUNS)[n]))
    if name == "layout":
        return np.random.default_rng(5000).normal(size=(257, 129))
    if name == "tie_small":
        return _ties(50, 1, 4)
    if name == "tie_big":
        return _ties(20000, 2, 3)
    if name == "nf_small":
        return _nonfinite(40, 6000)
    if name == "nf_big":
        return _nonfinite(20000, 6001)
    if name == "band_a":
        return _curves(400, 60, 7000)
    if name == "band_b":
        return _curves(400, 60, 7001).T.copy()  # (60, 400): the orientation hdi_plot transposes
    if name == "trace":
        rng = np.random.default_rng(8000)
        return np.stack([rng.normal(k, 1.0 + k, 3000) if k % 2 else rng.gamma(2.0 + k, 1.0, 3000) for k in range(5)])
    if name == "ragged":
        rng = np.random.default_rng(8001)
        return [rng.normal(-k, 0.5 + k, size) for k, size in enumerate(RAGGED)]
    raise KeyError(name)


def ends(a):
    """First and last 8 values of a drawn array (of every array of a list)."""
    parts = a if isinstance(a, list) else [a]
    return np.concatenate([np.concatenate([np.ravel(p)[:8], np.ravel(p)[-8:]]) for p in parts])


def checked_case(g, name):
    """`case(name)`, checked against the ends that the golden file recorded when the reference ran on it."""
    a = case(name)
    np.testing.assert_array_equal(ends(a), g[f"{name}_ends"], err_msg=f"the seeded recipe of {name} drew other numbers")
    return a


class HostHdi:
    """`_device.hdi_columns` in NumPy: a sort per column, the window widths and the first minimum."""

    def __init__(self):
        self.calls = []

    def __call__(self, sample2d, Ls, device=None, ws_bytes=0):
        s = np.array(sample2d, dtype=np.float64)
        assert s.ndim == 2
        n, m = s.shape
        self.calls.append(((n, m), tuple(int(L) for L in Ls)))
        flags = ~np.isfinite(s).all(axis=0)
        s.sort(axis=0)
        out = np.empty((len(Ls), 2, m))
        for k, L in enumerate(Ls):
            if L >= n:
                out[k, 0], out[k, 1] = s[0], s[-1]
            else:
                i = (s[L:] - s[:n - L]).argmin(axis=0)
                cols = np.arange(m)
                out[k, 0], out[k, 1] = s[i, cols], s[i + L, cols]
        out[:, :, flags] = -12345.0  # what a flagged column holds means nothing: the caller must not use it
        return out, flags
