"""NumPy restatements for the KDE2D tests (test infrastructure only: the product has no CPU path).

`raw_sums` is the reference's KDE2D.density (pdf/kde.py:272-275) without `norm`, chunked over the points; `HostKDE2D` is
the product's class with its device seam (`_raw_sums`, and the two evaluations built on the same sums) filled by it;
`HostDensity1D` stands in for `_device.DeviceDensity` (the truncated slice sums of GaussianKDE), so that
`matrix_plot_data` can run on a host without a GPU."""
import numpy as np
from scipy.special import erf

from inference_amd.pdf.kde2d import KDE2D


def raw_sums(x, y, q_x, q_y, a, b, chunk_bytes=1 << 27):
    """sum_j exp(-((x_j - a_i) q_x)^2 - ((y_j - b_i) q_y)^2), a block of points at a time (blocks of chunk_bytes)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    out = np.empty(a.size)
    step = max(1, chunk_bytes // (8 * x.size))
    for i in range(0, a.size, step):
        z_x = ((x[None, :] - a[i:i + step, None]) * q_x) ** 2
        z_y = ((y[None, :] - b[i:i + step, None]) * q_y) ** 2
        out[i:i + step] = np.exp(-z_x - z_y).sum(axis=1)
    return out


class HostKDE2D(KDE2D):
    """KDE2D with NumPy sums: never opens a device."""

    calls = 0  # calls of the raw-sum seam, over all instances

    def _open_device(self):
        return None

    def _raw_sums(self, a, b):
        HostKDE2D.calls += 1
        return raw_sums(self.x, self.y, self.q_x, self.q_y, a, b)

    def _raw_self_sums(self):
        return self._raw_sums(self.x, self.y)

    def _raw_grid_sums(self, x_axis, y_axis):
        X, Y = np.meshgrid(x_axis, y_axis)
        return self._raw_sums(X.ravel(), Y.ravel()).reshape(y_axis.size, x_axis.size)


class HostDensity1D:
    """The slice sums of csrc/kde.hip in NumPy, with the constructor and `sums` of `_device.DeviceDensity`."""

    def __init__(self, sorted_sample, lo, hi, device=None):
        self.s, self.lo, self.hi = np.asarray(sorted_sample, dtype=np.float64), np.asarray(lo), np.asarray(hi)

    def sums(self, x, regions, q, pdf=True, cdf=True):
        ps, cs = np.empty(len(x)), np.empty(len(x))
        for i, (xi, ri) in enumerate(zip(x, regions)):
            t = (xi - self.s[self.lo[ri]:self.hi[ri]]) * q
            ps[i] = np.exp(-(t * t)).sum()
            cs[i] = (1 + erf(t)).sum()
        return (ps if pdf else None), (cs if cdf else None)


def density_close(got, ref, n, norm, what, note):
    """The parity bound of the 2-D densities: rtol 1e-12 plus n x 2.3e-308 x norm (a term flushed to zero, or a factor
    pair that underflows, loses at most the smallest normal double, n times over).  Prints the worst relative error
    through note(what, err) before it asserts."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    atol = n * 2.3e-308 * norm
    err = np.abs(got - ref)
    big = np.abs(ref) > 1e12 * atol
    note(what, (err[big] / np.abs(ref[big])).max(initial=0.0))
    excess = err - (atol + 1e-12 * np.abs(ref))
    assert (excess <= 0).all(), f"{what}: worst excess {excess.max():.3e} at rel {np.nanmax(err / np.abs(ref)):.3e}"


def check_matrix_plot_data(data, g, style, note):
    """matrix_plot_data against the golden case `mp`: axes and limits to 1e-12 of the parameter's range, 1-D estimates
    to rtol 1e-12 (atol 1e-300, as test_kde_gpu.py holds the pdf), pair grids to the density bound, levels to rtol 1e-11."""
    samples = g["mp_samples"]
    span = (samples.max(axis=1) - samples.min(axis=1))[:, None]
    for key in ("axis_limits", "axis_arrays"):
        err = (np.abs(data[key] - g[f"mp_{key}"]) / span).max()
        note(f"{key} / range", err)
        assert data[key].shape == g[f"mp_{key}"].shape and err <= 1e-12
    m, rm = data["marginals"], g["mp_marginals"]
    assert m.shape == rm.shape
    err = np.abs(m - rm)
    note("1-D estimates", (err[rm > 1e-280] / rm[rm > 1e-280]).max(initial=0.0))
    assert (err <= 1e-300 + 1e-12 * rm).all()
    n = samples.shape[1]
    assert sorted(data["pairs"]) == [(i, j) for i in range(4) for j in range(i)]
    for (i, j), pair in data["pairs"].items():
        np.testing.assert_array_equal(pair["x"], data["axis_arrays"][j][::4])
        np.testing.assert_array_equal(pair["y"], data["axis_arrays"][i][::4])
        from inference_amd.pdf.kde2d import estimate_bandwidth, scales

        norm = scales(n, *estimate_bandwidth(samples[j], samples[i]))[2]
        density_close(pair["prob"], g[f"mp_prob_{i}{j}"], n, norm, f"pair grid ({style})", note)
        if style == "hdi":
            lv, rl = pair["levels"], g[f"mp_levels_{i}{j}"]
            assert lv.shape == rl.shape == (4,)
            err = (np.abs(lv - rl) / rl).max()
            note("hdi levels", err)
            assert err <= 1e-11, (i, j, lv, rl)
        else:
            assert "levels" not in pair
