"""
Golden vectors of the reference's KDE2D (pdf/kde.py:256-280) and of the arrays its matrix_plot draws
(plotting.py:139-245), written to kde2d.npz beside this file by IMPORTING the reference the way make_golden.py does
(its module level sets that import up; the file itself is not changed).

Run in the build container only:   python tests/golden/make_golden_kde2d.py

Cases (prefix in the archive).  Each density case records x, y, q_x, q_y, norm, scattered points (px, py) with their
densities (pdf), a 50 x 50 grid (gx, gy, grid) and the density at every sample (self).
  corr        n = 3000, correlation 0.8; ~1500 points from the core out to 10 standard deviations (exact zeros included)
  banana      n = 5000 on a curved ridge
  tiny        n = 3
  ties        n = 2000, both columns rounded to 0.1
  shift       n = 2000 centred at 10^6 with unit spread (cancellation in x_j - a)
  calls       on corr's sample: a scalar call, a list call, arguments of unequal length (zip truncation)
  degenerate  y = 2 x: infinite scales, every value NaN
  mp          4 parameters, n = 4000, two correlated pairs and one skewed column: every array matrix_plot computes for the
              styles "contour" and "hdi", assembled from sample_hdi, GaussianKDE and KDE2D exactly as matrix_plot calls them
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.pdf import GaussianKDE, sample_hdi  # noqa: E402
from inference.pdf.kde import KDE2D  # noqa: E402

OUT = {}


def scattered(rng, x, y, m_core, m_far, m_own):
    """Points around the sample: a core cloud, a ring from 3 to 10 standard deviations, and some of the samples."""
    cx, cy, sx, sy = x.mean(), y.mean(), x.std(), y.std()
    r = rng.uniform(3.0, 10.0, m_far)
    phi = rng.uniform(0.0, 2 * np.pi, m_far)
    own = rng.integers(0, x.size, m_own)
    px = np.concatenate([cx + 1.5 * sx * rng.normal(size=m_core), cx + sx * r * np.cos(phi), x[own]])
    py = np.concatenate([cy + 1.5 * sy * rng.normal(size=m_core), cy + sy * r * np.sin(phi), y[own]])
    return px, py


def record(prefix, rng, x, y, m=(1000, 400, 100), g=50):
    pdf = KDE2D(x=x, y=y)
    OUT[f"{prefix}_x"], OUT[f"{prefix}_y"] = x, y
    OUT[f"{prefix}_q_x"], OUT[f"{prefix}_q_y"], OUT[f"{prefix}_norm"] = map(np.float64, (pdf.q_x, pdf.q_y, pdf.norm))
    px, py = scattered(rng, x, y, *m)
    OUT[f"{prefix}_px"], OUT[f"{prefix}_py"] = px, py
    OUT[f"{prefix}_pdf"] = np.array(pdf(px, py))
    gx = np.linspace(x.min() - 0.5 * x.std(), x.max() + 0.5 * x.std(), g)
    gy = np.linspace(y.min() - 0.5 * y.std(), y.max() + 0.5 * y.std(), g)
    X, Y = np.meshgrid(gx, gy)
    OUT[f"{prefix}_gx"], OUT[f"{prefix}_gy"] = gx, gy
    OUT[f"{prefix}_grid"] = np.array(pdf(X.flatten(), Y.flatten())).reshape(g, g)
    OUT[f"{prefix}_self"] = np.array(pdf(x, y))
    return pdf


def main():
    rng = np.random.default_rng(20261017)
    z = rng.normal(size=(2, 3000))
    corr = record("corr", rng, 1.0 + 2.0 * z[0], -3.0 + 0.5 * (0.8 * z[0] + 0.6 * z[1]))
    assert (OUT["corr_pdf"] == 0.0).any() and (OUT["corr_pdf"] > 0.0).any()

    t = rng.normal(size=5000)
    record("banana", rng, t + 0.1 * rng.normal(size=5000), t**2 + 0.3 * rng.normal(size=5000))
    record("tiny", rng, np.array([0.3, -1.2, 2.5]), np.array([1.0, 0.4, -0.7]), m=(60, 30, 3), g=20)
    record("ties", rng, np.round(rng.normal(size=2000), 1), np.round(rng.normal(2.0, 3.0, 2000), 1), m=(400, 150, 50))
    record("shift", rng, 1e6 + rng.normal(size=2000), -1e6 + rng.normal(size=2000), m=(400, 150, 50))

    # the forms of __call__
    px, py = OUT["corr_px"], OUT["corr_py"]
    OUT["calls_scalar"] = np.float64(corr(float(px[3]), float(py[3])))
    OUT["calls_list"] = np.array(corr(list(px[:7]), list(py[:7])))
    OUT["calls_unequal"] = np.array(corr(px[:9], py[:5]))
    assert isinstance(corr(list(px[:7]), list(py[:7])), list) and OUT["calls_unequal"].size == 5

    xd = rng.integers(-40, 41, 500) / 8.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        deg = KDE2D(x=xd, y=2 * xd)
        OUT["degenerate_x"] = xd
        OUT["degenerate_scales"] = np.array([deg.q_x, deg.q_y, deg.norm])
        OUT["degenerate_pdf"] = np.array(deg(xd[:20] + 0.1, 2 * xd[:20]))
        OUT["degenerate_scalar"] = np.float64(deg(0.1, 0.3))
    assert np.isnan(OUT["degenerate_pdf"]).all() and np.isnan(OUT["degenerate_scalar"]), OUT["degenerate_scales"]

    # the arrays of matrix_plot (plotting.py:139-245) for "contour" and "hdi"
    n = 4000
    w = rng.normal(size=(4, n))
    samples = [w[0], 2.0 + 0.7 * w[0] + 0.5 * w[1], np.exp(0.5 * w[2]), -1.0 + 0.3 * (0.9 * w[2] + 0.45 * w[3])]
    fractions = (0.35, 0.65, 0.95)
    L = 200
    OUT["mp_samples"] = np.array(samples)
    OUT["mp_hdi_fractions"] = np.array(fractions)
    limits, arrays, marginals = [], [], []
    for sample in samples:
        lwr, upr = sample_hdi(sample, fraction=0.98)
        limits.append([lwr - (upr - lwr) * 0.3, upr + (upr - lwr) * 0.3])
        arrays.append(np.linspace(lwr - (upr - lwr) * 0.35, upr + (upr - lwr) * 0.35, L))
        marginals.append(np.array(GaussianKDE(sample)(arrays[-1])))
    OUT["mp_axis_limits"], OUT["mp_axis_arrays"], OUT["mp_marginals"] = map(np.array, (limits, arrays, marginals))
    for i in range(4):
        for j in range(i):
            x, y = samples[j], samples[i]
            pdf = KDE2D(x=x, y=y)
            sample_probs = pdf(x, y)
            pcts = [100 * (1 - f) for f in fractions]
            levels = [lv for lv in np.percentile(sample_probs, pcts)]
            X, Y = np.meshgrid(arrays[j][::4], arrays[i][::4])
            prob = np.array(pdf(X.flatten(), Y.flatten())).reshape([L // 4, L // 4])
            levels.append(prob.max())
            OUT[f"mp_prob_{i}{j}"] = prob  # the same array for both styles
            OUT[f"mp_levels_{i}{j}"] = np.array(sorted(levels))

    path = os.path.join(HERE, "kde2d.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
