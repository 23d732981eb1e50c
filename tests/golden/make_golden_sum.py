"""
Golden vectors of sums of stationary covariance kernels (CompositeCovariance: covariance.py:33-36, 47-105 of the
reference), written to sum.npz beside this file by IMPORTING the reference the way make_golden.py does (its module
level sets that import up; its helpers are reused, the file itself is not changed).

Run in the build container only:   python tests/golden/make_golden_sum.py

Cases (all with y_err > 0)
  serq      SquaredExponential + RationalQuadratic, N = 200, d = 2 (K_xx recorded: the smallest case)
  sese      SE + SE with a long and a short length scale, N = 300, d = 1
  serqwn    SE + RQ + WhiteNoise, N = 200, d = 2
  rqsesewn  RQ + SE + SE + WhiteNoise, N = 520, d = 3 (ragged: not a multiple of 64)
Per case: labels, bounds, alpha, mu / sigma at query points, the posterior, LML, LML gradient, LOO and LOO gradient at
three thetas, loo_predictions, and one seeded n_starts = 3 search (numpy.random.seed, as case_search does).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402

SE, RQ, WN = "se", "rq", "wn"


def make_cov(kinds):
    parts = [{SE: mg.SquaredExponential, RQ: mg.RationalQuadratic, WN: mg.WhiteNoise}[k]() for k in kinds]
    cov = parts[0]
    for p in parts[1:]:
        cov = cov + p
    return cov


def thetas_for(kinds, d, ells, k):
    """Covariance parameters of step k (mean parameter first)."""
    th = [0.05 * k]
    ell = iter(ells)
    for kind in kinds:
        if kind == WN:
            th.append(np.log(0.02) + 0.1 * k)
            continue
        le = next(ell)
        th.append(-0.3 + 0.1 * k)
        if kind == RQ:
            th.append(0.3 - 0.1 * k)
        th += [np.log(le) + 0.05 * (k + i) for i in range(d)]
    return np.array(th)


def dataset(seed, n, d):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, d))
    y = np.sin(4 * x.sum(axis=1)) + 0.3 * np.cos(23 * x[:, 0]) + 0.05 * rng.normal(size=n)
    e = np.full(n, 0.05) + 0.01 * rng.uniform(size=n)
    pts = rng.uniform(0, 1, (40, d))
    return x, y, e, pts


CASES = {
    "serq": ((SE, RQ), 200, 2, (0.5, 0.1), 11),
    "sese": ((SE, SE), 300, 1, (0.6, 0.04), 12),
    "serqwn": ((SE, RQ, WN), 200, 2, (0.4, 0.08), 13),
    "rqsesewn": ((RQ, SE, SE, WN), 520, 3, (0.7, 0.3, 0.06), 14),
}


def run_case(tag, kinds, n, d, ells, seed, out):
    x, y, e, pts = dataset(seed, n, d)
    thetas = np.array([thetas_for(kinds, d, ells, k) for k in range(3)])
    gp = mg.GpRegressor(x, y, y_err=e, kernel=make_cov(kinds), hyperpars=thetas[0])
    out[f"{tag}_x"], out[f"{tag}_y"], out[f"{tag}_y_err"], out[f"{tag}_pts"] = x, y, e, pts
    out[f"{tag}_thetas"] = thetas
    out[f"{tag}_labels"] = np.array(gp.hyperpar_labels)
    out[f"{tag}_bounds"] = np.array(gp.hp_bounds, dtype=float)
    if tag == "serq":
        out[f"{tag}_K_xx"] = gp.K_xx
    out[f"{tag}_alpha"] = gp.alpha
    mu, sig = gp(pts)
    out[f"{tag}_mu"], out[f"{tag}_sig"] = mu, sig
    pm, pc = gp.build_posterior(pts[:16])
    out[f"{tag}_post_mu"], out[f"{tag}_post_cov"] = pm, pc
    loo_mu, loo_sig = gp.loo_predictions()
    out[f"{tag}_loo_mu"], out[f"{tag}_loo_sig"] = loo_mu, loo_sig
    out[f"{tag}_lml"] = np.array([gp.marginal_likelihood(t) for t in thetas])
    res = [gp.marginal_likelihood_gradient(t) for t in thetas]
    out[f"{tag}_lml_grad"] = np.array([r[1] for r in res])
    out[f"{tag}_loo"] = np.array([gp.loo_likelihood(t) for t in thetas])
    res = [gp.loo_likelihood_gradient(t) for t in thetas]
    out[f"{tag}_loo_grad"] = np.array([r[1] for r in res])
    # seeded search (regression.py:589-605 draws its starting positions from the legacy global generator)
    np.random.seed(7)
    gs = mg.GpRegressor(x, y, y_err=e, kernel=make_cov(kinds), n_starts=3)
    out[f"{tag}_search_theta"] = np.asarray(gs.hyperpars, dtype=float)
    out[f"{tag}_search_lml"] = np.array(gs.marginal_likelihood(gs.hyperpars))


def main():
    out = {}
    for tag, (kinds, n, d, ells, seed) in CASES.items():
        run_case(tag, kinds, n, d, ells, seed, out)
    path = os.path.join(HERE, "sum.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
