"""
Golden vectors of GpRegressor with a DENSE data-error covariance (`y_cov`, regression.py:133, 239, 246-293, 475, 498, 534,
552 of the reference: K = cov(theta) + Y in every method), written to ycov.npz beside this file by IMPORTING the reference
the way make_golden.py does (its module level sets that import up; the file itself is not changed).

Run in the build container only:   python tests/golden/make_golden_ycov.py

The matrices Y come from tests/ycov_builders.py: kind (a) (`correlated_cov`) is stored, kind (b) (`kms_cov`, a permuted
Kac-Murdock-Szego matrix that every machine rebuilds bit for bit) is stored as its permutation plus 64 probe entries.

Cases
  se       SquaredExponential, N = 200, d = 2, Y of kind (a); K_xx at 64 rows / columns
  rqwn     RationalQuadratic + WhiteNoise, N = 130, d = 3 (ragged), Y of kind (a)
  serq     SE + RQ (a sum of stationary kernels), N = 200, d = 2, Y of kind (b)
  cp       ChangePoint([SE, RQ], axis = 0), N = 240, d = 2, Y of kind (b)
  het      SE + HeteroscedasticNoise, N = 150, d = 1, Y of kind (b)
  se1500   SquaredExponential, N = 1500, d = 3 (not a multiple of 64), Y of kind (b)
Per case: labels, bounds, alpha, mu / sigma at 40 query points, the posterior at 16 of them, loo_predictions, LML, LML
gradient, LOO and LOO gradient at three thetas; for the SE cases `gradient` and `spatial_derivatives` at the query points;
for se, rqwn and serq one seeded n_starts = 3 search (numpy.random.seed(7), as make_golden_sum.py).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
import ycov_builders as yb  # noqa: E402

SE, RQ, WN, HET, CP = "se", "rq", "wn", "het", "cp"

# tag: (model, N, d, kind of Y, seed, search)
CASES = {
    "se": (SE, 200, 2, "a", 21, True),
    "rqwn": ((RQ, WN), 130, 3, "a", 22, True),
    "serq": ((SE, RQ), 200, 2, "b", 23, True),
    "cp": (CP, 240, 2, "b", 24, False),
    "het": ((SE, HET), 150, 1, "b", 25, False),
    "se1500": (SE, 1500, 3, "b", 26, False),
}


def make_cov(model):
    if model == SE:
        return mg.SquaredExponential()
    if model == CP:
        return mg.ChangePoint(kernels=[mg.SquaredExponential, mg.RationalQuadratic], axis=0)
    parts = [{SE: mg.SquaredExponential, RQ: mg.RationalQuadratic, WN: mg.WhiteNoise, HET: mg.HeteroscedasticNoise}[k]()
             for k in model]
    cov = parts[0]
    for p in parts[1:]:
        cov = cov + p
    return cov


def dataset(seed, n, d):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, d))
    y = np.sin(4 * x.sum(axis=1)) + 0.3 * np.cos(23 * x[:, 0]) + 0.05 * rng.normal(size=n)
    pts = rng.uniform(0, 1, (40, d))
    return rng, x, y, pts


def stationary_theta(kind, d, ell, k):
    th = [-0.3 + 0.1 * k] + ([0.3 - 0.1 * k] if kind == RQ else [])
    return th + [np.log(ell) + 0.05 * (k + i) for i in range(d)]


def thetas_for(model, d, n, k, rng):
    """Hyper-parameters of step k (mean parameter first)."""
    th = [0.05 * k]
    if model == SE:
        return np.array(th + stationary_theta(SE, d, 0.3, k))
    if model == CP:
        th += stationary_theta(SE, d, 0.4, k) + stationary_theta(RQ, d, 0.08, k)
        return np.array(th + [0.45 + 0.03 * k, 0.05 + 0.02 * k])
    for kind, ell in zip(model, (0.4, 0.1)):
        if kind == WN:
            th.append(np.log(0.02) + 0.1 * k)
        elif kind == HET:
            th += list(np.log(0.05) + 0.3 * rng.standard_normal(n))
        else:
            th += stationary_theta(kind, d, ell, k)
    return np.array(th)


def make_y_cov(kind, n, rng, tag, out):
    if kind == "a":
        Y = yb.correlated_cov(*yb.correlated_cov_inputs(rng, n))
        out[f"{tag}_Y"] = Y
        return Y
    p = rng.permutation(n)
    Y = yb.kms_cov(p)
    ij = yb.kms_probes(p, rng)
    out[f"{tag}_perm"] = p
    out[f"{tag}_probe_ij"] = ij
    out[f"{tag}_probe_val"] = Y[ij[:, 0], ij[:, 1]]
    return Y


def run_case(tag, model, n, d, kind, seed, search, out):
    rng, x, y, pts = dataset(seed, n, d)
    Y = make_y_cov(kind, n, rng, tag, out)
    thetas = np.array([thetas_for(model, d, n, k, rng) for k in range(3)])
    gp = mg.GpRegressor(x, y, y_cov=Y, kernel=make_cov(model), hyperpars=thetas[0])
    out[f"{tag}_x"], out[f"{tag}_y"], out[f"{tag}_pts"] = x, y, pts
    out[f"{tag}_thetas"] = thetas
    out[f"{tag}_labels"] = np.array(gp.hyperpar_labels)
    out[f"{tag}_bounds"] = np.array(gp.hp_bounds, dtype=float)
    if tag == "se":
        ii = mg.idx64(n)
        out[f"{tag}_K_idx"] = ii
        out[f"{tag}_K_sub"] = gp.K_xx[np.ix_(ii, ii)]
    out[f"{tag}_alpha"] = gp.alpha
    mu, sig = gp(pts)
    out[f"{tag}_mu"], out[f"{tag}_sig"] = mu, sig
    pm, pc = gp.build_posterior(pts[:16])
    out[f"{tag}_post_mu"], out[f"{tag}_post_cov"] = pm, pc
    loo_mu, loo_sig = gp.loo_predictions()
    out[f"{tag}_loo_mu"], out[f"{tag}_loo_sig"] = loo_mu, loo_sig
    if model == SE:
        g_mu, g_cov = gp.gradient(pts)
        out[f"{tag}_grad_mu"], out[f"{tag}_grad_cov"] = g_mu, g_cov
        s_mu, s_var = gp.spatial_derivatives(pts)
        out[f"{tag}_sd_mu"], out[f"{tag}_sd_var"] = s_mu, s_var
    out[f"{tag}_lml"] = np.array([gp.marginal_likelihood(t) for t in thetas])
    out[f"{tag}_lml_grad"] = np.array([gp.marginal_likelihood_gradient(t)[1] for t in thetas])
    out[f"{tag}_loo"] = np.array([gp.loo_likelihood(t) for t in thetas])
    out[f"{tag}_loo_grad"] = np.array([gp.loo_likelihood_gradient(t)[1] for t in thetas])
    if search:
        # regression.py:589-605 draws its starting positions from the legacy global generator
        np.random.seed(7)
        gs = mg.GpRegressor(x, y, y_cov=Y, kernel=make_cov(model), n_starts=3)
        out[f"{tag}_search_theta"] = np.asarray(gs.hyperpars, dtype=float)
        out[f"{tag}_search_lml"] = np.array(gs.marginal_likelihood(gs.hyperpars))


def main():
    out = {}
    for tag, spec in CASES.items():
        run_case(tag, *spec, out)
    path = os.path.join(HERE, "ycov.npz")
    np.savez_compressed(path, allow_pickle=False, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
