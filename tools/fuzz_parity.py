"""Randomised parity sweep against the CPU oracle: random sizes, dimensions, kernels, noise levels; fit, LML and LOO with
gradients, predict, posterior, and (SquaredExponential) the spatial gradients.  tests/test_gpu_parity.py runs a seeded
sweep of it (`sweep`), tests/test_ycov_gpu.py one with dense data errors (`dense_noise=True`); from the command line:
python tools/fuzz_parity.py [seed] [cases] [max N] [dense]."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "inference-tools_amd")]
import numpy as np
import workloads as wl
from inference_amd.gp import GpRegressor, SquaredExponential, RationalQuadratic, WhiteNoise
from oracle import gp_oracle as orc

def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))

def dense_errors(e, perm):
    """A dense data-error covariance with the variances e_i^2 on its diagonal: (e_i e_j) 2^-|p_i - p_j| for a permutation p
    (a permuted Kac-Murdock-Szego matrix, symmetric bit for bit, its large entries far from the diagonal)."""
    return (e[:, None] * e[None, :]) * np.ldexp(1.0, -np.abs(perm[:, None] - perm[None, :]))

def sweep(seed=0, cases=16, nmax=2600, verbose=True, dense_noise=False):
    """-> list of (description, {quantity: relative error}) for `cases` random problems.  `dense_noise`: the data errors
    enter as a dense y_cov (`dense_errors`, its permutation drawn from a generator of its own, so that the problems are
    otherwise those of the same seed without it)."""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(cases):
        n = int(rng.integers(2, nmax)); d = int(rng.integers(1, 12)); kid = int(rng.integers(0, 2)); wn = bool(rng.integers(0, 2))
        x, y, e = wl.synthetic_dataset(1000 * seed + case, n, d)
        e = e * float(rng.uniform(0.5, 3.0))
        th = wl.timing_theta(kid, y, d) + 0.2 * rng.standard_normal(wl.timing_theta(kid, y, d).size)
        cov = (SquaredExponential if kid == wl.SE else RationalQuadratic)()
        if wn:
            cov = cov + WhiteNoise(); th = np.append(th, np.log(0.05))
        if dense_noise:
            Y = dense_errors(e, np.random.default_rng([seed, case]).permutation(n))
            gp = GpRegressor(x, y, y_cov=Y, hyperpars=th, kernel=cov)
            ref = orc.OracleGp(x, y, y_cov=Y, kernel=kid, hyperpars=th, white_noise=wn)
        else:
            gp = GpRegressor(x, y, y_err=e, hyperpars=th, kernel=cov)
            ref = orc.OracleGp(x, y, e, kernel=kid, hyperpars=th, white_noise=wn)
        m = int(rng.integers(1, 70))
        pts = wl.query_points(case, m, d)
        mu, sig = gp(pts); rmu, rsig = ref(pts)
        l, g = gp.marginal_likelihood_gradient(th); rl, rg = ref.marginal_likelihood_gradient(th)
        lo, go = gp.loo_likelihood_gradient(th); rlo, rgo = ref.loo_likelihood_gradient(th)
        pm, pc = gp.build_posterior(pts); rpm, rpc = ref.build_posterior(pts)
        errs = dict(alpha=rel(gp.alpha, ref.alpha), mu=rel(mu, rmu), sig=rel(sig, rsig), lml=rel(l, rl), grad=rel(g, rg),
                    loo=rel(lo, rlo), loo_grad=rel(go, rgo), post_mean=rel(pm, rpm), post_cov=rel(pc, rpc))
        if kid == wl.SE:
            dm, dv = gp.spatial_derivatives(pts); rdm, rdv = ref.spatial_derivatives(pts)
            errs.update(dmu=rel(dm, rdm), dvar=rel(dv, rdv))
        desc = f"n={n:5d} d={d:2d} m={m:2d} kernel={'SE' if kid == 0 else 'RQ'}{'+WN' if wn else '   '}{' dense y_cov' if dense_noise else ''}"
        out.append((desc, errs))
        if verbose:
            print(f"{desc}  worst {max(errs.values()):.2e}  " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()), flush=True)
    return out


if __name__ == "__main__":
    res = sweep(int(sys.argv[1]) if len(sys.argv) > 1 else 0, int(sys.argv[2]) if len(sys.argv) > 2 else 16,
                int(sys.argv[3]) if len(sys.argv) > 3 else 2600, dense_noise=len(sys.argv) > 4 and sys.argv[4] == "dense")
    worst = {}
    for _, errs in res:
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst relative error per quantity:", " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
