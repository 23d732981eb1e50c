"""Digests of a fixed, seeded list of small cases through the pair-tile kernels (csrc/pair_tile.h: the covariance builders
of kbuild.hip and the contractions of sparse.hip), to compare two builds of the library bit for bit:

    GPMI_LIB=<another libgpmi.so> python tools/sparse_bits.py a.npz > a.txt;  python tools/sparse_bits.py b.npz > b.txt;  diff a.txt b.txt

Every output array goes into the .npz and one SHA-256 line per array is printed (same order in every run).
Sparse cases: the four kernels, d in {1, 3, 17, 64} (d = 64: more than 64 KiB of LDS in the two column kernels), n = 200,
m = 70 (a full and a ragged tile of inducing inputs), panel_rows 128 (two panels: the accumulate passes) and 0 (one);
bound with gradient and alpha, bound_zgrad, fit, predict, posterior, posterior draws from supplied normals, spatial
derivatives at M = 1 and 130 with and without the variance part.
Builder cases: GpRegressor fits (alpha, log-determinant, mean and sigma at 130 points) at n in {130, 300}, d in {1, 17} for
the four kernels and a sum of two; a lockstep LML batch of three thetas, a lockstep predict batch, Matern spatial
derivatives; one fit at n = 7300, the size from which the fit builds its matrix in two launches.
The launchers of kbuild.hip a case reaches are named with the case."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "inference-tools_amd")]
import numpy as np
from inference_amd import _lib
from inference_amd._engine import SparseEngine
from inference_amd.gp import GpRegressor, Matern32, Matern52, RationalQuadratic, SquaredExponential

KINDS = {"se": (_lib.KERNEL_SE, SquaredExponential), "rq": (_lib.KERNEL_RQ, RationalQuadratic),
         "m32": (_lib.KERNEL_M32, Matern32), "m52": (_lib.KERNEL_M52, Matern52)}
res = {}


def record(name, arr):
    a = np.ascontiguousarray(np.asarray(arr, dtype=np.float64))
    res[name] = a
    print(f"{hashlib.sha256(a.tobytes()).hexdigest()}  {name} {a.shape}", flush=True)


def data(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, size=(n, d))
    y = np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(2.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y, rng.uniform(0.05, 0.15, size=n)


def cov_theta(kind, d):
    """[ln a, (ln kappa,) ln l_1 .. ln l_d] with unequal length scales"""
    scales = 0.4 * np.sqrt(d) * (1.0 + 0.1 * np.arange(d) / max(d - 1, 1))
    return [0.1] + ([0.3] if kind == "rq" else []) + list(np.log(scales))


def sparse_cases():
    print("# sparse model: every build in these cases is launch_kbuild_cross")
    for kind, (kid, _) in KINDS.items():
        for d in (1, 3, 17, 64):
            x, y, e = data(200, d, 100 + d)
            rng = np.random.default_rng(200 + d)
            z = x[rng.choice(200, size=70, replace=False)] + 0.01 * rng.standard_normal((70, d))
            q = rng.uniform(0.0, 1.0, size=(130, d))
            q[1], q[2] = x[100], z[35]  # (a data point and an inducing input among the queries)
            normals = rng.standard_normal((8, 130))
            theta = np.array(cov_theta(kind, d))
            for panel in (128, 0):
                tag = f"sgp {kind} d={d} panel={panel}"
                eng = SparseEngine(x, z)
                eng.set_targets(y - 0.2, e**2)
                F, g, alpha, info = eng.bound(kid, theta, 0.01, 1e-8, panel, True, True)
                record(f"{tag} bound F info", [F, info])
                record(f"{tag} bound grad", g)
                record(f"{tag} bound alpha", alpha)
                F, g, alpha, info, zg = eng.bound(kid, theta, 0.01, 1e-8, panel, True, True, want_zgrad=True)
                record(f"{tag} zgrad F info", [F, info])
                record(f"{tag} zgrad grad", g)
                record(f"{tag} zgrad alpha", alpha)
                record(f"{tag} zgrad dF/dZ", zg)
                record(f"{tag} fit F info", eng.fit(kid, theta, 0.01, 1e-8, panel))
                mean, var = eng.predict(q)
                record(f"{tag} predict mean", mean)
                record(f"{tag} predict var", var)
                mu, cov = eng.posterior(q)
                record(f"{tag} posterior mu", mu)
                record(f"{tag} posterior cov", cov)
                draws, mu, eps, info = eng.posterior_draws(q, n_draws=8, z=normals, jitter=1e-9)
                record(f"{tag} draws", np.zeros(1) if draws is None else draws)
                record(f"{tag} draws mu eps info", list(mu) + [eps, info])
                for M in (1, 130):
                    dm, dv = eng.spatial_derivatives(q[:M])
                    record(f"{tag} M={M} dmean", dm)
                    record(f"{tag} M={M} dvar", dv)
                    record(f"{tag} M={M} dmean alone", eng.spatial_derivatives(q[:M], want_var=False)[0])
                del eng


def fit_outputs(tag, gp, pts):
    record(f"{tag} alpha", gp.alpha)
    record(f"{tag} logdet", [gp._logdet])
    mu, sig = gp(pts)
    record(f"{tag} mu", mu)
    record(f"{tag} sig", sig)


def builder_cases():
    kernels = {k: (lambda c=c: c()) for k, (_, c) in KINDS.items()}
    kernels["se+m52"] = lambda: SquaredExponential() + Matern52()
    for n in (130, 300):
        for d in (1, 17):
            x, y, e = data(n, d, 300 + n + d)
            pts = np.random.default_rng(400 + d).uniform(0.0, 1.0, size=(130, d))
            for name, make in kernels.items():
                theta = np.array([float(y.mean())] + sum((cov_theta(k, d) for k in name.split("+")), []))
                gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=make())
                print(f"# fit + predict, {name}: launch_kbuild_square, launch_kbuild_cross")
                fit_outputs(f"gp {name} n={n} d={d}", gp, pts)
                if n == 300 and d == 17:
                    thetas = theta + 0.05 * np.random.default_rng(5).standard_normal((3, theta.size))
                    print(f"# lockstep LML batch, {name}: launch_kbuild_square_batched")
                    record(f"gp {name} lml batch", gp.marginal_likelihood_batch(thetas))
                    print(f"# lockstep predict batch, {name}: launch_kbuild_square_batched, launch_kbuild_cross_batched")
                    mean, std = gp.predict_marginalised(pts, thetas)
                    record(f"gp {name} predict batch mean", mean)
                    record(f"gp {name} predict batch std", std)
                    if name in ("m32", "m52"):
                        print(f"# Matern spatial derivatives, {name}: launch_kbuild_cross, launch_kbuild_cross_dprofile")
                        dm, dv = gp.spatial_derivatives_batch(pts)
                        record(f"gp {name} dmean", dm)
                        record(f"gp {name} dvar", dv)
                del gp
    # 57 tile rows: the factorisation opens in its look-ahead regime and the fit builds the matrix in two launches
    x, y, e = data(7300, 2, 77)
    theta = np.array([float(y.mean())] + cov_theta("se", 2))
    gp = GpRegressor(x, y, y_err=e, hyperpars=theta, kernel=SquaredExponential())
    print("# fit at n = 7300, se: launch_kbuild_square_part (both parts), launch_kbuild_cross")
    fit_outputs("gp se n=7300 d=2", gp, np.random.default_rng(9).uniform(0.0, 1.0, size=(130, 2)))


if __name__ == "__main__":
    out = sys.argv[1]
    sparse_cases()
    builder_cases()
    np.savez(out, **res)
