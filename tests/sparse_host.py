"""
NumPy / SciPy mirror of the variational inducing-point model (Titsias 2009) behind `SparseGpRegressor` and the
gpmi_sgp_* entry points: the bound F, its analytic gradient and the prediction, all in the stable "B form".  The kernels
come from tests/matern_host.py (formulas, not the package's code).

    sigma_i^2 = noise_var_i + s^2,  W = diag(1 / sigma_i^2),  eps = jitter a^2
    K_mm + eps I = L L^T,  G = K_mn W K_nm,  H = L^-1 G L^-T (symmetrised),  B = I + H = L_B L_B^T,  c = L_B^-1 L^-1 K_mn W r
    F = -1/2 [N ln 2 pi + sum ln sigma_i^2 + 2 sum ln diag(L_B) + r^T W r - c^T c] - 1/2 [a^2 sum w_i - tr H]
    mean(q) = u^T c,  var(q) = a^2 - |v|^2 + |u|^2,  v = L^-1 k_m(q),  u = L_B^-1 v

    S = L^-T B^-1 L^-1,  gamma = S K_mn W r,  alpha = W (r - K_nm gamma),  beta = L^-T L^-1 K_mn alpha,
    T = L^-T (I - B^-1) L^-1,  M1 = beta alpha^T + T K_mn W,  M2 = beta beta^T + L^-T (B - 2 I + B^-1) L^-1
    dF/dtheta_k = sum M1 o dK_mn/dtheta_k - 1/2 sum M2 o d(K_mm + eps I)/dtheta_k - 1/2 sum_i w_i da^2/dtheta_k
    dF/d ln s   = s^2 sum_i [alpha_i^2 - (R^-1)_ii + w_i^2 (a^2 - Q_ii)],  (R^-1)_ii = w_i - w_i^2 k_i^T S k_i,  Q_ii = |L^-1 k_i|^2

`ripple`: a callable (name, matrix) -> matrix applied to K_mm ("mm"), K_mn ("mn") and a query's K_mq ("mq") before
anything is computed from them - the tests perturb the entries by the K-build's accuracy class to size their tolerances.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import matern_host as mh

LN_2PI = float(np.log(2.0 * np.pi))


def cross_and_grads(kind, u, v, theta):
    """K(u, v) and its derivatives by theta = [ln a, (ln kappa,) ln l_1 .. ln l_d] (no diagonal term)."""
    a2, kappa, scales = mh.split(kind, theta)
    u2 = mh._u2(u, v, scales)
    s = 0.5 * u2.sum(axis=0)
    C, g = mh.profiles(kind, s, kappa)
    K = a2 * C
    grads = [2.0 * K]
    if kind == "rq":
        F = 1.0 + s / kappa
        grads.append(-K * (kappa * np.log(F) - s / F))
    grads.extend(a2 * g * u2k for u2k in u2)
    return K, grads


class SparseMirror:
    def __init__(self, kind, x, z, jitter=1e-8, ripple=None):
        self.kind, self.x, self.z, self.jitter = kind, np.asarray(x, float), np.asarray(z, float), float(jitter)
        self.ripple = ripple or (lambda name, A: A)
        self._key, self._kernels = None, None

    def _kernel_matrices(self, theta, grads=False):
        """Unrippled K_mm, K_mn and (grads) their derivatives at theta, kept for the last theta: rippled repeats are cheap."""
        key = np.asarray(theta, float).tobytes()
        if key != self._key or (grads and self._kernels[2] is None):
            if grads:
                Kmm, dmm = cross_and_grads(self.kind, self.z, self.z, theta)
                Kmn, dmn = cross_and_grads(self.kind, self.z, self.x, theta)
            else:
                Kmm, Kmn, dmm, dmn = mh.cross(self.kind, self.z, self.z, theta), mh.cross(self.kind, self.z, self.x, theta), None, None
            self._key, self._kernels = key, (Kmm, Kmn, dmm, dmn)
        return self._kernels

    def _matrices(self, theta):
        a2 = mh.split(self.kind, theta)[0]
        K0mm, K0mn, _, _ = self._kernel_matrices(theta)
        Kmm, Kmn = self.ripple("mm", K0mm), self.ripple("mn", K0mn)
        return a2, Kmm + self.jitter * a2 * np.eye(len(self.z)), Kmn

    def state(self, theta, white_var, r, noise_var):
        """Everything the bound, the prediction and the gradient share.  Raises numpy.linalg.LinAlgError if K_mm + eps I
        or B is not positive definite."""
        r = np.asarray(r, float)
        sig2 = (np.zeros(len(r)) if noise_var is None else np.asarray(noise_var, float)) + white_var
        w = 1.0 / sig2
        a2, Kmm, Kmn = self._matrices(theta)
        L = cholesky(Kmm, lower=True)
        G = (Kmn * w) @ Kmn.T
        H = solve_triangular(L, solve_triangular(L, G, lower=True).T, lower=True)
        H = 0.5 * (H + H.T)
        B = np.eye(len(H)) + H
        LB = cholesky(B, lower=True)
        b = Kmn @ (w * r)
        c = solve_triangular(LB, solve_triangular(L, b, lower=True), lower=True)
        F = (-0.5 * (len(r) * LN_2PI + np.log(sig2).sum() + 2.0 * np.log(np.diag(LB)).sum() + r @ (w * r) - c @ c)
             - 0.5 * (a2 * w.sum() - np.trace(H)))
        return dict(r=r, w=w, a2=a2, Kmm=Kmm, Kmn=Kmn, L=L, G=G, H=H, B=B, LB=LB, b=b, c=c, F=float(F))

    def bound(self, theta, white_var, r, noise_var=None):
        return self.state(theta, white_var, r, noise_var)["F"]

    def cond_kmm(self, theta):
        return float(np.linalg.cond(self._matrices(theta)[1]))

    def predict(self, theta, white_var, r, noise_var, q, st=None):
        st = st or self.state(theta, white_var, r, noise_var)
        Kmq = self.ripple("mq", mh.cross(self.kind, self.z, np.asarray(q, float), theta))
        v = solve_triangular(st["L"], Kmq, lower=True)
        u = solve_triangular(st["LB"], v, lower=True)
        return u.T @ st["c"], st["a2"] - (v**2).sum(axis=0) + (u**2).sum(axis=0)

    def bound_and_gradient(self, theta, white_var, r, noise_var=None, st=None):
        """(F, gradient by [theta, ln s], alpha): the last entry is 0 for white_var = 0.  st: the `state` of the same
        arguments, if the caller has it already."""
        st = st or self.state(theta, white_var, r, noise_var)
        r, w, a2, L, LB, Kmn, H, B = (st[k] for k in ("r", "w", "a2", "L", "LB", "Kmn", "H", "B"))
        m = len(L)
        Linv = solve_triangular(L, np.eye(m), lower=True)
        Binv = solve_triangular(LB, solve_triangular(LB, np.eye(m), lower=True), lower=True, trans="T")
        Binv = 0.5 * (Binv + Binv.T)
        S = Linv.T @ Binv @ Linv
        gamma = S @ st["b"]
        alpha = w * (r - Kmn.T @ gamma)
        beta = Linv.T @ (Linv @ (Kmn @ alpha))
        T = Linv.T @ (np.eye(m) - Binv) @ Linv
        M1 = np.outer(beta, alpha) + (T @ Kmn) * w
        M2 = np.outer(beta, beta) + Linv.T @ (B - 2.0 * np.eye(m) + Binv) @ Linv
        _, _, dmm, dmn = self._kernel_matrices(theta, grads=True)
        grad = np.zeros(len(theta) + 1)
        for k in range(len(theta)):
            dKmm = dmm[k] + (2.0 * self.jitter * a2 * np.eye(m) if k == 0 else 0.0)  # d eps / d ln a = 2 eps
            grad[k] = (M1 * dmn[k]).sum() - 0.5 * (M2 * dKmm).sum() - (a2 * w.sum() if k == 0 else 0.0)
        if white_var > 0.0:
            kSk = ((S @ Kmn) * Kmn).sum(axis=0)
            Qii = (solve_triangular(L, Kmn, lower=True) ** 2).sum(axis=0)
            grad[-1] = white_var * (alpha**2 - (w - w**2 * kSk) + w**2 * (a2 - Qii)).sum()
        return st["F"], grad, alpha

    def dense_bound(self, theta, white_var, r, noise_var=None):
        """The definition: ln N(r | 0, Q + Sigma) - 1/2 tr(W (a^2 I - Q)), Q = K_nm (K_mm + eps I)^-1 K_mn, through the
        N x N matrix (the form that loses digits when K_mm is ill conditioned; for well-conditioned checks only)."""
        r = np.asarray(r, float)
        sig2 = (np.zeros(len(r)) if noise_var is None else np.asarray(noise_var, float)) + white_var
        a2, Kmm, Kmn = self._matrices(theta)
        Q = Kmn.T @ np.linalg.solve(Kmm, Kmn)
        C = cholesky(Q + np.diag(sig2), lower=True)
        v = solve_triangular(C, r, lower=True)
        return float(-0.5 * (len(r) * LN_2PI + 2.0 * np.log(np.diag(C)).sum() + v @ v) - 0.5 * ((a2 - np.diag(Q)) / sig2).sum())


def fd4(f, theta, h=1e-3):
    """Fourth-order central difference of a scalar function, coordinate by coordinate."""
    theta = np.asarray(theta, float)
    out = np.zeros(len(theta))
    for k in range(len(theta)):
        e = np.zeros(len(theta))
        e[k] = h
        out[k] = (-f(theta + 2 * e) + 8.0 * f(theta + e) - 8.0 * f(theta - e) + f(theta - 2 * e)) / (12.0 * h)
    return out


def rippler(seed, rel=1e-13):
    """A `ripple` that multiplies every entry by 1 + rel xi, xi uniform in [-1, 1] (symmetric for K_mm)."""
    rng = np.random.default_rng(seed)

    def ripple(name, A):
        xi = rng.uniform(-1.0, 1.0, size=A.shape)
        if name == "mm":
            xi = np.triu(xi) + np.triu(xi, 1).T
        return A * (1.0 + rel * xi)

    return ripple


def dataset(n, d, seed=0):
    """x uniform in the unit cube, a smooth y plus noise of 0.1, y_err between 0.05 and 0.15."""
    rng = np.random.default_rng(5000 + 17 * n + d + seed)
    x = rng.uniform(0.0, 1.0, size=(n, d))
    y = np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(2.0 * x.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    return x, y, rng.uniform(0.05, 0.15, size=n)


def spread_rows(x, m):
    """m rows of x, far apart: farthest-point selection from row 0, sorted (well-conditioned inducing inputs)."""
    idx = [0]
    dmin = ((x - x[0]) ** 2).sum(axis=1)
    for _ in range(m - 1):
        i = int(np.argmax(dmin))
        idx.append(i)
        dmin = np.minimum(dmin, ((x - x[i]) ** 2).sum(axis=1))
    return np.sort(np.array(idx))


# ---- the five cases of the device tests (test_sparse_gpu.py, test_sparse_z_gpu.py, test_sparse_post_gpu.py) ----------

N_RIPPLES = 48
MU = 0.2  # the constant mean of every case


def case(number):
    if number == 1:
        kind, n, d, m, panel, white, use_err, ell = "se", 300, 3, 33, 128, 0.02, True, 0.35
    elif number == 2:
        kind, n, d, m, panel, white, use_err, ell = "m52", 2100, 2, 130, 512, 0.0, True, 0.2
    elif number == 3:
        kind, n, d, m, panel, white, use_err, ell = "rq", 257, 17, 64, 0, 0.01, False, 1.5
    elif number == 4:
        kind, n, d, m, panel, white, use_err, ell = "m32", 200, 64, 1, 0, 0.0, True, 3.0
    else:
        kind, n, d, m, panel, white, use_err, ell = "se", 70, 1, 129, 0, 0.0, True, 0.005
    x, y, e = dataset(n, d, seed=number)
    z = np.linspace(0.0, 1.0, m).reshape(-1, 1) if number == 5 else x[spread_rows(x, m)].copy()
    scales = ell * (1.0 + 0.1 * np.arange(d) / max(d - 1, 1))  # (unequal length scales: every dimension has its own gradient)
    theta = np.array([0.1] + ([0.3] if kind == "rq" else []) + list(np.log(scales)))
    q = np.random.default_rng(40 + number).uniform(0.0, 1.0, size=(17, d))  # (the query points of test_sparse_gpu.py)
    return dict(number=number, kind=kind, x=x, y=y, e=e if use_err else None, z=z, theta=theta, white=white, panel=panel, q=q)


# ---- the cases at the shapes where the device's schedules change (test_sparse_scale_*.py, golden/sparse_scale.npz) ----
# name: (kind, N, d, m, panel_rows, WhiteNoise variance, length scale); every case has y_err
SCALE_CASES = {
    "tiles3": ("se", 700, 2, 300, 256, 0.02, 0.05),
    "run4": ("m32", 32700, 1, 200, 32768, 0.0, 0.006),
    "run8": ("m52", 32700, 1, 450, 32768, 0.0, 0.003),
    "run16": ("m32", 32700, 1, 1000, 32768, 0.0, 0.0012),
    "long": ("se", 262444, 1, 5, 0, 0.01, 0.3),
    "max_m": ("m52", 300, 3, 4096, 0, 0.0, 0.04),
    "bench_like": ("se", 16385, 8, 512, 0, 0.01, 0.8),
}
SCALE_NAMES = tuple(SCALE_CASES)
# what gpmi_sgp_schedule must report for a case (inference_amd._engine.sgp_schedule), and a neighbouring smaller shape
# (n, m, panel_rows) -> the fields that must differ there: the case is on the branch it is named after, the neighbour is not
SCALE_SCHEDULE = {
    "tiles3": (dict(panel=256, m_pad=384, panels=3), (700, 256, 256), dict(m_pad=256)),
    "run4": (dict(panel=32768, m_pad=256, data_run_tiles=4, panels=1), (32700, 200, 16384), dict(data_run_tiles=2)),
    "run8": (dict(panel=32768, m_pad=512, data_run_tiles=8, panels=1), (32700, 450, 16384), dict(data_run_tiles=4)),
    "run16": (dict(panel=32768, m_pad=1024, data_run_tiles=16, panels=1), (32700, 1000, 16384), dict(data_run_tiles=8)),
    "long": (dict(panel=8192, m_pad=128, weight_blocks=1024, panels=33), (262144, 5, 0), dict(weight_blocks=1024, panels=32)),
    "max_m": (dict(m_pad=4096, kmm_run_tiles=8, panels=1), (300, 3968, 0), dict(kmm_run_tiles=4)),
    "bench_like": (dict(panel=8192, m_pad=512, panels=3), (16384, 512, 0), dict(panels=2)),
}
SELECT_N, SELECT_M, SELECT_EXTRA = 66000, 24, 700  # the selection at 258 workgroups (261 with the appended rows)


def scale_case(name):
    """The case `name` of SCALE_CASES, in the layout of `case`: the same data set, mean and unequal length scales, Z
    `spread_rows` of x except for max_m (the 16 x 16 x 16 cell centres of the unit cube, jittered) and bench_like (512
    random rows, sorted: the benchmark's choice)."""
    kind, n, d, m, panel, white, ell = SCALE_CASES[name]
    number = 11 + SCALE_NAMES.index(name)
    x, y, e = dataset(n, d, seed=number)
    if name == "max_m":
        c = (np.arange(16) + 0.5) / 16.0
        z = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
        z = z + np.random.default_rng(3).uniform(-0.01, 0.01, size=z.shape)
    elif name == "bench_like":
        z = x[np.sort(np.random.default_rng(number).choice(n, m, replace=False))].copy()
    else:
        z = x[spread_rows(x, m)].copy()
    scales = ell * (1.0 + 0.1 * np.arange(d) / max(d - 1, 1))
    theta = np.array([0.1] + list(np.log(scales)))
    q = np.random.default_rng(40 + number).uniform(0.0, 1.0, size=(17, d))
    return dict(number=number, name=name, kind=kind, x=x, y=y, e=e, z=np.ascontiguousarray(z), theta=theta, white=white,
                panel=panel, q=q)


def select_case():
    """The selection at n = 66000: (x, theta of Matern52 with l = (0.2, 0.22), weights 1 / y_err^2)."""
    x, _, e = dataset(SELECT_N, 2, seed=21)
    return x, np.array([0.0, np.log(0.2), np.log(0.22)]), 1.0 / e**2


def later_tile_rows(rows, run_tiles):
    """Mask over `rows` points summed in 64-row tiles, `run_tiles` tiles per workgroup: the rows in the third and later
    tiles of their run."""
    return (np.arange(rows) // 64) % run_tiles >= 2


def full_theta(case):
    th = [MU] + list(case["theta"])
    if case["white"] > 0.0:
        th.append(0.5 * np.log(case["white"]))
    return np.array(th)


def make_gp(case, panel_rows=None, jitter=1e-8, z=None):
    from inference_amd.gp import Matern32, Matern52, RationalQuadratic, SparseGpRegressor, SquaredExponential, WhiteNoise

    kern = {"se": SquaredExponential, "m52": Matern52, "m32": Matern32, "rq": RationalQuadratic}[case["kind"]]()
    if case["white"] > 0.0:
        kern = kern + WhiteNoise()
    return SparseGpRegressor(case["x"], case["y"], y_err=case["e"], inducing_points=case["z"] if z is None else z,
                             kernel=kern, hyperpars=full_theta(case), jitter=jitter,
                             panel_rows=case["panel"] if panel_rows is None else panel_rows)


def check(label, got, want, allow):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print(f"{label}: device error {err:.3e}, allowance {allow:.3e}")
    assert err <= allow, (label, err, allow)
