"""NumPy mirror of the generalised GP (inference_amd/gp/generalised.py, csrc/api_generalised.hip): the latent covariance
builders with their a^2 1e-12 jitter, Newton's iteration of Laplace's method with exactly the device's stopping rule and
step halving, log q, its gradient by the hyper-parameters, and the latent predictions.  Test infrastructure only."""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

SE, RQ, M32, M52 = 0, 1, 3, 4


def theta_offset(kernel):
    return 2 if kernel == RQ else 1


def _half_sq(u, v, theta, kernel):
    """(z, per-dimension dx^2 / l^2) with z = 1/2 sum_k dx_k^2 / l_k^2"""
    l = np.exp(np.asarray(theta, dtype=float)[theta_offset(kernel):])
    q = ((u[:, None, :] - v[None, :, :]) / l[None, None, :]) ** 2
    return 0.5 * q.sum(axis=2), q


def _profile(kernel, z, theta):
    """(C, G): K = a^2 C off the diagonal and dK / d ln l_k = a^2 G dx_k^2 / l_k^2"""
    if kernel == SE:
        C = np.exp(-z)
        return C, C
    if kernel == RQ:
        kappa = np.exp(theta[1])
        F = 1.0 + z / kappa
        C = np.exp(-kappa * np.log(F))
        return C, C / F
    two_nu = 3.0 if kernel == M32 else 5.0
    t = np.sqrt(2.0 * two_nu * z)
    e = np.exp(-t)
    if kernel == M32:
        return (1.0 + t) * e, 3.0 * e
    return (1.0 + t + t * t / 3.0) * e, (5.0 / 3.0) * (1.0 + t) * e


def cross_covariance(kernel, u, v, theta):
    z, _ = _half_sq(u, v, theta, kernel)
    return np.exp(2.0 * theta[0]) * _profile(kernel, z, theta)[0]


def covariance(kernel, x, theta):
    """latent K: a^2 (C + 1e-12 I)"""
    K = cross_covariance(kernel, x, x, theta)
    K[np.diag_indices_from(K)] = np.exp(2.0 * theta[0]) * (1.0 + 1e-12)
    return K


def covariance_gradients(kernel, x, theta):
    """dK / d theta_j in the kernel's layout (the jitter follows ln a)"""
    theta = np.asarray(theta, dtype=float)
    a2 = np.exp(2.0 * theta[0])
    z, q = _half_sq(x, x, theta, kernel)
    C, G = _profile(kernel, z, theta)
    K = a2 * C
    K[np.diag_indices_from(K)] = a2 * (1.0 + 1e-12)
    grads = [2.0 * K]
    if kernel == RQ:
        kappa = np.exp(theta[1])
        F = 1.0 + z / kappa
        Koff = a2 * C
        grads.append(-Koff * (kappa * np.log(F) - z / F))
    for k in range(x.shape[1]):
        grads.append(a2 * G * q[:, :, k])
    return grads


def psi_of(lik, y, aux, offset, a, fm):
    return -0.5 * (a @ fm) + lik.log_prob(y, fm + offset, aux).sum()


def laplace(lik, x, y, aux, offset, kernel, theta, tol=1e-9, max_iter=50, K=None):
    """Newton's iteration from a = 0.  Returns a dict: info (0 / k > 0 / -1), iterations, halvings, logq, psi, f, g, W, sw,
    d3, L (of B at the final f), K."""
    theta = np.asarray(theta, dtype=float)
    if K is None:
        K = covariance(kernel, x, theta)
    n = len(y)
    a, fm = np.zeros(n), np.zeros(n)
    psi = psi_of(lik, y, aux, offset, a, fm)
    out = dict(info=0, iterations=0, halvings=0, logq=-1e50, K=K)
    if not np.isfinite(psi):
        out["info"] = -1
        return out

    def factor(sw):
        B = np.eye(n) + sw[:, None] * K * sw[None, :]
        if not np.all(np.isfinite(B)):
            return None
        try:
            return cholesky(B, lower=True)
        except np.linalg.LinAlgError:
            return None

    converged = False
    for it in range(1, max_iter + 1):
        g, W, _ = lik.derivatives(y, fm + offset, aux)
        sw = np.sqrt(W)
        L = factor(sw)
        out["iterations"] = it
        if L is None:
            out["info"] = 1
            return out
        b = W * fm + g
        a_new = b - sw * cho_solve((L, True), sw * (K @ b))
        fm_new = K @ a_new
        psi_new = psi_of(lik, y, aux, offset, a_new, fm_new)
        step, h = 1.0, 0
        a_acc, fm_acc = a_new, fm_new
        while not (psi_new >= psi - 1e-12 * abs(psi)) and h < 10:
            h += 1
            step *= 0.5
            a_acc = a + step * (a_new - a)
            fm_acc = fm + step * (fm_new - fm)
            psi_new = psi_of(lik, y, aux, offset, a_acc, fm_acc)
        out["halvings"] += h
        if not np.isfinite(psi_new):
            out["info"] = -1
            return out
        dmax = np.abs(fm_acc - fm).max()
        a, fm, psi = a_acc, fm_acc, psi_new
        if dmax <= tol * (1.0 + np.abs(fm + offset).max()):
            converged = True
            break
    out["psi"] = psi
    if not converged:
        out["info"] = -1
        return out
    g, W, d3 = lik.derivatives(y, fm + offset, aux)
    sw = np.sqrt(W)
    L = factor(sw)
    if L is None:
        out["info"] = 1
        return out
    out.update(logq=psi - np.log(np.diag(L)).sum(), f=fm + offset, a=a, g=g, W=W, sw=sw, d3=d3, L=L)
    return out


def gradient(res, kernel, x, theta):
    """d log q / d theta from a converged `laplace` result: the contraction with (u, v, iK) = (g + 2 w, g, R)"""
    K, L, sw, g, d3 = res["K"], res["L"], res["sw"], res["g"], res["d3"]
    n = len(g)
    Binv = cho_solve((L, True), np.eye(n))
    R = sw[:, None] * Binv * sw[None, :]
    post = np.diag(K) - np.einsum("ia,ab,bi->i", K, R, K)
    s2 = 0.5 * post * d3
    w = s2 - R @ (K @ s2)
    u = g + 2.0 * w
    Q = 0.5 * (np.outer(u, g) + np.outer(g, u)) - R
    return np.array([0.5 * (Q * dK).sum() for dK in covariance_gradients(kernel, x, theta)])


def predict(res, kernel, x, theta, offset, pts):
    """latent mean m + k(q)^T g and variance a^2 - |L^-1 (sw o k(q))|^2 (K_qq without jitter, as the device)"""
    kq = cross_covariance(kernel, pts, x, np.asarray(theta, dtype=float))
    mean = offset + kq @ res["g"]
    v = solve_triangular(res["L"], (kq * res["sw"][None, :]).T, lower=True)
    return mean, np.exp(2.0 * theta[0]) - (v * v).sum(axis=0)


# ---- the cases of tests/test_generalised_gpu.py (inputs and mirror results live in tests/golden/generalised.npz) ----
def rippler(seed, rel=1e-13):
    """Multiplies every entry by 1 + rel xi, xi uniform in [-1, 1]; symmetric for a square matrix."""
    rng = np.random.default_rng(seed)

    def ripple(A):
        xi = rng.uniform(-1.0, 1.0, size=A.shape)
        if A.ndim == 2 and A.shape[0] == A.shape[1]:
            xi = np.triu(xi) + np.triu(xi, 1).T
        return A * (1.0 + rel * xi)

    return ripple


def _smooth(x):
    return np.sin(3.0 * x[:, 0]) + 0.5 * np.cos(2.0 * x.sum(axis=1))


# name -> (likelihood, kernel, N, d, M, seed)
CASES = {
    "poisson_se": ("Poisson", SE, 130, 3, 50, 11),        # one row past a 128-row tile
    "logistic_m52": ("Logistic", M52, 300, 2, 257, 5),    # three 8 sigma outliers: step halving
    "binomial_rq": ("Binomial", RQ, 257, 17, 1, 3),       # the 64 KiB LDS builders
    "poisson_m32": ("Poisson", M32, 640, 1, 129, 7),      # y = 0 rows, exposures 1 .. 50; a second 512-wide inverse block
}
# the case of tests/test_pair_regime_gpu.py: np = 5248 >= 5120, so the handle's first lane owns the CU-masked stream pair
# and every factorisation of B is one flag-ordered launch of 41 tile rows.  Its inputs are regenerated from the seed;
# tests/golden/generalised_pair.npz holds the mirror's logq, f, g, mean and var with their allowances (no gradient: the
# mirror's N^3 einsum per hyper-parameter is not worth it at this size)
PAIR_CASES = {
    "poisson_se_pair": ("Poisson", SE, 5130, 2, 300, 13),
}


def make_case(name):
    """Seeded inputs of a case: dict(lik_name, kernel, x, y, aux_arg, theta, theta2, pts)."""
    lik_name, kernel, n, d, m, seed = CASES[name] if name in CASES else PAIR_CASES[name]
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, size=(n, d))
    pts = rng.uniform(0.0, 1.0, size=(m, d))
    f = _smooth(x)
    if name in ("poisson_se", "poisson_se_pair"):
        aux = np.ones(n)
        y = rng.poisson(np.exp(1.0 + f)).astype(float)
        amp, scale = 0.0, np.log(0.5)
    elif name == "logistic_m52":
        aux = np.full(n, 0.1)
        y = f + aux * (np.sqrt(3.0) / np.pi) * rng.logistic(size=n)
        y[[17, 150, 288]] += np.array([8.0, -8.0, 8.0]) * 0.1
        amp, scale = 0.0, np.log(0.4)
    elif name == "binomial_rq":
        aux = np.full(n, 3.0)
        y = rng.binomial(3, 1.0 / (1.0 + np.exp(-2.0 * f))).astype(float)
        amp, scale = np.log(1.5), np.log(2.0)
    else:
        aux = np.round(rng.uniform(1.0, 50.0, size=n))
        y = rng.poisson(aux * np.exp(f - 2.0)).astype(float)
        assert (y == 0).sum() >= 5
        amp, scale = 0.0, np.log(0.3)
    theta = np.concatenate([[amp], [0.3] if kernel == RQ else [], np.full(d, scale)])
    return dict(lik_name=lik_name, kernel=kernel, x=x, y=y, aux_arg=aux, theta=theta, theta2=theta + 0.15, pts=pts)


def mirror_quantities(lik, aux, offset, c, ripple=None, want_grad=True):
    """The quantities the device is compared in, from the mirror: dict(logq, grad, f, g, mean, var) and the Newton log.
    `ripple`: applied to the mirror's K and to its cross-covariances.  `want_grad` False leaves `grad` out."""
    K = covariance(c["kernel"], c["x"], c["theta"])
    if ripple is not None:
        K = ripple(K)
    res = laplace(lik, c["x"], c["y"], aux, offset, c["kernel"], c["theta"], K=K)
    assert res["info"] == 0, res["info"]
    grad = gradient(res, c["kernel"], c["x"], c["theta"]) if want_grad else None
    kq = cross_covariance(c["kernel"], c["pts"], c["x"], c["theta"])
    if ripple is not None:
        kq = ripple(kq)
    mean = offset + kq @ res["g"]
    v = solve_triangular(res["L"], (kq * res["sw"][None, :]).T, lower=True)
    var = np.exp(2.0 * c["theta"][0]) - (v * v).sum(axis=0)
    q = dict(logq=np.array(res["logq"]), grad=grad, f=res["f"], g=res["g"], mean=mean, var=var)
    if not want_grad:
        del q["grad"]
    return q, (res["iterations"], res["halvings"])
