"""
NumPy / SciPy oracle of the Matern32 / Matern52 device kernels (the reference has no Matern, so there are no golden
values to compare with).  Everything here is written from the formulas, not from the package's code:

    s = 1/2 sum_k dx_k^2 / l_k^2,   u_k^2 = dx_k^2 / l_k^2,   theta = [ln a, ln l_1 .. ln l_d],   K = a^2 C(s)
    Matern32:  t = sqrt(6 s),   C = (1 + t) e^-t,             g = 3 e^-t
    Matern52:  t = sqrt(10 s),  C = (1 + t + t^2 / 3) e^-t,   g = 5/3 (1 + t) e^-t
    dK/d ln a = 2 K,   dK/d ln l_k = a^2 g u_k^2,   dK(q, x_n)/dq_k = a^2 g (x_n - q)_k / l_k^2,
    prior variance of the derivative along axis k: g(0) a^2 / l_k^2;   diagonal of a build: a^2 (C + 1e-12)

`HostKernel` is a plugin `CovarianceFunction` on these formulas (also for SquaredExponential and RationalQuadratic, the
partners in sums): `GpRegressor(kernel=HostKernel("m52"))` takes the package's generic route (host-built matrices, the
device's dense entry points) - a second, independent way to every quantity.  `OracleGp` is the first: the whole
regression in NumPy / SciPy on the host.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from inference_amd.gp.covariance import CovarianceFunction

JITTER = 1e-12
G0 = {"m32": 3.0, "m52": 5.0 / 3.0, "se": 1.0}


def n_shape(kind):
    return 1 if kind == "rq" else 0


def _u2(u, v, scales):
    """(d, n_u, n_v): ((u_k - v_k) / l_k)^2"""
    return np.array([((u[:, None, k] - v[None, :, k]) / scales[k]) ** 2 for k in range(u.shape[1])])


def profiles(kind, s, kappa=None):
    """(C, g) with dK/d ln l_k = a^2 g u_k^2, at s = 1/2 sum_k u_k^2."""
    if kind == "m32":
        t = np.sqrt(6.0 * s)
        return (1.0 + t) * np.exp(-t), 3.0 * np.exp(-t)
    if kind == "m52":
        t = np.sqrt(10.0 * s)
        return (1.0 + t + t * t / 3.0) * np.exp(-t), (5.0 / 3.0) * (1.0 + t) * np.exp(-t)
    if kind == "se":
        return np.exp(-s), np.exp(-s)
    if kind == "rq":
        F = 1.0 + s / kappa
        return F ** -kappa, F ** (-kappa - 1.0)
    raise ValueError(kind)


def split(kind, theta):
    theta = np.asarray(theta, dtype=float)
    a2 = np.exp(2.0 * theta[0])
    kappa = np.exp(theta[1]) if kind == "rq" else None
    return a2, kappa, np.exp(theta[1 + n_shape(kind):])


def cross(kind, u, v, theta):
    a2, kappa, scales = split(kind, theta)
    return a2 * profiles(kind, 0.5 * _u2(u, v, scales).sum(axis=0), kappa)[0]


def build(kind, x, theta):
    K = cross(kind, x, x, theta)
    K[np.diag_indices_from(K)] += split(kind, theta)[0] * JITTER
    return K


def build_and_grads(kind, x, theta):
    a2, kappa, scales = split(kind, theta)
    u2 = _u2(x, x, scales)
    s = 0.5 * u2.sum(axis=0)
    C, g = profiles(kind, s, kappa)
    K = a2 * (C + JITTER * np.eye(len(x)))
    grads = [2.0 * K]
    if kind == "rq":  # d/d ln kappa of a^2 (1 + s / kappa)^-kappa
        F = 1.0 + s / kappa
        grads.append(-K * (kappa * np.log(F) - s / F))
    grads.extend(a2 * g * u2k for u2k in u2)
    return K, grads


def gradient_terms(kind, q, x, theta):
    """(A (d, N), R (d,)): A_kn K(q, x_n) = dK(q, x_n)/dq_k, R_k = g(0) a^2 / l_k^2."""
    a2, kappa, scales = split(kind, theta)
    diff = x - q[None, :]
    C, g = profiles(kind, 0.5 * ((diff / scales) ** 2).sum(axis=1), kappa)
    return (diff / scales**2 * (g / C)[:, None]).T, G0[kind] * a2 / scales**2


class HostKernel(CovarianceFunction):
    """One stationary kernel ("m32", "m52", "se", "rq") as a plugin: every matrix in NumPy on the host."""

    def __init__(self, kind):
        self.kind = kind
        self.bounds = None

    def pass_spatial_data(self, x):
        self.x = np.asarray(x, dtype=float)
        self.n_params = self.x.shape[1] + 1 + n_shape(self.kind)
        self.hyperpar_labels = [f"host {self.kind} {i}" for i in range(self.n_params)]

    def estimate_hyperpar_bounds(self, y):
        self.bounds = [(-5.0, 5.0)] * self.n_params

    def __call__(self, u, v, theta):
        return cross(self.kind, np.asarray(u, float), np.asarray(v, float), theta)

    def build_covariance(self, theta):
        return build(self.kind, self.x, theta)

    def covariance_and_gradients(self, theta):
        return build_and_grads(self.kind, self.x, theta)

    def gradient_terms(self, v, x, theta):
        if self.kind == "rq":
            return super().gradient_terms(v, x, theta)
        return gradient_terms(self.kind, np.asarray(v, float), x, theta)


class HostModel:
    """A covariance model of the oracle: `parts` is a list of
         ("m32" | "m52" | "se" | "rq",)   a stationary kernel
         ("wn",)                          WhiteNoise, theta = [ln sigma]
         ("het",)                         HeteroscedasticNoise, theta = [ln sigma_1 .. ln sigma_N]
         ("cp", (kind0, kind1), axis)     a two-region ChangePoint, theta = [theta_0, theta_1, location, width]
       summed, the parameters back to back in that order."""

    def __init__(self, parts, x):
        self.parts, self.x = parts, np.asarray(x, dtype=float)
        n, d = self.x.shape
        self.counts = []
        for p in parts:
            if p[0] == "wn":
                self.counts.append(1)
            elif p[0] == "het":
                self.counts.append(n)
            elif p[0] == "cp":
                self.counts.append(sum(d + 1 + n_shape(k) for k in p[1]) + 2)
            else:
                self.counts.append(d + 1 + n_shape(p[0]))
        self.n_params = sum(self.counts)
        edges = np.concatenate([[0], np.cumsum(self.counts)])
        self.slices = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]

    def _cp(self, p, theta):
        d = self.x.shape[1]
        n0 = d + 1 + n_shape(p[1][0])
        n1 = d + 1 + n_shape(p[1][1])
        return theta[:n0], theta[n0:n0 + n1], theta[n0 + n1], theta[n0 + n1 + 1]

    @staticmethod
    def _window(xa, c, w):
        return 1.0 / (1.0 + np.exp(-(xa - c) / w))

    def cross(self, u, v, theta):
        out = np.zeros((len(u), len(v)))
        for p, sl in zip(self.parts, self.slices):
            th = theta[sl]
            if p[0] in ("wn", "het"):
                continue
            if p[0] == "cp":
                t0, t1, c, w = self._cp(p, th)
                fu, fv = self._window(u[:, p[2]], c, w), self._window(v[:, p[2]], c, w)
                out += np.outer(1 - fu, 1 - fv) * cross(p[1][0], u, v, t0) + np.outer(fu, fv) * cross(p[1][1], u, v, t1)
            else:
                out += cross(p[0], u, v, th)
        return out

    def prior_var(self, q, theta):
        """K(q, q) without jitter or noise, per row of q."""
        return np.array([self.cross(r[None, :], r[None, :], theta)[0, 0] for r in q])

    def build_and_grads(self, theta, grads=True):
        n = len(self.x)
        K, out = np.zeros((n, n)), []
        for p, sl in zip(self.parts, self.slices):
            th = theta[sl]
            if p[0] == "wn":
                Kp = np.exp(2.0 * th[0]) * np.eye(n)
                gp = [2.0 * Kp]
            elif p[0] == "het":
                Kp = np.diag(np.exp(2.0 * th))
                gp = []
                for i in range(n if grads else 0):
                    G = np.zeros((n, n))
                    G[i, i] = 2.0 * np.exp(2.0 * th[i])
                    gp.append(G)
            elif p[0] == "cp":
                t0, t1, c, w = self._cp(p, th)
                xa = self.x[:, p[2]]
                f = self._window(xa, c, w)
                K0, g0 = build_and_grads(p[1][0], self.x, t0)
                K1, g1 = build_and_grads(p[1][1], self.x, t1)
                W0, W1 = np.outer(1 - f, 1 - f), np.outer(f, f)
                Kp = W0 * K0 + W1 * K1
                gp = [W0 * G for G in g0] + [W1 * G for G in g1]
                z = (xa - c) / w
                for df in (-f * (1 - f) / w, -f * (1 - f) * z / w):  # d f / d location, d f / d width
                    A = -np.outer(df, 1 - f)
                    B = np.outer(df, f)
                    gp.append(K0 * (A + A.T) + K1 * (B + B.T))
            else:
                Kp, gp = build_and_grads(p[0], self.x, th)
            K += Kp
            out.extend(gp)
        return K, out


class LinearMeanHost:
    """A prior mean for `OracleGp`: mu(q) = m_0 + sum_k m_{1+k} (q_k - <x_k>), centred on the training points x.  Called
    with (points, m) it returns (mu at the points, the rows d mu / d m_p there (1 + d, M))."""

    def __init__(self, x):
        self.centre = np.asarray(x, float).mean(axis=0)
        self.n_params = 1 + len(self.centre)

    def __call__(self, points, m):
        rows = np.vstack([np.ones(len(points)), (np.asarray(points, float) - self.centre[None, :]).T])
        return np.asarray(m, float) @ rows, rows


class OracleGp:
    """GP regression on the host, theta = [the mean's parameters, covariance parameters].  The prior mean is a constant
    (one parameter) unless `mean` is given: a callable (points, m) -> (mu at the points, rows d mu / d m_p (n_mean, M)) with
    an attribute `n_params` (`LinearMeanHost`).  `y_err`: standard deviations (N,), or a dense data covariance (N, N)."""

    def __init__(self, x, y, y_err, model, theta, mean=None):
        self.x, self.y = np.asarray(x, float), np.asarray(y, float)
        y_err = np.asarray(y_err, float)
        self.sig = y_err if y_err.ndim == 2 else np.diag(y_err ** 2)
        self.m = model
        self.n = len(self.y)
        self.mean = mean
        self.nm = 1 if mean is None else mean.n_params
        self.theta = np.asarray(theta, float)
        self.K = self.m.build_and_grads(self.theta[self.nm:], grads=False)[0] + self.sig
        self.L = cholesky(self.K, lower=True)
        self.alpha = self._solve(self.L, self.y - self._mu(self.x, self.theta))

    @staticmethod
    def _solve(L, b):
        return solve_triangular(L.T, solve_triangular(L, b, lower=True), lower=False)

    def _mu(self, pts, theta):
        """The prior mean at `pts`: the scalar theta[0] for the constant mean, a vector otherwise."""
        return theta[0] if self.mean is None else self.mean(pts, theta[:self.nm])[0]

    def _mean_rows(self):
        """d mu / d m_p at the training points, (n_mean, N)."""
        return np.ones((1, self.n)) if self.mean is None else self.mean(self.x, self.theta[:self.nm])[1]

    def __call__(self, q):
        Kq = self.m.cross(q, self.x, self.theta[self.nm:])
        v = solve_triangular(self.L, Kq.T, lower=True)
        var = self.m.prior_var(q, self.theta[self.nm:]) - (v**2).sum(axis=0)
        return Kq @ self.alpha + self._mu(q, self.theta), np.sqrt(np.abs(var))

    def build_posterior(self, q):
        Kq = self.m.cross(q, self.x, self.theta[self.nm:])
        Q = solve_triangular(self.L, Kq.T, lower=True)
        return Kq @ self.alpha + self._mu(q, self.theta), self.m.cross(q, q, self.theta[self.nm:]) - Q.T @ Q

    def _factor(self, theta, grads):
        K, dK = self.m.build_and_grads(theta[self.nm:], grads=grads)
        L = cholesky(K + self.sig, lower=True)
        iL = solve_triangular(L, np.eye(self.n), lower=True)
        iK = iL.T @ iL
        return L, iK, iK @ (self.y - self._mu(self.x, theta)), dK

    def marginal_likelihood(self, theta):
        theta = np.asarray(theta, float)
        L, _, alpha, _ = self._factor(theta, False)
        return -0.5 * (self.y - self._mu(self.x, theta)) @ alpha - np.log(np.diag(L)).sum()

    def marginal_likelihood_gradient(self, theta):
        theta = np.asarray(theta, float)
        L, iK, alpha, dK = self._factor(theta, True)
        Q = np.outer(alpha, alpha) - iK
        g_mean = [alpha.sum()] if self.mean is None else list(self._mean_rows() @ alpha)
        grad = np.concatenate([g_mean, [0.5 * (Q * G).sum() for G in dK]])
        return -0.5 * (self.y - self._mu(self.x, theta)) @ alpha - np.log(np.diag(L)).sum(), grad

    def loo_likelihood(self, theta):
        theta = np.asarray(theta, float)
        _, iK, alpha, _ = self._factor(theta, False)
        var = 1.0 / np.diag(iK)
        return -0.5 * (var * alpha**2 + np.log(var)).sum()

    def loo_likelihood_gradient(self, theta):
        theta = np.asarray(theta, float)
        _, iK, alpha, dK = self._factor(theta, True)
        var = 1.0 / np.diag(iK)
        c1, c2 = alpha * var, 0.5 * var * (1.0 + var * alpha**2)
        grad = [(c1 * (iK @ row)).sum() for row in self._mean_rows()]
        for G in dK:
            Z = iK @ G
            grad.append((c1 * (Z @ alpha) - c2 * np.diag(Z @ iK)).sum())
        return -0.5 * (var * alpha**2 + np.log(var)).sum(), np.array(grad)

    # the reference's algorithms for the predictive gradients (one point at a time), with this oracle's gradient_terms
    def gradient(self, q, kind):
        mus, covs = [], []
        for r in q:
            k = cross(kind, r[None, :], self.x, self.theta[self.nm:])[0]
            A, R = gradient_terms(kind, r, self.x, self.theta[self.nm:])
            Q = solve_triangular(self.L, (A * k[None, :]).T, lower=True)
            mus.append(A @ (k * self.alpha))
            covs.append(R - Q.T @ Q)
        return np.array(mus), np.array(covs)

    def spatial_derivatives(self, q, kind):
        dmu, dvar = [], []
        for r in q:
            k = cross(kind, r[None, :], self.x, self.theta[self.nm:])[0]
            A, _ = gradient_terms(kind, r, self.x, self.theta[self.nm:])
            dmu.append(A @ (k * self.alpha))
            dvar.append(-2.0 * (A * k[None, :]) @ self._solve(self.L, k))
        return np.array(dmu), np.array(dvar)


def dataset(n, d, seed=0, far=True):
    """x uniform in [0, 4]^d with row 1 a copy of row 0 and (far) the last row 10^3 away; y smooth plus noise;
    y_err = 0.1."""
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    x = rng.uniform(0.0, 4.0, size=(n, d))
    x[1] = x[0]
    if far:
        x[-1] = x[-1] + 1e3
    y = np.sin(x[:, 0]) + 0.3 * np.cos(1.7 * x.sum(axis=1) % 7.0) + 0.1 * rng.standard_normal(n)
    return x, y, np.full(n, 0.1)


def theta_for(kind, d, seed=0):
    """[ln a, (ln kappa,) ln l_k]: a = e^0.2, l in [0.7, 2]."""
    rng = np.random.default_rng(77 + seed + d)
    th = [0.2] + ([0.4] if kind == "rq" else []) + list(np.log(rng.uniform(0.7, 2.0, size=d)))
    return np.array(th)
