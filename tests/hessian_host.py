"""
NumPy mirror of the exact Hessian of the log-marginal likelihood (gpmi_lml_hessian), written from the formulas with dense
derivative matrices - none of the device's tiling, profiles-by-halves or summation orders:

    LML = -1/2 r^T alpha - sum ln L_ii,   r = y - Phi^T m,   alpha = K^-1 r,   Q = alpha alpha^T - K^-1
    H_ij        = 1/2 sum Q o D_ij  -  (D_i alpha)^T K^-1 (D_j alpha)  +  1/2 tr(K^-1 D_i K^-1 D_j)       (T1, T2, T3)
    H_{m_p m_q} = -phi_p^T K^-1 phi_q,        H_{m_p theta_j} = -phi_p^T K^-1 D_j alpha
    K = a^2 (C(u) + 1e-12 I) + diag(noise) + sigma^2 I,   q_k = dx_k^2 / l_k^2,   u = sum_k q_k,   s = u / 2
    dK/d ln l_k = a^2 g q_k,   d2K/d ln l_k d ln l_m = a^2 (g2 q_k q_m - 2 delta_km g q_k)
    dK/d ln a = 2 a^2 (C + 1e-12 I),   d2K/d ln a^2 = twice that,   d2K/d ln a d theta_j = 2 dK/d theta_j
    se:  g = g2 = C = e^-s        m52: t = sqrt(5 u), g = 5/3 (1 + t) e^-t, g2 = 25/3 e^-t
    m32: t = sqrt(3 u), g = 3 e^-t, g2 = 9 e^-t / t (the product g2 q_k q_m is 0 at coincident points)
    rq:  F = 1 + s / kappa, C = F^-kappa, A = kappa ln F - s / F, rho = ln kappa:
         g = C / F, g2 = C (1 + 1 / kappa) / F^2, dK/d rho = -K A, d2K/d rho^2 = K (A^2 - A + s^2 / (kappa F^2)),
         d2K/d rho d ln l_k = a^2 C q_k (F - 1 - A F) / F^2
    WhiteNoise: dK/d ln sigma = 2 sigma^2 I, second derivative 4 sigma^2 I, no mixed terms.

Parameter order of every result: the mean's parameters, the kernel's ([ln a, (ln kappa,) ln l_1 .. ln l_d]), then ln sigma if
there is a WhiteNoise term.  `dtype=numpy.longdouble` runs the whole evaluation in long double (the inverse: the float64
inverse refined by Newton-Schulz steps in long double).
"""
import numpy as np

JITTER = 1e-12


_BITS = 21


def _slices(A, axis):
    """A = scale * sum_p c_p 2^(-21 p) along rows (axis 1) or columns (axis 0): four float64 slices of 21-bit integers over
    2^21, scale a power of two per row / column.  Every step is exact in long double."""
    m = np.abs(A).max(axis=axis, keepdims=True).astype(np.float64)
    m[m == 0.0] = 1.0
    scale = np.ldexp(np.longdouble(1.0), (np.floor(np.log2(m)) + 1).astype(np.int64))
    R = A / scale
    out = []
    for _ in range(4):
        c = np.rint(np.ldexp(R, _BITS))
        out.append(np.ldexp(c, -_BITS).astype(np.float64))
        R = np.ldexp(R, _BITS) - c
    return out, scale


def matmul(A, B):
    """A @ B.  Long double operands: by error-free slicing - products of 21-bit slices summed over n <= 2048 terms are
    exact in float64 whatever the order, so the float64 BLAS does the work (NumPy's own long-double product runs 640^3 in
    seconds) - the ten slice pairs down to 2^-84 of (row maximum x column maximum), added in long double."""
    if A.dtype != np.longdouble:
        return A @ B
    assert A.shape[1] <= 2048
    a, sa = _slices(A, 1)
    b, sb = _slices(B, 0)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=np.longdouble)
    for order in range(3, -1, -1):  # smallest contributions first
        part = np.zeros_like(out)
        for p in range(order + 1):
            part += (a[p] @ b[order - p]).astype(np.longdouble)
        out += np.ldexp(part, -_BITS * order)
    return out * sa * sb


def _inverse(K, dtype):
    X = np.linalg.inv(np.asarray(K, dtype=np.float64))
    if dtype is np.float64:
        return 0.5 * (X + X.T)
    X = X.astype(dtype)
    eye = np.eye(len(K), dtype=dtype)
    for _ in range(2):  # quadratic: (1e-16 cond)^2 after the first step already
        X = X + matmul(X, eye - matmul(K, X))
    return 0.5 * (X + X.T)


def _profiles(kind, s, kappa, dtype):
    """C, g, g2 and, for rq, (A, F); g2 of m32 is returned as 0 at s = 0."""
    if kind == "se":
        C = np.exp(-s)
        return C, C, C, None
    if kind == "m32":
        t = np.sqrt(6 * s)
        e = np.exp(-t)
        g2 = np.zeros_like(t)
        pos = t > 0
        g2[pos] = 9 * e[pos] / t[pos]
        return (1 + t) * e, 3 * e, g2, None
    if kind == "m52":
        t = np.sqrt(10 * s)
        e = np.exp(-t)
        return (1 + t + t * t / 3) * e, dtype(5) / 3 * (1 + t) * e, dtype(25) / 3 * e, None
    if kind == "rq":
        F = 1 + s / kappa
        lnF = np.log1p(s / kappa)
        C = np.exp(-kappa * lnF)
        return C, C / F, C * (1 + 1 / kappa) / F**2, (kappa * lnF - s / F, F)
    raise ValueError(kind)


def hessian(kind, x, y, noise_var, theta_mean, phi, theta_kernel, ln_sigma=None, dtype=np.float64, ripple=None):
    """The LML, its gradient, its Hessian H and the three terms of H (T1 + T2 + T3 = H; the mean's blocks are in T2) with
    `scale` = |T1| + |T2| + |T3|, as a dict.  phi: (n_mean, n) rows d mu / d m_p; ripple: an (n, n) symmetric array r, K is
    replaced by K o (1 + r) before it is inverted (the derivative matrices stay): the yardstick's own sensitivity."""
    dtype = np.longdouble if dtype is np.longdouble else np.float64
    x = np.asarray(x, dtype=dtype)
    n, d = x.shape
    phi = np.asarray(phi, dtype=dtype).reshape(-1, n)
    n_mean = len(phi)
    th = np.asarray(theta_kernel, dtype=dtype)
    shape = 1 if kind == "rq" else 0
    a2 = np.exp(2 * th[0])
    kappa = np.exp(th[1]) if shape else None
    scales = np.exp(th[1 + shape:])
    q = np.array([((x[:, None, k] - x[None, :, k]) / scales[k]) ** 2 for k in range(d)])
    s = q.sum(axis=0) / 2
    C, g, g2, rq = _profiles(kind, s, kappa, dtype)
    eye = np.eye(n, dtype=dtype)
    Ka = a2 * (C + dtype(JITTER) * eye)
    sig2 = np.exp(2 * dtype(ln_sigma)) if ln_sigma is not None else dtype(0)
    K = Ka + np.diag(np.asarray(noise_var, dtype=dtype)) + sig2 * eye
    Kinv_of = K * (1 + np.asarray(ripple, dtype=dtype)) if ripple is not None else K
    iK = _inverse(Kinv_of, dtype)
    r = np.asarray(y, dtype=dtype) - np.asarray(theta_mean, dtype=dtype) @ phi
    alpha = iK @ r
    Q = np.outer(alpha, alpha) - iK

    # first derivatives, in the kernel's order
    D = [2 * Ka]
    if shape:
        D.append(-Ka * rq[0])
    D.extend(a2 * g * q[k] for k in range(d))
    if ln_sigma is not None:
        D.append(2 * sig2 * eye)
    nk = 1 + shape + d  # the kernel's parameters
    PT = len(D)

    def second(i, j):  # i <= j
        if ln_sigma is not None and j == nk:
            return 4 * sig2 * eye if i == nk else None
        if i == 0:
            return 2 * D[j]
        if shape and i == 1:
            A, F = rq
            if j == 1:
                return Ka * (A * A - A + s * s / (kappa * F * F))
            return a2 * C * q[j - 2] * (F - 1 - A * F) / (F * F)
        k, m = i - 1 - shape, j - 1 - shape
        out = a2 * g2 * q[k] * q[m]
        return out - 2 * D[i] if k == m else out

    W = [Di @ alpha for Di in D]
    G = [matmul(iK, Di) for Di in D]
    Z = [Gi @ alpha for Gi in G]
    P = n_mean + PT
    T1, T2, T3 = (np.zeros((P, P), dtype=dtype) for _ in range(3))
    for i in range(PT):
        for j in range(i, PT):
            Dij = second(i, j)
            t1 = (Q * Dij).sum() / 2 if Dij is not None else dtype(0)
            t2 = -(W[i] @ Z[j])
            t3 = (G[i] * G[j].T).sum() / 2
            for a, b in ((i, j), (j, i)):
                T1[n_mean + a, n_mean + b] = t1
                T2[n_mean + a, n_mean + b] = t2
                T3[n_mean + a, n_mean + b] = t3
    iKphi = phi @ iK
    T2[:n_mean, :n_mean] = -(iKphi @ phi.T)
    T2[:n_mean, :n_mean] = (T2[:n_mean, :n_mean] + T2[:n_mean, :n_mean].T) / 2
    for j in range(PT):
        T2[:n_mean, n_mean + j] = -(phi @ Z[j])
        T2[n_mean + j, :n_mean] = T2[:n_mean, n_mean + j]
    grad = np.concatenate([phi @ alpha, [(Q * Di).sum() / 2 for Di in D]])
    L = np.linalg.cholesky(np.asarray(K, dtype=np.float64))
    lml = float(-0.5 * (r @ alpha)) - float(np.log(np.diag(L)).sum())
    return dict(lml=lml, grad=grad, H=T1 + T2 + T3, T1=T1, T2=T2, T3=T3, scale=np.abs(T1) + np.abs(T2) + np.abs(T3),
                n_mean=n_mean, alpha=alpha)


def ripple_spread(kind, x, y, noise_var, theta_mean, phi, theta_kernel, ln_sigma=None, count=48, size=1e-13, seed=0):
    """The largest movement, per entry, of the float64 mirror's own H under `count` symmetric relative ripples of `size`
    on its K: (P, P).  Computed without the code under test."""
    args = (kind, x, y, noise_var, theta_mean, phi, theta_kernel, ln_sigma)
    base = hessian(*args)["H"]
    rng = np.random.default_rng(seed)
    n = len(y)
    spread = np.zeros_like(base)
    for _ in range(count):
        r = rng.uniform(-1.0, 1.0, (n, n))
        r = np.triu(r) + np.triu(r, 1).T
        spread = np.maximum(spread, np.abs(hessian(*args, ripple=size * r)["H"] - base))
    return spread
