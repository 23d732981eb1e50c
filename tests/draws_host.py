"""
NumPy mirror of the posterior-draw entry points (include/gpmi.h: gpmi_posterior_draws, gpmi_mvn_draws,
gpmi_draws_normals), written from the header's description, not from the library's code:

  * `philox4x32_10`  the Random123 generator, vectorised over counters;
  * `normals`        the library's stream of standard normals: element (s, j) from (seed, s, j) alone;
  * `draws_oracle`   mu + z chol(sym(Sigma) + eps I)^T with eps = jitter_rel * max diag(Sigma).

`NORMAL_ULPS` bounds the difference of two implementations of the stream in units of 2^-53 r, r = sqrt(-2 ln u1) the
radius of the pair: |dz| <= 32 . 2^-53 . r.  Four sources: the argument fl(2 pi) u2 of sine and cosine, with an absolute
error of at most 2 . 2 pi . 2^-53; sine and cosine themselves, at most 4 ulp; the logarithm, at most 3 ulp; a correctly
rounded square root.  Together about 24 . 2^-53 . r on either side.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")  # fl(2 pi)
NORMAL_ULPS = 32.0


def philox4x32_10(counter, key):
    """counter: (..., 4) and key: (..., 2) arrays of 32-bit words (broadcast against each other); returns (..., 4) uint64
    words below 2^32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SHIFT32) ^ c1 ^ k0, p1 & MASK32, (p0 >> SHIFT32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def uniforms(seed, first_draw, n, m):
    """(u1 in (0, 1], u2 in [0, 1)), each (n, ceil(m / 2)): pair p of draw first_draw + s."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    pairs = (m + 1) // 2
    s = (int(first_draw) + np.arange(n, dtype=object)) & 0xFFFFFFFFFFFFFFFF  # Python integers: no wrap below 2^64
    s_lo = np.array([int(v) & 0xFFFFFFFF for v in s], dtype=np.uint64)[:, None]
    s_hi = np.array([int(v) >> 32 for v in s], dtype=np.uint64)[:, None]
    p = np.arange(pairs, dtype=np.uint64)[None, :]
    counter = np.stack(np.broadcast_arrays(p, s_lo, s_hi, np.uint64(0)), axis=-1)
    r = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    n1 = ((r[..., 0] >> np.uint64(5)) << np.uint64(26)) + (r[..., 1] >> np.uint64(6)) + np.uint64(1)
    n2 = ((r[..., 2] >> np.uint64(5)) << np.uint64(26)) + (r[..., 3] >> np.uint64(6))
    return n1.astype(np.float64) * 2.0**-53, n2.astype(np.float64) * 2.0**-53  # both conversions exact (<= 2^53)


def normals(seed, first_draw, n, m, with_radius=False):
    """Rows first_draw .. first_draw + n - 1 of the stream of `seed`, (n, m); with_radius: also r per element."""
    u1, u2 = uniforms(seed, first_draw, n, m)
    r = np.sqrt(-2.0 * np.log(u1))
    a = TWO_PI * u2
    z = np.empty((n, 2 * u1.shape[1]))
    z[:, 0::2] = r * np.cos(a)
    z[:, 1::2] = r * np.sin(a)
    if with_radius:
        return z[:, :m], np.repeat(r, 2, axis=1)[:, :m]
    return z[:, :m]


def sym(Sigma):
    """The symmetric matrix whose lower triangle is Sigma's (what the library reads)."""
    lower = np.tril(np.asarray(Sigma, dtype=float))
    return lower + np.tril(lower, -1).T


def draws_oracle(mu, Sigma, jitter_rel, z):
    S = sym(Sigma)
    eps = jitter_rel * np.diagonal(S).max()
    L = np.linalg.cholesky(S + eps * np.eye(S.shape[0]))
    return np.asarray(mu, dtype=float)[None, :] + np.asarray(z, dtype=float) @ L.T


def posterior_covariance_longdouble(K, Kq, Kqq):
    """K_qq - Q^T Q, Q = L^-1 K_qx^T, L L^T = K, from the given float64 matrices in numpy.longdouble arithmetic throughout,
    rounded once at the end: what the posterior covariance of the regression oracles would be without their own rounding."""
    ld = np.longdouble
    K, B, n = np.asarray(K, dtype=ld), np.array(np.asarray(Kq).T, dtype=ld), len(K)
    L = np.zeros_like(K)
    for j in range(n):  # column Cholesky
        v = K[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    Q = np.zeros_like(B)
    for i in range(n):  # forward substitution, all right-hand sides at once
        Q[i] = (B[i] - L[i, :i] @ Q[:i]) / L[i, i]
    return np.asarray(np.asarray(Kqq, dtype=ld) - Q.T @ Q, dtype=np.float64)


def moment_statistics(z):
    """The four standardised statistics of a block of would-be standard normals (each ~ N(0, 1) under the hypothesis):
    mean sqrt(n), (var - 1) sqrt(n / 2), (m4 - 3) sqrt(n / 96), corr(even, odd columns) sqrt(n / 2)."""
    v = np.asarray(z, dtype=float).ravel()
    n = v.size
    even, odd = z[:, 0::2].ravel(), z[:, 1::2].ravel()
    k = min(even.size, odd.size)
    return np.array([v.mean() * np.sqrt(n), ((v**2).mean() - 1.0) * np.sqrt(n / 2.0), ((v**4).mean() - 3.0) * np.sqrt(n / 96.0),
                     (even[:k] * odd[:k]).mean() * np.sqrt(n / 2.0)])
