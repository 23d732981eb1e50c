"""
Host side of the kernel-level tests (tests/test_kernels_gpu.py, tests/test_kernel_host_cpu.py): seeded builders of
operands, the comparison helpers that name the 128 x 128 tiles in which a device result differs, and backward-error
ratios evaluated in extended precision.  NumPy only: no GPU and no library import, so everything here is also exercised
by the CPU suite.

Exact cases.  Small-integer operands make every product and every partial sum an integer far below 2^53: whatever the
summation order, tile shape or schedule, an fp64 kernel must then return the host result bit for bit.
  * GEMM: A, B in [-4, 4], C in [-2^20, 2^20], k <= 1152: |partial sums| <= 2^20 + 16 k < 2^21.
  * Cholesky: L0 has identity 128 x 128 diagonal blocks and integers from {-span .. span} in every block below them;
    A = L0 L0^T.  Every pivot a blocked factorisation with 128-wide (or narrower, aligned) blocks meets is exactly 1,
    every inverse diagonal block exactly I, every TRSM and trailing update integer arithmetic: the factor is L0.
  * K^-1: int_nilpotent_chol_case keeps the entries of L0 below the diagonal tiles to blocks between a few groups of
    tile rows, so that L0^-1 and K^-1 = L0^-T L0^-1 are small-integer matrices as well.

Bounded cases.  rho_* are componentwise backward-error ratios in units of u = 2^-53, with the residual accumulated in
np.longdouble (64-bit mantissa: its own rounding is 2^-11 u per operation and cannot reach the caps they are compared
with).  The denominators |L||L|^T ... are sums of non-negative terms and are formed in fp64 (relative error n u).
"""
import numpy as np

TILE = 128
U = 2.0 ** -53
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 2e-19)  # x87 extended or better; the bound tests skip without it
C_PAD = -12345.5      # sentinel of the padding columns of a C / matrix buffer (no exact result is a half-integer)
OPERAND_PAD = 2.0 ** 30  # padding of the A / B buffers: finite, and any use of it moves a result by >= 2^30


# ---------------------------------------------------------------------------------------------------------- builders
def int_gemm_case(m, n, k, ldc, lda, ldb, lower, seed):
    """Operands of C -= A B^T with exact integer arithmetic.  Returns a dict: the three full buffers as uploaded
    (`C0` m x ldc, `A` m x lda, `B` n x ldb, padding columns filled with sentinels), the shapes, and `E` (m x n), the
    exact result of the whole rectangle (with `lower` the device only produces its lower tiles: compare through
    gemm_mismatches)."""
    assert ldc >= n and lda >= k and ldb >= k and k <= 1152
    rng = np.random.default_rng(seed)
    C0 = np.full((m, ldc), C_PAD)
    C0[:, :n] = rng.integers(-2 ** 20, 2 ** 20 + 1, (m, n))
    A = np.full((m, lda), OPERAND_PAD)
    A[:, :k] = rng.integers(-4, 5, (m, k))
    B = np.full((n, ldb), OPERAND_PAD)
    B[:, :k] = rng.integers(-4, 5, (n, k))
    case = dict(m=m, n=n, k=k, ldc=ldc, lda=lda, ldb=ldb, lower=int(lower), C0=C0, A=A, B=B)
    case["E"] = gemm_expected(C0, A, B, n, k)
    return case


def gemm_expected(C0, A, B, n, k):
    """C - A B^T of the integer operands inside the buffers: exact in fp64 (every partial sum an integer < 2^21), so
    BLAS' summation order does not matter."""
    E = C0[:, :n] - A[:, :k] @ B[:n, :k].T
    assert np.abs(E).max() < 2.0 ** 22
    return E


def float_gemm_case(m, n, k, seed):
    """Full-mantissa normal operands whose magnitudes are spread over six decades per row (for rho_gemm)."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-3, 3, (m, 1))
    A = rng.standard_normal((m, k)) * 10.0 ** rng.uniform(-3, 3, (m, 1))
    B = rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return C, A, B


def int_chol_case(n, seed, span=1, f32=None):
    """(L0, A): L0 unit lower triangular with identity 128 x 128 diagonal blocks and integers from {-span .. span} in
    every block below them, A = L0 L0^T exactly.  Above n = 1024 the product is formed in float32 (an order of
    magnitude faster): it is exact there because every partial sum is an integer below 2^24.  `f32` forces the route."""
    rng = np.random.default_rng(seed)
    L0 = rng.integers(-span, span + 1, (n, n)).astype(np.float64)
    blk = np.arange(n) // TILE
    L0[blk[:, None] <= blk[None, :]] = 0.0
    L0[np.arange(n), np.arange(n)] = 1.0
    if (n > 1024) if f32 is None else f32:
        assert n * span * span + 1 < 2 ** 24  # bounds every partial sum of every entry
        L32 = L0.astype(np.float32)
        A = (L32 @ L32.T).astype(np.float64)
        assert np.abs(A).max() < 2 ** 24
    else:
        A = L0 @ L0.T
    return L0, A


def int_nilpotent_chol_case(groups, seed, n=None):
    """(L0, W, A) with W = L0^-1 a small-integer matrix: an integer factor whose INVERSE is exact too, for the paths that
    form L^-T and K^-1 = L^-T L^-1 (int_chol_case's inverse grows like 128^(nt - 1) and leaves 2^53 after a few tiles).
    The tile rows are cut into len(groups) consecutive groups of groups[i] 128-tiles; L0 = I + M with integers from
    {-1, 0, 1} in the blocks (group_i, group_j), i > j, and nothing else: M^g = 0 for g groups, so
    W = I - M + M^2 - ... +- M^(g-1), and A = L0 L0^T factors to L0 with every pivot 1 as for int_chol_case.
    n below 128 * sum(groups) returns the leading n x n parts (the leading part of a unit lower triangular matrix
    inverts to the leading part of its inverse; A is then the leading part of the full A).

    Sufficient condition for exactness, asserted here: with aW = I + |M| + ... + |M|^(g-1) >= |W|, |L0| entrywise, every
    intermediate of a blocked substitution on the identity is bounded entrywise by aW, a product with an inverse block
    sums at most 512 and K^-1 = W^T W at most n products of two such entries: n * aW.max()^2 < 2^53 covers the whole
    path, whatever the order of summation.  The matrix products below are formed in fp64 and are exact for the same
    reason (the partial sums of aW are non-negative integers below aW.max())."""
    full = TILE * int(sum(groups))
    n = full if n is None else n
    assert 0 < n <= full and len(groups) >= 1
    rng = np.random.default_rng(seed)
    M = rng.integers(-1, 2, (full, full)).astype(np.float64)
    grp = np.repeat(np.arange(len(groups)), np.asarray(groups) * TILE)
    M[grp[:, None] <= grp[None, :]] = 0.0
    M = M[:n, :n]
    I = np.eye(n)
    aM = np.abs(M)
    aW, W = I.copy(), I.copy()
    for _ in range(len(groups) - 1):  # Horner: I + |M| (I + |M| (...)),  I - M (I - M (...))
        aW = I + aM @ aW
        W = I - M @ W
    bound = n * float(aW.max()) ** 2
    assert bound < 2.0 ** 53, f"groups {tuple(groups)} at n = {n}: n aW.max()^2 = 2^{np.log2(bound):.1f} is not below 2^53"
    L0 = I + M
    A = L0 @ L0.T
    return L0, W, A


# (n, groups) of the exact K^-1 cases (seed NILPOTENT_SEED); 900 is the 1024 case cut to 900 rows; 768 has six tiles
# (nt % 4 == 2), the last outer block made of a tile of the second group and the third group's only tile
NILPOTENT_SEED = 1
NILPOTENT_CASES = [(384, (1, 1, 1)), (640, (1, 1, 1, 1, 1)), (768, (2, 3, 1)), (896, (2, 2, 2, 1)), (900, (3, 3, 2)),
                   (1024, (3, 3, 2)), (1536, (3, 3, 3, 3)), (2176, (5, 4, 4, 4))]
# (n, m) of the exact Z = Q K^-1 cases on int_chol_case(n): Z0 m x n from {-1, 0, 1}, Q = Z0 A
ROWS_KINV_CASES = [(384, 1), (640, 129), (768, 129), (896, 127), (1024, 513), (2176, 129), (2176, 1024), (2176, 1025),
                   (6656, 1024)]


def rows_kinv_case(A, m, seed):
    """(Z0, Q = Z0 A) for the exact backward row solve, with the condition that keeps every product with a 512 x 512
    inverse block (entries below 2^15, 512 terms) an exact integer sum asserted."""
    n = A.shape[0]
    Z0 = np.random.default_rng(seed).integers(-1, 2, (m, n)).astype(np.float64)
    Q = Z0 @ A  # exact: |A| <= n, every partial sum an integer below n^2
    assert 512 * np.abs(Q).max() * 2.0 ** 15 < 2.0 ** 53
    return Z0, Q


def spd_case(n, kind, seed):
    """A symmetric positive definite test matrix.  "well": B B^T + n I with B n x 64 (the matrix of
    tools/chain_trace.py); "graded": D A_well D with D = diag(10^linspace(0, -6, n)); "gp": a squared-exponential
    covariance on sorted 1-D points plus 1e-6 I."""
    rng = np.random.default_rng(seed)
    if kind in ("well", "graded"):
        B = rng.standard_normal((n, 64))
        A = B @ B.T + n * np.eye(n)
        if kind == "graded":
            d = 10.0 ** np.linspace(0.0, -6.0, n)
            A = d[:, None] * A * d[None, :]
    elif kind == "gp":
        x = np.sort(rng.uniform(0.0, 10.0, n))
        A = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2) + 1e-6 * np.eye(n)
    else:
        raise ValueError(kind)
    return 0.5 * (A + A.T)


def pad_identity(A, ld, fill=C_PAD):
    """blockdiag(A, I) at the next multiple of 128, in a buffer of pitch ld whose padding columns hold `fill`: the
    shape gpmi_dev_potrf takes (the library pads a ragged matrix the same way)."""
    n = A.shape[0]
    npad = -(-n // TILE) * TILE
    assert ld >= npad
    buf = np.full((npad, ld), fill)
    buf[:, :npad] = 0.0
    buf[:n, :n] = A
    buf[np.arange(n, npad), np.arange(n, npad)] = 1.0
    return buf


# ------------------------------------------------------------------- what a flag-ordered launch books as its FLOPs
FLOW_OUTER = 4  # tile columns per outer panel (csrc/potrf_flow.hip: OBT)
TILE_UPDATE_FLOPS = 2.0 * TILE ** 3  # one 128 x 128 tile taking one tile column


def flow_update_flops(m):
    """The FLOPs that potrf_flow_tail books under GPMI_PROF_FLOW for a tail of m tile rows (flow_build: flops_update), in
    closed form.  Tile (i, j), j <= i, takes the tile columns k < j, each of them once, as one-column tasks or inside a
    K = 512 chunk; the chain launch of column k itself updates tile (k + 1, k + 1), so a diagonal tile (i, i) is left
    with i - 1 columns; a diagonal tile keeps its lower triangle only and is booked at 3/4:
        sum_i [ i (i - 1) / 2 + 3/4 max(i - 1, 0) ]  tile updates of 2 * 128^3 FLOPs.
    Every term is a multiple of 2^19 far below 2^53: the sum is exact in fp64 whatever its order."""
    units = sum(i * (i - 1) / 2.0 + 0.75 * max(i - 1, 0) for i in range(m))
    return units * TILE_UPDATE_FLOPS


def flow_update_flops_of_lists(tasks):
    """The same from task lists as gpmi_flow_task_lists returns them (rows of 8 ints; column 0 the type: 0 panel TRSM,
    1 one-column update of a 64 x 64 sub-tile, 2 K = 512 chunk of a whole tile, 3 K = 512 chunk of a sub-tile): a
    sub-tile is a quarter of a tile, and a diagonal tile has three of them."""
    kind = np.asarray(tasks)[:, 0]
    units = 0.25 * np.count_nonzero(kind == 1) + FLOW_OUTER * np.count_nonzero(kind == 2) \
        + 0.25 * FLOW_OUTER * np.count_nonzero(kind == 3)
    return units * TILE_UPDATE_FLOPS


# ------------------------------------------------------------------------------------- comparisons that name tiles
def _bits_equal(a, b):
    return np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)


def _tile_report(bad, what, got=None, want=None, limit=12):
    """One line per 128 x 128 tile of the boolean mask `bad` that holds a True (at most `limit` lines)."""
    out = []
    rows, cols = bad.shape
    for ti in range(-(-rows // TILE)):
        for tj in range(-(-cols // TILE)):
            sub = bad[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE]
            if not sub.any():
                continue
            r, c = np.argwhere(sub)[0]
            quads = sorted({(int(a) // 64, int(b) // 64) for a, b in np.argwhere(sub)})
            line = (f"tile ({ti}, {tj}): {int(sub.sum())} entries {what}; 64 x 64 quarters {quads}; first at "
                    f"[{ti * TILE + r}, {tj * TILE + c}]")
            if got is not None:
                line += f" got {got[ti * TILE + r, tj * TILE + c]!r}"
            if want is not None:
                line += f" want {want[ti * TILE + r, tj * TILE + c]!r}"
            out.append(line)
    if len(out) > limit:
        out = out[:limit] + [f"... and {len(out) - limit} more tiles"]
    return out


def gemm_mismatches(got, case, E=None):
    """Compare the whole downloaded C buffer of gpmi_dev_gemm_nt with the exact result; returns a list of messages, one
    per offending tile (empty: correct).  Required: padding columns and, with `lower`, every strictly-upper 128-tile
    bit-identical to the upload; everything on or below the diagonal equal to E; above the diagonal inside a diagonal
    tile each element either the original or the exact updated value (include/gpmi.h does not say which: the 128 x 128
    kernels update the whole tile, the 64 x 64 kernels its two diagonal quarters)."""
    m, n, C0 = case["m"], case["n"], case["C0"]
    E = case["E"] if E is None else E
    msgs = []
    pad_bad = ~_bits_equal(got[:, n:], C0[:, n:])
    if pad_bad.any():
        r, c = np.argwhere(pad_bad)[0]
        msgs.append(f"padding: {int(pad_bad.sum())} entries changed, first at [{r}, {n + c}] (tile row {r // TILE})")
    G, O = got[:, :n], C0[:, :n]
    if not case["lower"]:
        return msgs + _tile_report(G != E, "differ from C - A B^T", G, E)
    ti = np.arange(m)[:, None] // TILE
    tj = np.arange(n)[None, :] // TILE
    on_or_below = np.arange(m)[:, None] >= np.arange(n)[None, :]
    upper_tile = tj > ti
    diag_upper = (tj == ti) & ~on_or_below
    msgs += _tile_report(on_or_below & (G != E), "differ from C - A B^T", G, E)
    msgs += _tile_report(upper_tile & ~_bits_equal(G, O), "of a strictly-upper tile changed", G, O)
    msgs += _tile_report(diag_upper & (G != E) & ~_bits_equal(G, O), "above the diagonal are neither original nor updated",
                         G, E)
    return msgs


def chol_mismatches(got, buf0, L0):
    """Compare the whole buffer after gpmi_dev_potrf with the exact factor L0 (n x n, n a multiple of 128; buf0 is
    the buffer as uploaded).  Required (include/gpmi.h): the lower triangle equals L0; padding columns, strictly-upper
    128-tiles and the part of tile (0, 0) above the diagonal are bit-identical to the upload; above the diagonal inside
    the other diagonal tiles - workspace of the trailing updates - every value is finite."""
    n = L0.shape[0]
    msgs = []
    pad_bad = ~_bits_equal(got[:, n:], buf0[:, n:])
    if pad_bad.any():
        r, c = np.argwhere(pad_bad)[0]
        msgs.append(f"padding: {int(pad_bad.sum())} entries changed, first at [{r}, {n + c}] (tile row {r // TILE})")
    G, O = got[:, :n], buf0[:, :n]
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    lower = i >= j
    upper_tile = (j // TILE) > (i // TILE)
    diag_upper = ((j // TILE) == (i // TILE)) & ~lower
    first_upper = diag_upper & (i < TILE)
    msgs += _tile_report(lower & (G != L0), "differ from L0", G, L0)
    msgs += _tile_report((upper_tile | first_upper) & ~_bits_equal(G, O), "above the factor changed", G, O)
    msgs += _tile_report(diag_upper & ~np.isfinite(G), "above the diagonal of a diagonal tile are not finite", G)
    return msgs


# -------------------------------------------------------------------------------------- extended-precision ratios
def check_rows(n, seed=0):
    """Rows on which the ratios are evaluated: all for n <= 640; beyond, every tile-boundary row (0, 127, 128, 129,
    ..., n - 1) and 32 seeded random ones - rows x n^2 longdouble operations instead of n^3."""
    if n <= 640:
        return np.arange(n)
    rows = {0, n - 1}
    for b in range(TILE, n, TILE):
        rows.update((b - 1, b, b + 1))
    rows.update(int(r) for r in np.random.default_rng(seed).integers(0, n, 32))
    return np.array(sorted(r for r in rows if 0 <= r < n))


def _ratio(num, den):
    """max num / den in units of u; 0 / 0 (a structural zero reproduced exactly) counts as 0, x / 0 as inf."""
    num = np.abs(np.asarray(num, dtype=np.longdouble))
    den = np.asarray(den, dtype=np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(num == 0, 0, np.where(den == 0, np.inf, num / den))
    return float(q.max() / U) if q.size else 0.0


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def rho_chol(A, L, rows=None):
    """max_ij |A - L L^T|_ij / (|L| |L|^T)_ij over the given rows (default check_rows), L lower triangular."""
    n = A.shape[0]
    rows = check_rows(n) if rows is None else rows
    L = np.tril(L)
    R = _ld(A[rows]) - _ld(L[rows]) @ _ld(L).T
    return _ratio(R, np.abs(L[rows]) @ np.abs(L).T)


def rho_solve_rows(X, L, Q, rows=None):
    """The same ratio for X L^T = Q: max |X L^T - Q| / (|X| |L^T|) over the given rows of X (default: all)."""
    rows = np.arange(X.shape[0]) if rows is None else rows
    L = np.tril(L)
    R = _ld(X[rows]) @ _ld(L).T - _ld(Q[rows])
    return _ratio(R, np.abs(X[rows]) @ np.abs(L).T)


def rho_solve(A, alpha, r):
    """The same ratio for A alpha = r: max_i |A alpha - r|_i / (|A| |alpha|)_i."""
    R = _ld(A) @ _ld(alpha) - _ld(r)
    return _ratio(R, np.abs(A) @ np.abs(alpha))


def rho_gemm(Chat, C, A, B, rows=None):
    """max |Chat - (C - A B^T)| / (|C| + |A| |B|^T) over the given rows (default: all)."""
    rows = np.arange(C.shape[0]) if rows is None else rows
    R = _ld(Chat[rows]) - (_ld(C[rows]) - _ld(A[rows]) @ _ld(B).T)
    return _ratio(R, np.abs(C[rows]) + np.abs(A[rows]) @ np.abs(B).T)


def inverse_residual(A, iK, rows=None):
    """max |A iK - I| over the given rows (default check_rows), as a plain number (not in units of u)."""
    n = A.shape[0]
    rows = check_rows(n) if rows is None else rows
    R = _ld(A[rows]) @ _ld(iK)
    R[np.arange(len(rows)), rows] -= 1
    return float(np.abs(R).max())


def loo_vectors(alpha, ikdiag):
    """(c1, c2) of the leave-one-out gradient in longdouble: var = 1 / diag(K^-1), c1 = alpha var,
    c2 = var (1 + var alpha^2) / 2."""
    var = 1 / _ld(ikdiag)
    a = _ld(alpha)
    return a * var, var * (1 + var * a * a) / 2


def rho_loo_p(p, iK, alpha, ikdiag):
    """max_i |p - K^-1 c1|_i / (|K^-1| |c1|)_i for an exactly known K^-1 (integer data)."""
    c1, _ = loo_vectors(alpha, ikdiag)
    R = _ld(p) - _ld(iK) @ c1
    return _ratio(R, np.abs(iK) @ np.abs(c1.astype(np.float64)))


def rho_loo_w(Wm, iK, alpha, ikdiag, rows=None):
    """max |W - K^-1 diag(c2) K^-1| / (|K^-1| diag(c2) |K^-1|) over the given rows (default check_rows), K^-1 exact."""
    n = iK.shape[0]
    rows = check_rows(n) if rows is None else rows
    _, c2 = loo_vectors(alpha, ikdiag)
    R = _ld(Wm[rows]) - (_ld(iK[rows]) * c2) @ _ld(iK).T
    return _ratio(R, (np.abs(iK[rows]) * c2.astype(np.float64)) @ np.abs(iK).T)


def kappa_blocks(L, b):
    """The largest 2-norm condition number of the b x b diagonal blocks of the factor L (the last one may be smaller):
    what a multiplication by an explicitly inverted diagonal block can cost in backward error."""
    n = L.shape[0]
    return max(float(np.linalg.cond(np.tril(L[s:min(s + b, n), s:min(s + b, n)]), 2)) for s in range(0, n, b))


# --------------------------------------------------------------------------- plain NumPy references (CPU test, table)
def substitute_rows(L, Q):
    """X with X L^T = Q by plain forward substitution, one column at a time."""
    n = L.shape[0]
    X = np.zeros_like(Q)
    for j in range(n):
        X[:, j] = (Q[:, j] - X[:, :j] @ L[j, :j]) / L[j, j]
    return X


def substitute_back_rows(L, Q):
    """X with X L = Q by plain backward substitution, one column at a time."""
    n = L.shape[0]
    X = np.zeros_like(Q)
    for j in range(n - 1, -1, -1):
        X[:, j] = (Q[:, j] - X[:, j + 1:] @ L[j + 1:, j]) / L[j, j]
    return X


def solve_spd(L, r):
    """alpha = L^-T L^-1 r by the two substitutions."""
    v = substitute_rows(L, r[None, :])
    return substitute_back_rows(L, v)[0]


def inverse_spd(L):
    """K^-1 = L^-T L^-1 from W = L^-1 (rows of the identity through the forward substitution)."""
    W = substitute_rows(L, np.eye(L.shape[0])).T  # X L^T = I  ->  X = L^-T, W = X^T = L^-1
    return W.T @ W


# the caps of the bounded tests, in units of u (residuals in longdouble); kappa = 0 for a plain reference
def cap_chol(n, k128=0.0):
    return (n + 1) * (1 + k128)


def cap_solve_rows(n, k512=0.0):
    return (n + 1) * (1 + k512)


def cap_alpha(n, k128=0.0):
    return 3 * (n + 1) * (1 + k128) ** 2


def cap_loo_p(n):
    """p = K^-1 c1 with K^-1 exact: an n-term dot product in any order of summation (each term one product and at most
    n - 1 additions, or FMAs: n roundings) of c1 = alpha * (1 / d), two roundings: (1 + delta)^(n + 2), gamma_(n+2) <
    (n + 3) u for n u << 1; one more unit for the rounding of p's own reference."""
    return n + 4


def cap_loo_w(n):
    """W = G G^T, G = K^-1 diag(s), s = sqrt(c2).  c2 as computed: var = 1 / d (1 rounding, used twice), var alpha alpha
    (2 more), 1 + . (1; the terms are positive, the sum's relative error is no larger than the term's), the product with
    var / 2 (1; the halving is exact): at most 6 relative roundings under the square root, which halves them, plus its
    own: s within (1 + delta)^4 of sqrt(c2).  G_ij = K^-1_ij s_j: 5.  A term G_ij G_kj of the n-term dot product carries
    10 and collects n more in any order of summation: gamma_(n+10) < (n + 11) u; one more unit as for p."""
    return n + 12


def cap_inverse(n, cond_a, k128=0.0):
    """bound on max |A iK - I| itself (already multiplied by u)"""
    return (n + 1) * (1 + k128) ** 2 * cond_a * U
