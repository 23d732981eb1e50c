"""
Kernel-level tests of the fp64 hot path: gpmi_dev_gemm_nt (gemm_f64.hip), gpmi_dev_potrf (potrf.hip, potrf_flow.hip,
potrf_diag.h), `info`, the sweeps and many-right-hand-side solves behind the dense entry points (solve.hip), and K^-1,
the leave-one-out pieces and the backward row solve (parts F and G).

Sharpness comes from integer data (tests/kernel_host.py): every operation is then exact, so the device must return the
host result bit for bit whatever the summation order, tile shape or schedule, and a failure names the 128 x 128 tiles
that differ.  Real-valued matrices are held to componentwise backward-error caps whose residuals are evaluated in
np.longdouble; tests/test_kernel_host_cpu.py shows that LAPACK and plain substitution meet every one of these
conditions on their own.  Only operand shapes and leading dimensions (n, n + 32, n + 128) that the library or tools/
use are passed.

Which factorisation schedule a call reaches depends on the HANDLE, not only on n.  The flag-ordered tail (8 to 4095
tile rows) and the look-ahead steps (52 or more trailing tile rows) need the CU-masked stream pair, which only the first
lane of a handle whose data set has np >= 5120 owns.  A bare handle - `dev`, `dev_noflow`, parts B and C - factorises
in stream order on the full chip at EVERY size, whatever GPMI_OPT_NO_FLOW says.  Part H repeats the exact factor and
`info` on `dev_pair`, a handle that owns the pair, and proves from the library's own launch counters which schedule
each call took.  Part H comes last: by then every other handle of this file that owns a pair (the n = 6656 engine of
part G) has been closed.

Which GEMM kernel a shape reaches (launch_gemm_part; `tiles` counts 128 x 128 tiles):
  k <= 128 or tiles < 384 -> 64 x 64 tiles: the LDS-DMA ring kernel when k % 64 == 0 and k >= 128, else register-staged;
      rectangles of at most 48 tiles with k > 128 use 32 x 64 register-staged tiles instead (the (384, 256) rectangles
      at k = 144, 192, 1024; their lower-triangular twins keep 64 x 64 tiles, and (1024, 1024) at k = 192 is a
      rectangle that reaches the 64 x 64 ring kernel with k > 128);
  tiles >= 384 and k > 128 -> 128 x 128 tiles: the ring kernel when k % 128 == 0, else register-staged.
The 64 x 64 kernels walk the tile list in units of 64: a lower-triangular product of ntc 128-columns has strips of
8, ..., and a last strip of (2 ntc) % 8 (or 8) 64-columns; (6016, 1152) at k = 256 walks 128-tiles with a last strip of 1.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_host as kh

pytestmark = pytest.mark.gpu

needs_longdouble = pytest.mark.skipif(not kh.LONGDOUBLE_OK, reason="np.longdouble has no 64-bit mantissa here")


class Dev:
    """Device buffers and the device-pointer entry points on one handle (as tools/bench_gemm.py uses them)."""

    PAIR_POINTS = 5120  # 40 tile rows: the smallest data set whose first lane gets the CU-masked stream pair

    def __init__(self, no_flow=False, pair=False):
        """`pair`: the handle is given PAIR_POINTS dummy points (d = 1, distinct x, y = 0, unit noise) before anything
        else: lane 0 then owns the CU-masked stream pair and gpmi_dev_potrf, which runs on lane 0, borrows it."""
        from inference_amd import _lib

        self.lib = _lib
        self.h = _lib.Handle(0)
        if pair:
            n = self.PAIR_POINTS
            x, y, noise = np.arange(n, dtype=np.float64), np.zeros(n), np.ones(n)
            self.h.call("gpmi_set_data", _lib.dptr(x), _lib.dptr(y), _lib.dptr(noise), None, n, 1)
        if no_flow:
            self.h.call("gpmi_set_option", _lib.OPT_NO_FLOW, 1)

    def no_flow(self, on):
        """GPMI_OPT_NO_FLOW, read at every factorisation: 1 keeps the flag-ordered tail off"""
        self.h.call("gpmi_set_option", self.lib.OPT_NO_FLOW, int(on))

    def stamps(self, on):
        """The in-kernel stamps of the trailing-update classes (GPMI_PROF_SYRK, _SYRK_REST, _SYRK_SLICE, _FLOW) on or
        off; the counters start from zero."""
        self.h.call("gpmi_profile_enable", (2 << self.lib.PROF_SYRK) if on else 0)
        self.h.call("gpmi_profile_reset")

    def booked(self):
        """{class: (launches, FLOPs)} of the flag-ordered launches (PROF_FLOW), the update slices on the panel stream
        (PROF_SYRK_SLICE) and the 128 x 128-tile trailing updates (PROF_SYRK) since the last stamps() or booked()"""
        out = {}
        for klass in (self.lib.PROF_FLOW, self.lib.PROF_SYRK_SLICE, self.lib.PROF_SYRK):
            launches, flops = C.c_int64(-1), C.c_double(-1.0)
            self.h.call("gpmi_profile_read", klass, C.byref(launches), None, C.byref(flops), None)
            out[klass] = (launches.value, flops.value)
        self.h.call("gpmi_profile_reset")
        return out

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        self.h.call("gpmi_dev_alloc", a.nbytes, C.byref(p))
        self.h.call("gpmi_dev_upload", p, a.ctypes.data_as(C.c_void_p), a.nbytes)
        return p

    def put(self, p, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.h.call("gpmi_dev_upload", p, a.ctypes.data_as(C.c_void_p), a.nbytes)

    def download(self, p, shape):
        out = np.empty(shape)
        self.h.call("gpmi_dev_download", out.ctypes.data_as(C.c_void_p), p, out.nbytes)
        return out

    def free(self, *ptrs):
        for p in ptrs:
            self.h.call("gpmi_dev_free", p)

    def gemm(self, case, same):
        """C -= A B^T of an int_gemm_case / float case dict; `same`: A and B are one buffer (the SYRK shape of the
        trailing updates: B = the first n rows of the panel A lives in).  Returns (whole C buffer, expected E)."""
        m, n, k = case["m"], case["n"], case["k"]
        dC = self.upload(case["C0"])
        if same:
            P = case["P"]
            dP = self.upload(P)
            try:
                self.h.call("gpmi_dev_gemm_nt", dC, case["ldc"], dP, P.shape[1], dP, P.shape[1], m, n, k, case["lower"])
                got = self.download(dC, case["C0"].shape)
            finally:
                self.free(dC, dP)
            return got, case["E_same"]
        dA, dB = self.upload(case["A"]), self.upload(case["B"])
        try:
            self.h.call("gpmi_dev_gemm_nt", dC, case["ldc"], dA, case["lda"], dB, case["ldb"], m, n, k, case["lower"])
            got = self.download(dC, case["C0"].shape)
        finally:
            self.free(dC, dA, dB)
        return got, case["E"]

    def potrf(self, buf, n, repeats=1):
        """In-place factorisation of the n x n matrix in `buf` (pitch buf.shape[1]), `repeats` times from the same
        upload: [(whole buffer, info), ...]."""
        d = self.upload(buf)
        out = []
        try:
            for rep in range(repeats):
                if rep:
                    self.put(d, buf)
                info = C.c_int(-7)
                self.h.call("gpmi_dev_potrf", d, n, buf.shape[1], C.byref(info))
                out.append((self.download(d, buf.shape), info.value))
        finally:
            self.free(d)
        return out


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.h.close()


@pytest.fixture(scope="module")
def dev_noflow():
    d = Dev(no_flow=True)
    yield d
    d.h.close()


def fail_with_tiles(msgs, what):
    if msgs:
        pytest.fail(what + ":\n  " + "\n  ".join(msgs), pytrace=False)


# =========================================================================================== A. gpmi_dev_gemm_nt
def _gemm_case(m, n, k, lower, pads, seed):
    """int_gemm_case with pitches n + pads[0], k + pads[1], k + pads[2], plus the shared operand buffer of the
    same-buffer variant (max(m, n) rows, pitch k + 32) and its expected result."""
    case = kh.int_gemm_case(m, n, k, n + pads[0], k + pads[1], k + pads[2], lower, seed)
    rng = np.random.default_rng(seed + 1000)
    P = np.full((max(m, n), k + 32), kh.OPERAND_PAD)
    P[:, :k] = rng.integers(-4, 5, (max(m, n), k))
    case["P"] = P
    case["E_same"] = kh.gemm_expected(case["C0"], P[:m], P, n, k)
    return case


# (m, n, k, lower, (ldc - n, lda - k, ldb - k)); the distinct-buffer variants cover lda != ldb
SMALL = [(m, n, k, lo, pads)
         for (m, n) in ((128, 128), (256, 128), (384, 256))
         for k, pads in ((16, (32, 32, 128)), (48, (0, 0, 32)), (144, (128, 32, 0)),  # register-staged 64 x 64 (32 x 64)
                         (128, (32, 128, 32)), (192, (32, 32, 128)), (1024, (32, 0, 32)))  # ring 64 x 64 (32 x 64 staged)
         for lo in (0, 1)] + [(1024, 1024, 192, 0, (32, 32, 128))]
# tile-walk edges at k = 128 (64 x 64 ring kernel)
WALK = ([(n, n, 128, 1, (32, 32, 128)) for n in (128, 896, 1024, 1152, 2176)]  # ntc = 1, 7, 8, 9, 17, square
        + [(2304, 128 * c, 128, 1, (32, 32, 0)) for c in (1, 7, 9)]            # ... with tile rows below the triangle
        + [(256, 2176, 128, 0, (32, 32, 128)),    # ntr <= 16 < ntc: the column-major branch (4 x 34 tiles of 64)
           (1024, 1152, 128, 0, (32, 128, 32)),   # ... at its edge: 16 x 18 tiles of 64
           (1152, 1280, 128, 0, (32, 32, 128)),   # 18 x 20: row-major although ntc > ntr
           (2176, 256, 128, 0, (128, 32, 32)),    # ntr > 16
           (640, 384, 128, 0, (32, 32, 128)),     # 60 workgroups
           (384, 128, 128, 0, (0, 32, 128))])     # 12 workgroups
BIG = ([(m, n, k, lo, (32, 32, 128))
        for (m, n, lo) in ((2048, 3072, 0), (3584, 3584, 1), (4096, 2048, 1))   # 384, 406, 392 tiles
        for k in (256, 384, 144, 272)]                                          # ring 128 x 128, register-staged 128 x 128
       + [(6016, 1152, 256, 1, (32, 32, 128))])                                 # 387 tiles: strips of 8 and 1 tile columns


def _id(c):
    return f"{c[0]}x{c[1]}-k{c[2]}-{'lower' if c[3] else 'rect'}"


@pytest.mark.parametrize("shape", SMALL + WALK + BIG, ids=_id)
def test_gemm_integer_exact(dev, shape):
    """C -= A B^T on integers equals the host product bit for bit in the whole buffer: twice, with A and B one buffer
    (the trailing update's SYRK shape) and with distinct buffers of different pitch."""
    m, n, k, lower, pads = shape
    case = _gemm_case(m, n, k, lower, pads, seed=m + 3 * n + 7 * k + lower)
    for same in (True, False):
        got, E = dev.gemm(case, same)
        fail_with_tiles(kh.gemm_mismatches(got, case, E),
                        f"gpmi_dev_gemm_nt m={m} n={n} k={k} lower={lower} ld={case['ldc']}/{case['lda']}/{case['ldb']} "
                        f"{'A and B the same buffer' if same else 'distinct buffers'}")


# one floating-point case per kernel: 64 x 64 staged, 64 x 64 ring, 32 x 64 staged, 128 x 128 ring, 128 x 128 staged
FLOAT = [(128, 128, 48), (384, 256, 128), (384, 256, 192), (2048, 3072, 256), (2048, 3072, 144)]


@needs_longdouble
@pytest.mark.parametrize("m,n,k", FLOAT, ids=lambda v: str(v))
def test_gemm_float_backward_error(dev, m, n, k):
    """Full-mantissa operands spread over six decades per row: rho_gemm <= k + 2, the rigorous bound for any summation
    order with FMA (k products, k + 1 additions, each (1 + delta), |delta| <= u: gamma_{k+1} <= (k + 2) u here) - what a
    reduced-precision product, which the integer cases cannot see, would break by orders of magnitude."""
    Cm, A, B = kh.float_gemm_case(m, n, k, seed=k + m)
    case = dict(m=m, n=n, k=k, ldc=n + 32, lda=k + 32, ldb=k + 128, lower=0, E=None)
    case["C0"] = np.zeros((m, n + 32))
    case["C0"][:, :n] = Cm
    case["A"] = np.zeros((m, k + 32))
    case["A"][:, :k] = A
    case["B"] = np.zeros((n, k + 128))
    case["B"][:, :k] = B
    got, _ = dev.gemm(case, same=False)
    rho = kh.rho_gemm(got[:, :n], Cm, A, B, kh.check_rows(m))
    print(f"\nKERNEL-RHO gemm m={m} n={n} k={k}: rho_gemm {rho:.2f} (cap {k + 2})")
    assert rho <= k + 2
    assert np.array_equal(got[:, n:], case["C0"][:, n:])


# =========================================================================================== B. gpmi_dev_potrf
def _chol_buffers(n, pad, seed, span=3):
    """(L0, A, the buffer to upload).  The 128-tiles strictly above the diagonal hold the padding sentinel instead of
    A's mirror image: the factorisation neither reads nor writes them (the library builds covariance matrices without
    them)."""
    L0, A = kh.int_chol_case(n, seed, span)
    buf = kh.pad_identity(A, n + pad)
    t = np.arange(n) // kh.TILE
    buf[:, :n][t[:, None] < t[None, :]] = kh.C_PAD
    return L0, A, buf


# (n, ld - n, no_flow) on the BARE handles: every case runs the stream-ordered schedule on the full chip, because a bare
# handle has no CU-masked stream pair (the `no_flow` cases differ from the others in their seed and pitch only; the
# schedules that need the pair are part H's).  128: the diagonal kernel alone; 896 / 1024, 1152, 2176: 7, 8, 9 and 17 tile
# rows - a partial last panel and a partial strip; 4096: the first trailing update has 406 tiles at K = 512 (128 x 128
# kernel, split point, mixed launch); 7168: 56 tile rows, fourteen outer panels in stream order.
POTRF = [(128, 32, 0), (256, 0, 0), (896, 32, 0), (1024, 32, 0), (1152, 128, 0), (2176, 32, 0), (4096, 32, 0),
         (1152, 32, 1), (4096, 32, 1), (7168, 32, 0)]


@pytest.mark.parametrize("n,pad,no_flow", POTRF,
                         ids=[f"n{n}-ld+{p}-bare{'-noflow' if nf else ''}{'-slow' if n == 7168 else ''}" for n, p, nf in POTRF])
def test_potrf_integer_exact(dev, dev_noflow, n, pad, no_flow):
    """The factor of A = L0 L0^T is L0 bit for bit (here: on a bare handle, in stream order; part H: the flag-ordered
    and look-ahead schedules): every pivot is exactly 1 (the refinements of
    rcp_newton, rsqrt_refined and factor16_steps.h return 1.0 for 1.0 whatever the hardware seed), every inverse
    diagonal block I, every TRSM and update integer arithmetic.  The rest of the buffer as include/gpmi.h states it:
    padding columns, strictly-upper tiles and the upper triangle of tile (0, 0) untouched, the upper triangles of the
    other diagonal tiles workspace.  Factored twice on one handle: the second buffer is bit-identical to the first.
    (n = 7168 is this file's one slow case: its half-gigabyte matrix is built, uploaded and compared on the host.)"""
    L0, A, buf0 = _chol_buffers(n, pad, seed=n + no_flow)
    (got, info), (got2, info2) = (dev_noflow if no_flow else dev).potrf(buf0, n, repeats=2)
    assert info == 0 and info2 == 0
    fail_with_tiles(kh.chol_mismatches(got, buf0, L0), f"gpmi_dev_potrf n={n} ld={n + pad} no_flow={no_flow}")
    same = got.view(np.int64) == got2.view(np.int64)
    fail_with_tiles(kh._tile_report(~same, "differ between two factorisations of the same upload", got, got2),
                    f"gpmi_dev_potrf n={n} repeated")


# =========================================================================================== C. info
INFO_K = [1, 16, 17, 128, 129, 640, 1152]


@pytest.fixture(scope="module")
def info_case():
    return _chol_buffers(1152, 32, seed=77)


@pytest.mark.parametrize("no_flow", [0, 1], ids=["bare", "bare-noflow"])
def test_potrf_info_is_the_leading_minor(dev, dev_noflow, info_case, no_flow):
    """(Bare handles: stream order either way.)  A[k-1, k-1] lowered by 2 makes the k-th pivot exactly -1 (it is 1 in the sound matrix, and the entry enters no
    earlier pivot): info == k, the order of the first leading minor that is not positive definite.  Only the
    factorisation is called on these matrices."""
    L0, A, buf0 = info_case
    d = dev_noflow if no_flow else dev
    assert d.potrf(buf0, 1152)[0][1] == 0
    for k in INFO_K:
        buf = buf0.copy()
        buf[k - 1, k - 1] -= 2.0
        assert d.potrf(buf, 1152)[0][1] == k, f"pivot {k} = -1 (no_flow={no_flow})"
    # two bad pivots: the first is reported
    buf = buf0.copy()
    buf[640, 640] -= 2.0
    buf[16, 16] -= 2.0
    assert d.potrf(buf, 1152)[0][1] == 17


def test_potrf_info_reports_a_nan_pivot(dev):
    """One NaN on the diagonal, at row 129 of a 256 x 256 matrix (stream order): the pivot is not finite, info == 130."""
    L0, A, buf0 = _chol_buffers(256, 32, seed=78)
    buf0[129, 129] = np.nan
    assert dev.potrf(buf0, 256)[0][1] == 130


def _engine(n, y):
    from inference_amd._engine import GpEngine

    return GpEngine(np.zeros((n, 1)), y)


def test_fit_dense_info_at_a_ragged_size():
    """The same through gpmi_fit_dense at n = 1000 (padded to 1024 with an identity block): info == k up to k = n, and
    0 for the sound matrix - the padding is never reported."""
    n = 1000
    L0, A = kh.int_chol_case(n, seed=79)
    eng = _engine(n, np.zeros(n))
    try:
        assert eng.fit_dense(A, np.zeros(n))[2] == 0
        for k in (1, 16, 17, 128, 129, 640, 1000):
            Ak = A.copy()
            Ak[k - 1, k - 1] -= 2.0
            assert eng.fit_dense(Ak, np.zeros(n))[2] == k, f"pivot {k} = -1"
        assert eng.fit_dense(A, np.zeros(n))[2] == 0  # and the handle factorises a sound matrix again
    finally:
        eng.close()


# =========================================================================================== D. dense entry points
@pytest.mark.parametrize("n", [127, 128, 129, 1000, 2048, 4224])
def test_fit_dense_integer_exact(n):
    """fit_dense(A = L0 L0^T, mu = 0) with y = A a0: get_L() == L0, alpha == a0 and logdet == 0.0 exactly.  The single
    right-hand-side sweeps multiply by the inverse diagonal blocks (exactly I) and subtract integer products: with
    |a0| <= 3 and L0 in {-1, 0, 1} every intermediate (L0^T a0, its partial sums) is an integer below n * 3 < 2^53."""
    L0, A = kh.int_chol_case(n, seed=n + 5)
    a0 = np.random.default_rng(n + 6).integers(-3, 4, n).astype(float)
    y = A @ a0  # exact: |entries| <= 3 n^2
    eng = _engine(n, y)
    try:
        for rep in range(2):
            alpha, logdet, info = eng.fit_dense(A, np.zeros(n))
            assert info == 0
            L = eng.get_L()
            fail_with_tiles(kh._tile_report(L != L0, "differ from L0", L, L0), f"fit_dense + get_L n={n}")
            bad = np.flatnonzero(alpha != a0)
            assert bad.size == 0, f"alpha differs at {bad[:8]} (128-blocks {sorted(set((bad // 128).tolist()))[:8]})"
            assert logdet == 0.0
    finally:
        eng.close()


_SOLVE = {}


@pytest.fixture(scope="module")
def solve_engines():
    """One fitted engine per n for the many-right-hand-side tests: (engine, L0, a0)."""

    def get(n):
        if n not in _SOLVE:
            L0, A = kh.int_chol_case(n, seed=n + 9)
            a0 = np.random.default_rng(n + 10).integers(-3, 4, n).astype(float)
            eng = _engine(n, A @ a0)
            alpha, logdet, info = eng.fit_dense(A, np.zeros(n))
            assert info == 0 and np.array_equal(alpha, a0)
            _SOLVE[n] = (eng, L0, a0)
        return _SOLVE[n]

    yield get
    for eng, _, _ in _SOLVE.values():
        eng.close()
    _SOLVE.clear()


# m = 1664 (n = 640 only): mt = 13 tile rows, where the out-of-place product with the inverse blocks leaves the 32-row tiles
SOLVE_ROWS = [(n, m) for n in (640, 2176) for m in (1, 127, 129, 513)] + [(640, 1664)]


@pytest.mark.parametrize("n,m", SOLVE_ROWS, ids=[f"{n}-{m}" for n, m in SOLVE_ROWS])
def test_solve_rows_and_predict_dense_integer_exact(solve_engines, n, m):
    """X = Q L0^-T for Q = X0 L0^T with X0 from {-1, 0, 1}, its Gram matrix, and predict_dense on the same rows: all
    required bit for bit.  Why every intermediate of the many-right-hand-side path (solve.hip: build_inv2,
    trsm_rows_forward) is an integer below 2^53 for these inputs:
      * the inverse diagonal blocks invD are exactly I; build_inv2 forms the inverse of each 512-wide diagonal block of
        L0 (identity 128-blocks, N strictly block-lower with entries in {-1, 0, 1}) as products of integer blocks:
        I - N + N^2 - N^3, entries bounded by 1 + 2 * 128 + 128^2 < 2^15 (N^2 sums over at most two 128-blocks, N^3
        over one pair of them);
      * Q has entries |q| <= n < 2^12; the block solve X_J = Q_J inv2^T sums 512 integer products below 2^27 each
        (< 2^36 in all) to an entry of X0; the K = 512 update Q -= X_J L^T subtracts integer products of entries of
        X0 and L0;
      * the Gram matrix sums n products of entries of X0 (|G| <= n) and is therefore exactly symmetric; kalpha sums
        q_j a0_j (|.| <= 3 n^2), sumsq sums x^2.
    The backward row solve (trsm_rows_backward) and the in-place forward one are not on the path of these entry points:
    parts F and G below.  m = 1664 (mt = 13 > 12) moves the product with the inverse blocks from 32 x 32 register-staged
    tiles to the 64 x 64 ring kernel with the contraction cut at the diagonal (kskip 2)."""
    eng, L0, a0 = solve_engines(n)
    X0 = np.random.default_rng(n + 31 * m).integers(-1, 2, (m, n)).astype(float)
    Q = X0 @ L0.T
    X, G = eng.solve_rows(Q, want_rows=True, want_gram=True)
    fail_with_tiles(kh._tile_report(X != X0, "differ from X0", X, X0), f"solve_rows n={n} m={m}")
    Gx = X0 @ X0.T
    fail_with_tiles(kh._tile_report(G != Gx, "differ from X0 X0^T", G, Gx), f"solve_rows Gram n={n} m={m}")
    assert np.array_equal(G, G.T)
    G_only = eng.solve_rows(Q, want_rows=False, want_gram=True)[1]
    assert np.array_equal(G_only, Gx)
    ka, ss = eng.predict_dense(Q)
    assert np.array_equal(ka, Q @ a0), np.flatnonzero(ka != Q @ a0)[:8]
    assert np.array_equal(ss, (X0 ** 2).sum(1)), np.flatnonzero(ss != (X0 ** 2).sum(1))[:8]


# =========================================================================================== E. bounds on real matrices
@needs_longdouble
@pytest.mark.parametrize("kind", ["well", "graded", "gp"])
@pytest.mark.parametrize("n", [129, 640, 1152])
def test_backward_error_bounds(dev, n, kind):
    """Componentwise backward errors of the factor, the many-right-hand-side solve, alpha and K^-1 on real-valued
    matrices, in units of u with residuals in longdouble.  A standard Cholesky or substitution satisfies each ratio with
    n + 1; every multiplication by an explicitly inverted diagonal block (128 wide in the factorisation and the
    sweeps, 512 wide in solve_rows) may cost a factor of that block's condition number kappa_b, measured on LAPACK's
    factor.  The caps come from that reasoning, not from the device (tests/test_kernel_host_cpu.py: the references meet
    them with kappa = 0); the achieved values are tabulated in DESIGN.md section 2."""
    A = kh.spd_case(n, kind, seed=n)
    L_ref = np.linalg.cholesky(A)
    k128, k512 = kh.kappa_blocks(L_ref, 128), kh.kappa_blocks(L_ref, 512)
    cond = float(np.linalg.cond(A, 2))
    rng = np.random.default_rng(n + 1)
    Q = rng.standard_normal((129, n))
    r = rng.standard_normal(n)
    rows = kh.check_rows(n)
    # gpmi_dev_potrf on blockdiag(A, I), the padding the library itself applies
    npad = -(-n // 128) * 128
    buf0 = kh.pad_identity(A, npad + 32)
    got, info = dev.potrf(buf0, npad)[0]
    assert info == 0
    L_dev = np.tril(got[:n, :n])
    rho_p = kh.rho_chol(A, L_dev, rows)
    eng = _engine(n, r)
    try:
        alpha, logdet, info = eng.fit_dense(A, np.zeros(n))
        assert info == 0
        L = eng.get_L()
        rho_f = rho_p if np.array_equal(L, L_dev) else kh.rho_chol(A, L, rows)
        X = eng.solve_rows(Q)[0]
        rho_x = kh.rho_solve_rows(X, L, Q)
        rho_a = kh.rho_solve(A, alpha, r)
        lml, alpha2, iK, info = eng.lml_dense(A, np.zeros(n), want_alpha=True, want_inverse=True)
        assert info == 0
    finally:
        eng.close()
    res = kh.inverse_residual(A, iK, rows)
    print(f"\nKERNEL-RHO n={n} {kind}: kappa_128 {k128:.2e} kappa_512 {k512:.2e} cond {cond:.2e} | rho_chol dev_potrf "
          f"{rho_p:.2f} fit_dense {rho_f:.2f} (cap {kh.cap_chol(n, k128):.3g}) | rho_solve_rows {rho_x:.2f} (cap "
          f"{kh.cap_solve_rows(n, k512):.3g}) | rho_alpha {rho_a:.2f} (cap {kh.cap_alpha(n, k128):.3g}) | |A iK - I| "
          f"{res:.2e} (cap {kh.cap_inverse(n, cond, k128):.2e})")
    assert rho_p <= kh.cap_chol(n, k128)
    assert rho_f <= kh.cap_chol(n, k128)
    assert rho_x <= kh.cap_solve_rows(n, k512)
    assert rho_a <= kh.cap_alpha(n, k128)
    assert np.array_equal(iK, iK.T), "K^-1 of lml_dense is not bit-symmetric"
    assert res <= kh.cap_inverse(n, cond, k128)
    assert np.array_equal(alpha2, alpha) or kh.rho_solve(A, alpha2, r) <= kh.cap_alpha(n, k128)


# =========================================================================================== F. K^-1 and leave-one-out
# Exact on the factors of kernel_host.int_nilpotent_chol_case, whose inverse W = L0^-1 is a small-integer matrix.  The
# path (api_single.hip: LN_INVERSE | LN_SYRK | LN_MIRROR, lane_loo_middle) and what each size reaches:
#   * L^-T from the identity: trsm_rows_forward IN PLACE (Qout == nullptr: the product with the 512 x 512 inverse block
#     goes to the scratch panel, copy_panel_kernel brings it back) with upper_rhs (block row t joins at its own outer
#     block: mt = Je).  The products have kskip 2 and run on 32 x 32 tiles up to mt = 12; n = 2176 adds mt = 16 (w = 4:
#     gemm_dma64_kernel<TILES_RECT, OP_ASSIGN>, the 64 x 64 ring kernel with the shortened contraction) and mt = 17
#     (w = 1: the 32 x 128 one-tile-column form);
#   * build_inv2: nt % 4 == 3 (the 1 x 2 corner) at n = 384 and 896, 0 at 1024 and 1536, 1 at 640 and 2176, 2 at 768; n = 900 is
#     the 1024 case cut to 900 rows, the identity padding inside the last tile;
#   * K^-1 = L^-T L^-1: lane_syrk(.., 1), always 128 x 128 tiles, gemm_dma_kernel<TILES_LOWER, OP_ASSIGN> with the
#     contraction of tile row ti started at kbeg = 128 ti; then mirror_lower_kernel;
#   * diag K^-1: rows_sumsq over L^-T and launch_negate.
_NIL = {}


@pytest.fixture(scope="module")
def nil_cases():
    """One case per n, built once: dict(L0, W, A, iK = W^T W, a0 in [-3, 3], y = A a0, v = L0^T a0)."""

    def get(n):
        if n not in _NIL:
            L0, W, A = kh.int_nilpotent_chol_case(dict(kh.NILPOTENT_CASES)[n], kh.NILPOTENT_SEED, n)
            a0 = np.random.default_rng(n + 1).integers(-3, 4, n).astype(float)
            _NIL[n] = dict(L0=L0, W=W, A=A, iK=W.T @ W, a0=a0, y=A @ a0, v=L0.T @ a0)  # exact: integers below 3 n^2
        return _NIL[n]

    yield get
    _NIL.clear()


NIL_N = [n for n, _ in kh.NILPOTENT_CASES]


@pytest.mark.parametrize("n", NIL_N)
def test_inverse_integer_exact(nil_cases, n):
    """lml_dense(A, 0, want_alpha, want_inverse) on A = L0 L0^T with y = A a0, twice on one engine: info == 0,
    alpha == a0, K^-1 == W^T W in every entry (structural zeros, the identity block of the last group and both
    triangles included; a failure names its tiles), K^-1 bit-symmetric, and lml == -(v . v) / 2 with v = L0^T a0
    (ln 1 = 0; v . v is an integer below 9 n^3).  Why it is exact: kernel_host.int_nilpotent_chol_case."""
    c = nil_cases(n)
    eng = _engine(n, c["y"])
    try:
        for rep in range(2):
            lml, alpha, iK, info = eng.lml_dense(c["A"], np.zeros(n), want_alpha=True, want_inverse=True)
            assert info == 0
            bad = np.flatnonzero(alpha != c["a0"])
            assert bad.size == 0, f"alpha differs at {bad[:8]} (128-blocks {sorted(set((bad // 128).tolist()))[:8]})"
            fail_with_tiles(kh._tile_report(iK != c["iK"], "differ from W^T W", iK, c["iK"]),
                            f"lml_dense K^-1 n={n} (evaluation {rep})")
            assert np.array_equal(iK, iK.T), "K^-1 of lml_dense is not bit-symmetric"
            assert lml == -0.5 * (c["v"] @ c["v"])
    finally:
        eng.close()


@needs_longdouble
@pytest.mark.parametrize("n", NIL_N)
def test_leave_one_out_pieces_exact_and_bounded(nil_cases, n):
    """loo_dense(A, 0, want_gradient_pieces=True) on the same matrices: alpha == a0 and diag K^-1 == diag(W^T W)
    exactly.  p = K^-1 c1 and W_out = K^-1 diag(c2) K^-1 are not integer (c1 = alpha / d and sqrt(c2) come from a
    division and a square root); with K^-1 itself exact they are held to componentwise caps in units of u, residuals in
    longdouble against c1, c2 evaluated in longdouble from a0 and the exact diagonal:
      |p - K^-1 c1| <= (n + 4) u |K^-1| |c1|                          (kernel_host.cap_loo_p)
      |W_out - K^-1 diag(c2) K^-1| <= (n + 12) u |K^-1| diag(c2) |K^-1|   (kernel_host.cap_loo_w)
    Each is the n-term dot-product bound for any order of summation - a term is rounded once as a product and at most
    n - 1 times in the additions (or n times by FMAs): (1 + delta)^n - plus the roundings of the operands: 2 for c1 (the
    reciprocal and the product), 10 for a product of two entries of G = K^-1 diag(sqrt c2) (under the root 1 / d, two
    products with alpha, the addition, the product with var / 2 - var counted twice: 6 roundings, halved by the root, plus
    the root's own and the scaling of the column: 5 per entry); gamma_(n + 2) < (n + 3) u, gamma_(n + 10) < (n + 11) u,
    and one unit for the reference.  tests/test_kernel_host_cpu.py: plain fp64 NumPy meets both.  W_out is the SYRK
    without k-skipping (lane_syrk(.., 0)) of the column-scaled inverse and must be bit-symmetric."""
    c = nil_cases(n)
    eng = _engine(n, c["y"])
    try:
        alpha, ikdiag, p, Wm, info = eng.loo_dense(c["A"], np.zeros(n), want_gradient_pieces=True)
    finally:
        eng.close()
    assert info == 0
    bad = np.flatnonzero(alpha != c["a0"])
    assert bad.size == 0, f"alpha differs at {bad[:8]}"
    d = np.diag(c["iK"]).copy()
    bad = np.flatnonzero(ikdiag != d)
    assert bad.size == 0, f"diag K^-1 differs at {bad[:8]}: got {ikdiag[bad[:4]]}, want {d[bad[:4]]}"
    rho_p = kh.rho_loo_p(p, c["iK"], c["a0"], d)
    rho_w = kh.rho_loo_w(Wm, c["iK"], c["a0"], d)
    print(f"\nKERNEL-RHO loo n={n}: rho_loo_p {rho_p:.2f} (cap {kh.cap_loo_p(n)}) | rho_loo_w {rho_w:.2f} (cap {kh.cap_loo_w(n)})")
    assert rho_p <= kh.cap_loo_p(n)
    assert rho_w <= kh.cap_loo_w(n)
    assert np.array_equal(Wm, Wm.T), "W of loo_dense is not bit-symmetric"


# =========================================================================================== G. Z = Q K^-1
# solve_rows_kinv runs the pair of in-place row solves of the spatial derivatives on caller-built rows: the in-place
# trsm_rows_forward WITHOUT upper_rhs, then trsm_rows_backward - per outer block, from the last to the first, the k-major
# product with the untransposed inverse block (kskip 4, kbeg = tj * BN, the mirrored tile-column order; 32 x 32 tiles at
# every shape the 1024-row chunk allows), the k-major K = 512 OP_SUB update of the columns to the left (64 x 64
# register-staged tiles; 128 x 128 from mt * J >= 384 tiles on) and the copy of the panel back into Q.
# On the dense int_chol_case(n): the global inverse is never formed, only the 512-block inverses (entries below 2^15, see
# test_solve_rows_and_predict_dense_integer_exact).  Z0 from {-1, 0, 1}, Q = Z0 A; the forward solve returns X = Z0 L0
# (|x| <= n) from right-hand sides whose partial sums are sums of products of entries of X and L0 (below n^2), the
# backward one Z0 from X; a product with an inverse block sums 512 products of an entry bounded like Q and one below 2^15:
# 512 |Q|.max 2^15 < 2^53, asserted by kernel_host.rows_kinv_case.
def _rows_kinv_check(eng, A, n, m):
    Z0, Q = kh.rows_kinv_case(A, m, seed=n + 37 * m)
    Z = eng.solve_rows_kinv(Q)
    fail_with_tiles(kh._tile_report(Z != Z0, "differ from Z0", Z, Z0), f"solve_rows_kinv n={n} m={m}")


# (2176, 1024): mt * w * 16 = 512, the last shape of the backward product on 32 x 32 tiles by its own rule; (2176, 1025):
# a second chunk of one row; (6656, 1024), the slow one: the smallest shape whose update has mt * J >= 384 tiles and
# runs gemm_nt_kernel<TILES_RECT, OP_SUB, k-major, 128, 128>
@pytest.mark.parametrize("n,m", kh.ROWS_KINV_CASES,
                         ids=[f"n{n}-m{m}{'-slow' if n == 6656 else ''}" for n, m in kh.ROWS_KINV_CASES])
def test_rows_kinv_integer_exact(solve_engines, n, m):
    """Z = Q K^-1 through solve_rows_kinv equals Z0 bit for bit; a failure names its tiles."""
    if n != 6656:
        eng, L0, a0 = solve_engines(n)
        _rows_kinv_check(eng, kh.int_chol_case(n, seed=n + 9)[1], n, m)  # (the matrix the engine was fitted with)
        return
    L0, A = kh.int_chol_case(n, seed=n + 9)
    eng = _engine(n, np.zeros(n))
    try:
        assert eng.fit_dense(A, np.zeros(n))[2] == 0
        _rows_kinv_check(eng, A, n, m)
    finally:
        eng.close()


def test_rows_kinv_narrow_steps_integer_exact(tmp_path):
    """The same at (2176, 129) over the 128-wide steps of the backward solve (GPMI_BACKWARD_OB=0: one in-place k-major
    product with invD_k and one K = 128 update per tile column).  The switch is read once per process: a fresh child."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, m = 2176, 129
    code = (
        "import sys\n"
        f"sys.path[:0] = [{root!r}, {os.path.join(root, 'inference-tools_amd')!r}, {os.path.join(root, 'tests')!r}]\n"
        "import numpy as np, kernel_host as kh\n"
        "from inference_amd._engine import GpEngine\n"
        "n, m = int(sys.argv[2]), int(sys.argv[3])\n"
        "L0, A = kh.int_chol_case(n, seed=n + 9)\n"
        "Z0, Q = kh.rows_kinv_case(A, m, seed=n + 37 * m)\n"
        "eng = GpEngine(np.zeros((n, 1)), np.zeros(n))\n"
        "info = eng.fit_dense(A, np.zeros(n))[2]\n"
        "Z = eng.solve_rows_kinv(Q)\n"
        "eng.close()\n"
        "np.savez(sys.argv[1], info=np.array([info]), Z=Z, Z0=Z0)\n")
    out = str(tmp_path / "narrow.npz")
    run = subprocess.run([sys.executable, "-c", code, out, str(n), str(m)], env=dict(os.environ, GPMI_BACKWARD_OB="0"),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    r = dict(np.load(out))
    assert r["info"][0] == 0
    fail_with_tiles(kh._tile_report(r["Z"] != r["Z0"], "differ from Z0", r["Z"], r["Z0"]),
                    f"solve_rows_kinv n={n} m={m} over 128-wide steps")


def test_rows_kinv_leaves_the_engine_intact(solve_engines):
    """solve_rows_kinv solves in place in the query workspace and reuses the cached inverse blocks: solve_rows and
    predict_dense on the same engine still return their exact results afterwards, and so does a second call."""
    n, m = 2176, 129
    eng, L0, a0 = solve_engines(n)
    A = kh.int_chol_case(n, seed=n + 9)[1]
    _rows_kinv_check(eng, A, n, m)
    X0 = np.random.default_rng(n + 31 * m).integers(-1, 2, (m, n)).astype(float)
    Q = X0 @ L0.T
    X = eng.solve_rows(Q)[0]
    fail_with_tiles(kh._tile_report(X != X0, "differ from X0", X, X0), f"solve_rows after solve_rows_kinv n={n} m={m}")
    ka, ss = eng.predict_dense(Q)
    assert np.array_equal(ka, Q @ a0) and np.array_equal(ss, (X0 ** 2).sum(1))
    _rows_kinv_check(eng, A, n, m + 1)


# =========================================================================================== H. on a handle with the pair
# gpmi_dev_potrf on a handle whose lane 0 owns the CU-masked stream pair (Dev(pair=True)): the only way the device-pointer
# entry point reaches potrf_flow.hip and the look-ahead steps of potrf_lower.  Schedule by size (nt tile rows):
#   nt < 8 (896)                     stream order, no flag-ordered launch
#   8 <= nt < 56 (1024 .. 4096)      the whole matrix is ONE flag-ordered launch of nt rows
#   7168 (nt = 56)                   panel 0 in stream order; step 0 overlapped (52 trailing rows: columns of panel 1, panel 1 on
#                                    the 32-CU stream beside the rest of the update on the others); then a 48-row flag-ordered tail
#   7680 (nt = 60)                   two overlapped steps in a row (56 and 52 trailing rows: the second waits for the first's
#                                    ev_main / ev_panel, and for ev_slice if the first had sliced), then the same 48-row tail
# The witnesses.  With the in-kernel stamps on (gpmi_profile_enable(2 << PROF_SYRK)) potrf_flow_tail books one launch and
# the FLOPs of its update tasks under GPMI_PROF_FLOW.  Those FLOPs are a function of the tail's tile rows alone
# (kernel_host.flow_update_flops, checked against the shipped task lists by tests/test_kernel_host_cpu.py): a launch
# count of 1 with the FLOPs of nt rows says the whole matrix went through the task kernel, a count of 1 with the FLOPs of
# 48 rows at nt = 56 / 60 says the steps before it were the overlapped ones - a tail entered one step early or late would
# book 52 or 44 rows, a whole-matrix launch 56 or 60, and they all differ.  (GPMI_PROF_SYRK_SLICE cannot serve at these
# sizes: slice_tiles of potrf.hip gives (su - chain) / (per_main + per_panel) = 24 tiles at 52 trailing rows and 42 at
# 56 with 224 + 32 CUs and the fused panel column, both below one round of 64, so no slice is launched; the tests assert
# that too.)  A count of 0 on this handle where a launch is due, an `info` of GPMI_INFO_FLOW_TIMEOUT (-6), a RuntimeWarning
# or a handle that has fallen back to GPMI_OPT_NO_FLOW fail the test: nothing here may pass by way of the stream-ordered
# schedule.
# Observed on an MI355X: see DESIGN.md section 2.1 for the counts and durations.
PAIR_TAIL_ROWS = 48  # trailing tile rows at which the look-ahead regime (GPMI_LOOKAHEAD_MIN = 52, outer panels of 4) ends


def _flow_rows(n):
    """Tile rows of the flag-ordered launch of an n x n factorisation on a handle with the pair (0: none)."""
    nt = n // kh.TILE
    if nt < 8:
        return 0
    return nt if nt - 4 < 52 else PAIR_TAIL_ROWS


_PAIR_CASES = {}


@pytest.fixture(scope="module")
def pair_case():
    """_chol_buffers(n, 32, seed=n); the sizes that both the exact and the info test use are built once and kept."""

    def get(n):
        if n in _PAIR_CASES:
            return _PAIR_CASES[n]
        case = _chol_buffers(n, 32, seed=n)
        if n in (1152, 2176, 7168):
            _PAIR_CASES[n] = case
        return case

    yield get
    _PAIR_CASES.clear()


@pytest.fixture(scope="module")
def dev_pair():
    d = Dev(pair=True)
    yield d
    d.h.close()


def _witness(d, n, expect_rows, what):
    """Reads and prints the counters of the factorisation just run and holds them to `expect_rows` (0: stream order)."""
    booked = d.booked()
    launches, flops = booked[d.lib.PROF_FLOW]
    slices = booked[d.lib.PROF_SYRK_SLICE][0]
    print(f"\nFLOW-WITNESS {what} n={n}: FLOW launches {launches}, FLOPs {flops:.6e} (a {expect_rows}-row launch books "
          f"{kh.flow_update_flops(expect_rows):.6e}), SYRK_SLICE launches {slices}, SYRK launches {booked[d.lib.PROF_SYRK][0]}")
    assert not getattr(d.h, "_no_flow", False), "the handle has fallen back to the stream-ordered schedule"
    if expect_rows == 0:
        assert launches == 0, f"{what} n={n}: a flag-ordered launch where none is due"
        return
    assert launches >= 1, f"{what} n={n}: no flag-ordered launch - this call ran in stream order"
    assert launches == 1 and flops == kh.flow_update_flops(expect_rows), \
        f"{what} n={n}: {launches} launches booking {flops!r} FLOPs, not one launch of {expect_rows} tile rows"
    assert slices == 0


PAIR_N = [896, 1024, 1152, 2176, 4096, 7168, 7680]


@pytest.mark.filterwarnings("error::RuntimeWarning")
@pytest.mark.parametrize("n", PAIR_N, ids=[f"n{n}-pair{'-slow' if n >= 7168 else ''}" for n in PAIR_N])
def test_potrf_integer_exact_on_the_pair_handle(dev_pair, pair_case, n):
    """test_potrf_integer_exact in the flag-ordered and look-ahead schedules (ld = n + 32): factored twice with the
    flag-ordered tail allowed - the first time with the stamps on, for the witness - and once under GPMI_OPT_NO_FLOW
    on the same handle (where 7168 and 7680 keep their overlapped steps and finish in stream order).  All three buffers
    are exact everywhere (kernel_host.chol_mismatches: factor, padding, strictly-upper tiles, tile (0, 0)), the two
    repeats are bit-identical, and info == 0 (never -6, the time-out of a flag-ordered poll).
    Witness: GPMI_PROF_FLOW launches and FLOPs, see the comment above - one launch of n / 128 rows for 1024 .. 4096, one
    of 48 rows for 7168 and 7680 (the look-ahead witness: slice_tiles is 0 at these sizes, so the FLOPs of the tail
    are what tells an overlapped step from a stream-ordered one), none at 896 and none under GPMI_OPT_NO_FLOW."""
    d = dev_pair
    L0, A, buf0 = pair_case(n)
    rows = _flow_rows(n)
    p = d.upload(buf0)
    try:
        def run(label, stamped, expect_rows):
            d.put(p, buf0)
            if stamped:
                d.stamps(True)
            info = C.c_int(-7)
            try:
                d.h.call("gpmi_dev_potrf", p, n, buf0.shape[1], C.byref(info))
                if stamped:
                    _witness(d, n, expect_rows, label)
            finally:
                d.stamps(False)
            assert info.value == 0, f"{label} n={n}: info {info.value}"
            got = d.download(p, buf0.shape)
            fail_with_tiles(kh.chol_mismatches(got, buf0, L0), f"gpmi_dev_potrf on the pair handle, {label}, n={n} ld={n + 32}")
            return got

        first = run("flag-ordered, first", True, rows)
        second = run("flag-ordered, second", False, rows)
        same = first.view(np.int64) == second.view(np.int64)
        fail_with_tiles(kh._tile_report(~same, "differ between two factorisations of the same upload", first, second),
                        f"gpmi_dev_potrf on the pair handle n={n} repeated")
        del first, second, same
        d.no_flow(1)
        try:
            run("GPMI_OPT_NO_FLOW", True, 0)
        finally:
            d.no_flow(0)
    finally:
        d.free(p)


def test_bare_handle_books_no_flag_ordered_launch(dev):
    """The other side of the witness: the same call on a bare handle, at a size part H factors as one flag-ordered
    launch, books none."""
    n = 1152
    L0, A, buf0 = _chol_buffers(n, 32, seed=n)
    dev.stamps(True)
    try:
        (got, info), = dev.potrf(buf0, n)
        _witness(dev, n, 0, "bare handle")
    finally:
        dev.stamps(False)
    assert info == 0
    fail_with_tiles(kh.chol_mismatches(got, buf0, L0), f"gpmi_dev_potrf on the bare handle, stamps on, n={n}")


# n -> [(label, {row: new diagonal value or None for "lowered by 2"}, expected info)]
def _pair_info_cases(n):
    if n == 1152:
        cases = [(f"pivot {k} = -1", {k - 1: None}, k) for k in INFO_K]
        cases.append(("pivots 17 and 641 = -1", {640: None, 16: None}, 17))   # the first is reported
        cases.append(("NaN on the diagonal at row 700", {700: np.nan}, 701))
        return cases
    ks = {2176: (2049, 2176),  # the ragged last panel (tile row 16 alone)
          # first panel, before anything overlaps; the panel factored on the 32-CU stream beside the overlapped update;
          # inside the flag-ordered tail; the last pivot
          7168: (100, 642, 4024, 7168)}[n]
    return [(f"pivot {k} = -1", {k - 1: None}, k) for k in ks]


@pytest.mark.filterwarnings("error::RuntimeWarning")
@pytest.mark.parametrize("n", [1152, 2176, 7168], ids=["n1152-pair", "n2176-pair", "n7168-pair-slow"])
def test_potrf_info_on_the_pair_handle(dev_pair, pair_case, n):
    """test_potrf_info_is_the_leading_minor where the failing pivot sits inside the task kernel's launch or beside an
    overlapped update: every call returns info == k - not GPMI_INFO_FLOW_TIMEOUT, no error, no warning -, every one of
    them took the flag-ordered schedule (witness as above, stamps on throughout), and after EVERY failing call the next
    factorisation of the sound matrix on the same handle gives the bits of the first one, which is checked against L0: no
    flag, abort word or task-list state survives an abandoned factorisation."""
    d = dev_pair
    L0, A, buf0 = pair_case(n)
    rows = _flow_rows(n)
    ld = buf0.shape[1]
    p = d.upload(buf0)
    d.stamps(True)
    try:
        def factor(label):
            info = C.c_int(-7)
            d.h.call("gpmi_dev_potrf", p, n, ld, C.byref(info))
            _witness(d, n, rows, label)
            return info.value

        assert factor("sound") == 0
        ref = d.download(p, buf0.shape)
        fail_with_tiles(kh.chol_mismatches(ref, buf0, L0), f"gpmi_dev_potrf on the pair handle n={n}")
        for label, changes, want in _pair_info_cases(n):
            kept = {r: buf0[r, r] for r in changes}
            for r, v in changes.items():
                buf0[r, r] = kept[r] - 2.0 if v is None else v
            try:
                d.put(p, buf0)
            finally:
                for r, v in kept.items():
                    buf0[r, r] = v
            got = factor(label)
            assert got == want, f"n={n}, {label}: info {got}, expected {want}"
            d.put(p, buf0)
            assert factor(f"sound, after {label}") == 0
            again = d.download(p, buf0.shape)
            same = again.view(np.int64) == ref.view(np.int64)
            fail_with_tiles(kh._tile_report(~same, "differ from the factorisation before the failing one", again, ref),
                            f"gpmi_dev_potrf on the pair handle n={n}, sound matrix after {label}")
    finally:
        d.stamps(False)
        d.free(p)
