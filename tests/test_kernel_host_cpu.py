"""
The references of the kernel-level GPU tests (tests/test_kernels_gpu.py), checked without a GPU: LAPACK and a plain
NumPy substitution alone meet every condition those tests impose on the device - bit equality on the integer cases, the
backward-error caps with kappa = 0 on the real-valued ones - and the comparison helpers fail, naming the tile, when a
result is off by one in one place.
"""
import numpy as np
import pytest

import kernel_host as kh

needs_longdouble = pytest.mark.skipif(not kh.LONGDOUBLE_OK, reason="np.longdouble has no 64-bit mantissa here")

# (n, span) of every int_chol_case the GPU tests use
CHOL_SIZES = [(128, 3), (256, 3), (896, 3), (1024, 3), (1152, 3), (2176, 3), (4096, 3), (7168, 3), (7680, 3),
              (127, 1), (129, 1), (640, 1), (1000, 1), (2048, 1), (2176, 1), (4224, 1)]


@pytest.mark.parametrize("n,span", CHOL_SIZES)
def test_lapack_reproduces_the_integer_factor(n, span):
    L0, A = kh.int_chol_case(n, seed=n, span=span)
    assert np.array_equal(A, A.T)
    assert np.array_equal(np.diag(L0), np.ones(n)) and np.array_equal(L0, np.tril(L0))
    for s in range(0, n, kh.TILE):  # identity diagonal blocks, dense blocks below them
        assert np.array_equal(L0[s:s + kh.TILE, s:s + kh.TILE], np.eye(min(kh.TILE, n - s)))
    if n > kh.TILE:
        assert np.count_nonzero(L0[kh.TILE:, :kh.TILE]) > 0.5 * L0[kh.TILE:, :kh.TILE].size * (1 if span > 1 else 0.9)
    L = np.linalg.cholesky(A)
    assert np.array_equal(L, L0), kh.chol_mismatches(L, A, L0)[:3]


def test_float32_route_equals_float64_route():
    L0a, Aa = kh.int_chol_case(1024, seed=5, span=3, f32=True)
    L0b, Ab = kh.int_chol_case(1024, seed=5, span=3, f32=False)
    assert np.array_equal(L0a, L0b) and np.array_equal(Aa, Ab)


def test_integer_sweeps_are_exact_on_the_host():
    """alpha == a0 and X == X0 by plain substitution: what part D asks of the device."""
    n = 640
    L0, A = kh.int_chol_case(n, seed=3)
    rng = np.random.default_rng(4)
    a0 = rng.integers(-3, 4, n).astype(float)
    assert np.array_equal(kh.solve_spd(L0, A @ a0), a0)
    X0 = rng.integers(-1, 2, (129, n)).astype(float)
    assert np.array_equal(kh.substitute_rows(L0, X0 @ L0.T), X0)
    # the inverse of a 512-wide diagonal block of L0 (what the many-right-hand-side solve multiplies by) is an integer
    # matrix far below 2^53
    W = kh.substitute_rows(L0[:512, :512], np.eye(512)).T
    assert np.array_equal(W, np.round(W)) and np.abs(W).max() < 2.0 ** 40
    assert np.array_equal(W @ L0[:512, :512], np.eye(512))


# ---- the exact K^-1 cases (int_nilpotent_chol_case) and the exact Z = Q K^-1 cases
@pytest.mark.parametrize("n,groups", kh.NILPOTENT_CASES, ids=[f"n{n}" for n, _ in kh.NILPOTENT_CASES])
def test_nilpotent_factor_and_its_inverse_are_exact(n, groups):
    """L0 W == I and A == L0 L0^T hold exactly, W and K^-1 are integer matrices inside the asserted bound, and LAPACK
    and the plain substitutions reproduce L0, W^T, W^T W and Z0 bit for bit: what parts F and G ask of the device."""
    L0, W, A = kh.int_nilpotent_chol_case(groups, kh.NILPOTENT_SEED, n)
    I = np.eye(n)
    assert L0.shape == W.shape == A.shape == (n, n)
    assert np.array_equal(L0 @ W, I) and np.array_equal(W @ L0, I)
    assert np.array_equal(A, L0 @ L0.T) and np.array_equal(A, A.T)
    assert np.array_equal(W, np.round(W)) and np.array_equal(W, np.tril(W)) and np.array_equal(np.diag(W), np.ones(n))
    for s in range(0, n, kh.TILE):  # identity diagonal tiles
        assert np.array_equal(L0[s:s + kh.TILE, s:s + kh.TILE], np.eye(min(kh.TILE, n - s)))
    iK = W.T @ W
    assert np.array_equal(iK, np.round(iK)) and n * np.abs(W).max() ** 2 < 2.0 ** 53
    # the inverse is not trivial: entries beyond {-1, 0, 1} (products of blocks), and of its 512-wide diagonal blocks of
    # more than one tile (what build_inv2 forms) at most the first is the identity (n = 2176: its group has five tiles)
    assert np.abs(W).max() > 1
    dense = [np.count_nonzero(W[s:s + 512, s:s + 512]) > 512 + 1000 for s in range(0, n - kh.TILE, 512)]
    assert all(dense[1:]) and (dense[0] or n == 2176)
    if n == 384:  # the same in integer arithmetic
        Li, Wi = L0.astype(np.int64), W.astype(np.int64)
        assert np.array_equal(Li @ Wi, np.eye(n, dtype=np.int64))
        assert np.array_equal(Li @ Li.T, A.astype(np.int64)) and np.array_equal(Wi.T @ Wi, iK.astype(np.int64))
    assert np.array_equal(np.linalg.cholesky(A), L0)
    if n <= 1024:  # (the plain substitutions are O(n) NumPy calls of O(n^2) each)
        assert np.array_equal(kh.substitute_rows(L0, I), W.T)
        assert np.array_equal(kh.inverse_spd(L0), iK)
        Z0, Q = kh.rows_kinv_case(A, 5, seed=n)
        assert np.array_equal(kh.substitute_back_rows(L0, kh.substitute_rows(L0, Q)), Z0)
    a0 = np.random.default_rng(n + 1).integers(-3, 4, n).astype(float)
    assert np.array_equal(iK @ (A @ a0), a0)


def test_nilpotent_case_cut_is_the_leading_part():
    L0, W, A = kh.int_nilpotent_chol_case((3, 3, 2), kh.NILPOTENT_SEED)
    L1, W1, A1 = kh.int_nilpotent_chol_case((3, 3, 2), kh.NILPOTENT_SEED, 900)
    assert np.array_equal(L1, L0[:900, :900]) and np.array_equal(W1, W[:900, :900]) and np.array_equal(A1, A[:900, :900])


def test_nilpotent_builder_refuses_a_partition_beyond_2_to_53():
    with pytest.raises(AssertionError, match="not below 2\\^53"):
        kh.int_nilpotent_chol_case((2, 2, 2, 2, 2, 2), kh.NILPOTENT_SEED)


def test_tile_report_names_a_wrong_entry_of_the_inverse():
    L0, W, A = kh.int_nilpotent_chol_case((1, 1, 1), kh.NILPOTENT_SEED)
    iK = W.T @ W
    assert kh._tile_report(iK != iK.copy(), "differ from W^T W") == []
    bad = iK.copy()
    bad[300, 140] += 1.0
    msgs = kh._tile_report(bad != iK, "differ from W^T W", bad, iK)
    assert len(msgs) == 1 and msgs[0].startswith("tile (2, 1): 1 entries differ from W^T W") and "[300, 140]" in msgs[0], msgs


@pytest.mark.parametrize("n,m", kh.ROWS_KINV_CASES[:-1], ids=[f"n{n}-m{m}" for n, m in kh.ROWS_KINV_CASES[:-1]])
def test_rows_kinv_case_meets_its_condition(n, m):
    """Q = Z0 A of part G stays inside the condition rows_kinv_case asserts, and the two plain substitutions return Z0
    (on a few of the rows: they are O(n) NumPy calls each)."""
    L0, A = kh.int_chol_case(n, seed=n + 9)
    Z0, Q = kh.rows_kinv_case(A, m, seed=n + 37 * m)
    assert np.array_equal(Q, np.round(Q))
    rows = slice(0, min(m, 3))
    assert np.array_equal(kh.substitute_back_rows(L0, kh.substitute_rows(L0, Q[rows])), Z0[rows])


@needs_longdouble
@pytest.mark.parametrize("n,groups", [c for c in kh.NILPOTENT_CASES if c[0] <= 1024],
                         ids=[f"n{n}" for n, _ in kh.NILPOTENT_CASES if n <= 1024])
def test_plain_numpy_meets_the_leave_one_out_caps(n, groups):
    """p = K^-1 c1 and W = K^-1 diag(c2) K^-1 evaluated in plain fp64 NumPy from the exact K^-1, in the order of
    operations of the device (c1 = alpha (1 / d), G = K^-1 diag(sqrt c2), W = G G^T), meet cap_loo_p and cap_loo_w; a
    relative perturbation of 1e-10 in one entry does not."""
    L0, W, A = kh.int_nilpotent_chol_case(groups, kh.NILPOTENT_SEED, n)
    iK = W.T @ W
    a0 = np.random.default_rng(n + 1).integers(-3, 4, n).astype(float)
    d = np.diag(iK).copy()
    var = 1.0 / d
    p = iK @ (a0 * var)
    G = iK * np.sqrt(0.5 * var * (1.0 + var * a0 * a0))
    Wm = G @ G.T
    rho_p, rho_w = kh.rho_loo_p(p, iK, a0, d), kh.rho_loo_w(Wm, iK, a0, d)
    print(f"\nreference n={n}: rho_loo_p {rho_p:.2f} (cap {kh.cap_loo_p(n)}), rho_loo_w {rho_w:.2f} (cap {kh.cap_loo_w(n)})")
    assert rho_p <= kh.cap_loo_p(n) and rho_w <= kh.cap_loo_w(n)
    p2, W2 = p.copy(), Wm.copy()
    i = int(np.argmax(np.abs(p)))
    p2[i] *= 1 + 1e-10
    W2[0, 0] *= 1 + 1e-10
    assert kh.rho_loo_p(p2, iK, a0, d) > 1e3 and kh.rho_loo_w(W2, iK, a0, d) > 1e3


def test_builders_are_deterministic():
    a, b = kh.int_gemm_case(256, 128, 48, 160, 80, 176, 1, seed=9), kh.int_gemm_case(256, 128, 48, 160, 80, 176, 1, seed=9)
    for key in ("C0", "A", "B", "E"):
        assert np.array_equal(a[key], b[key])
    assert not np.array_equal(a["E"], kh.int_gemm_case(256, 128, 48, 160, 80, 176, 1, seed=10)["E"])
    assert np.abs(a["A"][:, :48]).max() == 4 and np.abs(a["C0"][:, :128]).max() <= 2 ** 20
    assert (a["C0"][:, 128:] == kh.C_PAD).all() and (a["A"][:, 48:] == kh.OPERAND_PAD).all()
    for x, y in zip(kh.int_chol_case(300, 2, 3), kh.int_chol_case(300, 2, 3)):
        assert np.array_equal(x, y)
    for x, y in zip(kh.float_gemm_case(128, 128, 32, 1), kh.float_gemm_case(128, 128, 32, 1)):
        assert np.array_equal(x, y)
    for kind in ("well", "graded", "gp"):
        assert np.array_equal(kh.spd_case(129, kind, 7), kh.spd_case(129, kind, 7))
        assert not np.array_equal(kh.spd_case(129, kind, 7), kh.spd_case(129, kind, 8))
    assert np.array_equal(kh.check_rows(1152, 3), kh.check_rows(1152, 3))
    rows = set(kh.check_rows(1152).tolist())
    assert {0, 127, 128, 129, 1023, 1024, 1025, 1151} <= rows and len(rows) <= 2 + 3 * 8 + 32
    assert np.array_equal(kh.check_rows(640), np.arange(640))


@pytest.mark.parametrize("m", [1, 2, 8, 9, 17, 32, 41, 48, 52, 56, 60])
def test_flow_flops_formula_equals_the_shipped_task_lists(m):
    """kernel_host.flow_update_flops (the look-ahead witness of tests/test_kernels_gpu.py) against the task lists the
    library ships for a tail of m tile rows, counted task by task; the count does not depend on how many workgroups
    the lists are dealt to, and tails of 48, 52 and 56 rows and whole matrices of 56 and 60 book different amounts."""
    import ctypes as C

    from inference_amd import _lib

    lib = _lib.load()
    for nwg in (448, 64):
        cnt = C.c_int64(0)
        assert lib.gpmi_flow_task_lists(m, nwg, 0, None, C.byref(cnt)) == 0
        tasks = np.zeros((max(cnt.value, 1), 8), dtype=np.int32)
        tasks[:, 0] = -1
        assert lib.gpmi_flow_task_lists(m, nwg, cnt.value, tasks.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(cnt)) == 0
        assert kh.flow_update_flops_of_lists(tasks[:cnt.value]) == kh.flow_update_flops(m)
    assert kh.flow_update_flops(48) == 18106.75 * 2.0 * 128 ** 3
    assert len({kh.flow_update_flops(k) for k in (41, 44, 48, 52, 56, 60)}) == 6


# ---- sensitivity of the comparison helpers: a host result that is wrong in one place must fail and name the tile
@pytest.mark.parametrize("lower", [0, 1])
def test_gemm_comparison_names_a_wrong_subtile(lower):
    case = kh.int_gemm_case(384, 256, 128, 256 + 32, 128, 128 + 32, lower, seed=1)
    good = case["C0"].copy()
    good[:, :256] = case["E"]
    if lower:  # the strictly-upper tile keeps the upload
        good[:128, 128:256] = case["C0"][:128, 128:256]
    assert kh.gemm_mismatches(good, case) == []
    E_wrong = case["E"].copy()
    E_wrong[256 + 64:384, 128:128 + 64] += 1.0  # one 64 x 64 sub-tile of the expected C off by 1
    msgs = kh.gemm_mismatches(good, case, E_wrong)
    assert len(msgs) == 1 and msgs[0].startswith("tile (2, 1): 4096 entries") and "[(1, 0)]" in msgs[0], msgs
    one = good.copy()
    one[129, 1] += 1.0  # one entry
    msgs = kh.gemm_mismatches(one, case)
    assert len(msgs) == 1 and msgs[0].startswith("tile (1, 0): 1 entries") and "[129, 1]" in msgs[0], msgs
    pad = good.copy()
    pad[200, 256 + 3] = 0.0
    assert any(m.startswith("padding: 1 entries changed, first at [200, 259]") for m in kh.gemm_mismatches(pad, case))


def test_gemm_comparison_lower_rules():
    case = kh.int_gemm_case(256, 256, 128, 256, 128, 128, 1, seed=2)
    good = case["C0"].copy()
    tril = np.tril(np.ones((256, 256), bool))
    good[tril] = case["E"][tril]
    assert kh.gemm_mismatches(good, case) == []  # above the diagonal of a diagonal tile: the original is accepted
    upd = good.copy()
    upd[:128, :128] = case["E"][:128, :128]
    assert kh.gemm_mismatches(upd, case) == []   # ... and so is the updated value
    bad = good.copy()
    bad[3, 100] += 1.0                           # ... but nothing else
    msgs = kh.gemm_mismatches(bad, case)
    assert len(msgs) == 1 and msgs[0].startswith("tile (0, 0)") and "neither original nor updated" in msgs[0], msgs
    up = good.copy()
    up[5, 200] = case["E"][5, 200]               # a strictly-upper tile must not be touched
    msgs = kh.gemm_mismatches(up, case)
    assert len(msgs) == 1 and msgs[0].startswith("tile (0, 1)") and "strictly-upper" in msgs[0], msgs


def test_chol_comparison_names_a_wrong_entry():
    n, ld = 384, 384 + 32
    L0, A = kh.int_chol_case(n, seed=6, span=3)
    buf0 = kh.pad_identity(A, ld)
    good = buf0.copy()
    tril = np.tril(np.ones((n, n), bool))
    good[:, :n][tril] = L0[tril]
    good[130, 200] = 77.0  # above the diagonal inside diagonal tile (1, 1): workspace
    assert kh.chol_mismatches(good, buf0, L0) == []
    L_wrong = L0.copy()
    L_wrong[300, 140] += 1.0  # one entry of L0 off by 1
    msgs = kh.chol_mismatches(good, buf0, L_wrong)
    assert len(msgs) == 1 and msgs[0].startswith("tile (2, 1): 1 entries differ from L0") and "[300, 140]" in msgs[0], msgs
    for (r, c), where in (((3, 100), "tile (0, 0)"), ((10, 300), "tile (0, 2)")):
        bad = good.copy()
        bad[r, c] += 1.0
        msgs = kh.chol_mismatches(bad, buf0, L0)
        assert len(msgs) == 1 and msgs[0].startswith(where) and "above the factor changed" in msgs[0], msgs
    bad = good.copy()
    bad[130, 200] = np.nan
    assert any("not finite" in m for m in kh.chol_mismatches(bad, buf0, L0))
    bad = good.copy()
    bad[7, n + 1] = 1.0
    assert any(m.startswith("padding") for m in kh.chol_mismatches(bad, buf0, L0))


# ---- the caps of part E hold for the plain references with kappa = 0
@needs_longdouble
@pytest.mark.parametrize("kind", ["well", "graded", "gp"])
@pytest.mark.parametrize("n", [129, 640, 1152])
def test_references_meet_the_caps_with_kappa_zero(n, kind):
    A = kh.spd_case(n, kind, seed=n)
    L = np.linalg.cholesky(A)
    rng = np.random.default_rng(n + 1)
    rho = kh.rho_chol(A, L)
    Q = rng.standard_normal((129, n))
    X = kh.substitute_rows(L, Q)
    rho_x = kh.rho_solve_rows(X, L, Q)
    r = rng.standard_normal(n)
    alpha = kh.solve_spd(L, r)
    rho_a = kh.rho_solve(A, alpha, r)
    res = kh.inverse_residual(A, kh.inverse_spd(L))
    cond = float(np.linalg.cond(A, 2))
    print(f"\nreference n={n} {kind}: rho_chol {rho:.2f} (cap {kh.cap_chol(n)}), rho_solve_rows {rho_x:.2f} "
          f"(cap {kh.cap_solve_rows(n)}), rho_alpha {rho_a:.2f} (cap {kh.cap_alpha(n)}), |A iK - I| {res:.2e} "
          f"(cap {kh.cap_inverse(n, cond):.2e}, cond {cond:.2e}), kappa_128 {kh.kappa_blocks(L, 128):.2e}, "
          f"kappa_512 {kh.kappa_blocks(L, 512):.2e}")
    assert rho <= kh.cap_chol(n)
    assert rho_x <= kh.cap_solve_rows(n)
    assert rho_a <= kh.cap_alpha(n)
    assert res <= kh.cap_inverse(n, cond)


@needs_longdouble
def test_float_gemm_reference_meets_its_cap():
    """A plain fp64 product meets rho_gemm <= k + 2 (the bound for any summation order, with or without FMA), and a
    product rounded to float32 does not: the case catches a reduced-precision multiply the integer cases cannot."""
    m, n, k = 128, 128, 144
    C, A, B = kh.float_gemm_case(m, n, k, seed=3)
    assert kh.rho_gemm(C - A @ B.T, C, A, B) <= k + 2
    low = C - (A.astype(np.float32) @ B.astype(np.float32).T).astype(np.float64)
    assert kh.rho_gemm(low, C, A, B) > 1e6


def test_ratio_helpers_detect_a_perturbation():
    n = 129
    A = kh.spd_case(n, "well", 1)
    L = np.linalg.cholesky(A)
    assert kh.kappa_blocks(np.eye(n), 128) == 1.0 and kh.kappa_blocks(L, 128) >= 1.0
    if kh.LONGDOUBLE_OK:
        base = kh.rho_chol(A, L)
        L2 = L.copy()
        L2[100, 50] *= 1 + 1e-10
        assert kh.rho_chol(A, L2) > 1e3 > base
