"""CPU-only checks behind the lockstep batches of the sparse model: the schedule gpmi_sgp_bound_batch runs
(gpmi_sgp_batch_schedule is host code: no device call), and the conditions on the fixtures of tests/sparse_batch_host.py
that keep the comparisons of tests/test_sparse_batch_gpu.py honest, asserted on the NumPy mirror."""
import numpy as np
import pytest

import sparse_batch_host as bh
import sparse_host as sh
from inference_amd._engine import sgp_batch_schedule, sgp_schedule

GIB = 1 << 30


def test_chunk_is_the_batch_where_the_budget_allows():
    for want_grad in (False, True):
        s = sgp_batch_schedule(300, 33, 3, 7, panel_rows=128, want_grad=want_grad)
        assert (s["chunk"], s["chunks"]) == (7, 1)
    # the library's own budget (24 GiB unless GPMI_BATCH_GIB says otherwise) against an explicit one
    big = sgp_batch_schedule(100000, 512, 8, 64, want_grad=True, budget_bytes=24 * GIB)
    assert big["chunk"] == min(64, 24 * GIB // big["bytes_per_problem"]) and big["chunks"] == -(-64 // big["chunk"])
    assert sgp_batch_schedule(100000, 512, 8, 64, want_grad=True, budget_bytes=200 * GIB)["chunk"] == 64


def test_max_chunk_is_respected():
    assert [sgp_batch_schedule(300, 33, 3, 7, panel_rows=128, max_chunk=k)["chunks"] for k in (0, 1, 3, 7, 9)] == [1, 7, 3, 1, 1]
    s = sgp_batch_schedule(300, 33, 3, 7, panel_rows=128, max_chunk=3)
    assert s["chunk"] == 3
    assert sgp_batch_schedule(300, 33, 3, 5000)["chunk"] == 1024  # (the most problems one launch carries)


def test_a_budget_below_one_problem_gives_chunks_of_one():
    s = sgp_batch_schedule(300, 33, 3, 7, panel_rows=128, budget_bytes=1)
    assert (s["chunk"], s["chunks"]) == (1, 7)
    per = s["bytes_per_problem"]
    assert sgp_batch_schedule(300, 33, 3, 7, panel_rows=128, budget_bytes=3 * per + per // 2)["chunk"] == 3
    assert sgp_batch_schedule(300, 33, 3, 7, panel_rows=128, budget_bytes=per - 1)["chunk"] == 1


def test_bytes_per_problem_follow_the_documented_formula():
    """include/gpmi.h: doubles per problem and the parameters (KParams: two ints, three doubles, 64 inverse squares; two
    info words)."""
    for n, m, d, panel in ((300, 33, 3, 128), (2100, 130, 2, 512), (100000, 512, 8, 0), (70, 129, 1, 0)):
        single = sgp_schedule(n, m, panel)
        P, mp = single["panel"], single["m_pad"]
        ld = mp + 32
        doubles = 9 * mp * ld + 256 * mp + 4 * mp + 3 * P + 128 + 4096 + 3 * max(mp * (P + 32), P * ld) + 2 * n + 2
        fixed = 8 + 3 * 8 + 64 * 8 + 2 * 4
        assert sgp_batch_schedule(n, m, d, 1, panel_rows=panel)["bytes_per_problem"] == 8 * doubles + fixed
        doubles += n + max(P, mp) * mp * (d + 2) // 4096
        assert sgp_batch_schedule(n, m, d, 1, panel_rows=panel, want_grad=True)["bytes_per_problem"] == 8 * doubles + fixed


def test_panels_are_those_of_the_single_evaluation():
    for n, m, panel in ((300, 33, 128), (2100, 130, 512), (257, 64, 0), (70, 129, 0), (16385, 512, 0), (262444, 5, 0)):
        single, batch = sgp_schedule(n, m, panel), sgp_batch_schedule(n, m, 2, 3, panel_rows=panel)
        assert (batch["panel"], batch["panels"], batch["m_pad"]) == (single["panel"], single["panels"], single["m_pad"])


@pytest.mark.parametrize("kwargs", [dict(n=1), dict(m=0), dict(m=4097), dict(d=0), dict(d=65), dict(panel_rows=-1),
                                    dict(panel_rows=32769), dict(T=-1), dict(max_chunk=-1), dict(budget_bytes=-1)])
def test_argument_ranges(kwargs):
    args = dict(n=300, m=33, d=3, T=7)
    args.update(kwargs)
    with pytest.raises(ValueError):
        sgp_batch_schedule(**args)


def test_an_empty_batch_has_no_chunks():
    assert sgp_batch_schedule(300, 33, 3, 0)["chunks"] == 0


@pytest.mark.parametrize("number", bh.BATCH_CASES)
def test_row_sets_are_well_conditioned(number):
    """cond(K_mm + eps I) <= 1e4 for every row: the device's error then stays inside allowances sized by 1e-13 ripples."""
    case = sh.case(number)
    rows = bh.row_set(case)
    assert rows.shape == (bh.N_ROWS, len(sh.full_theta(case))) and np.array_equal(rows[0], sh.full_theta(case))
    assert (np.abs(rows[1:, 1:] - rows[0, 1:]) <= 0.3).all() and (np.abs(rows[1:, 1:] - rows[0, 1:]) > 0.0).all()
    assert set(np.round(rows[:, 0] - sh.MU, 12)) <= {-0.5, 0.0, 0.5}
    cond = bh.cond_rows(case, rows)
    print(f"case {number}: largest cond(K_mm + eps I) of the row set {cond.max():.3e}")
    assert (cond <= 1e4).all(), cond


def test_the_failure_fixture_fails_in_one_row_only():
    """jitter 0: the four regular rows factorise in NumPy at cond(K_mm) <= 1e6; the failing row's K_mm is the all-ones
    matrix exactly, whose second pivot is exactly 0."""
    case = sh.case(1)
    rows = bh.failure_rows(case)
    assert rows.shape[0] == bh.FAIL_ROWS and np.array_equal(rows[bh.FAIL_POSITION], bh.failing_row(case))
    mir = sh.SparseMirror(case["kind"], case["x"], case["z"], jitter=0.0)
    for t, row in enumerate(rows):
        mu, theta, white = bh.split_row(case, row)
        if t == bh.FAIL_POSITION:
            K = mir._matrices(theta)[1]
            assert np.array_equal(K, np.ones_like(K))
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(K)
            with pytest.raises(np.linalg.LinAlgError):
                mir.bound(theta, white, case["y"] - mu, bh.noise_var(case))
        else:
            assert mir.cond_kmm(theta) <= 1e6
            assert np.isfinite(mir.bound(theta, white, case["y"] - mu, bh.noise_var(case)))
