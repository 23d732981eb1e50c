"""CPU checks behind tests/test_sparse_scale_gpu.py: the schedule queries gpmi_sgp_schedule / gpmi_select_schedule against
the branches the scale cases are named after (and the neighbouring shapes that must fall on the other side), their
argument errors, the golden fixture tests/golden/sparse_scale.npz (inputs regenerate bit for bit; the conditions its maker
asserts hold in the stored numbers), and the mirror itself at m_pad > 256 (tiles3) against the dense definition and a
fourth-order finite difference.  No device call is made: the two queries are host arithmetic.

Bounds of the two mirror checks (tiles3: |F| = 1.7e2, cond(K_mm + eps I) = 1.1e3, max |dF/dtheta| = 7.4e2, max |dF/dZ| = 3e2):
  dense definition   the N x N route solves with K_mm and factorises Q + Sigma: cond x 2^-52 x |F| x a few hundred sums
                     ~ 1e-13 x cond x |F| = 1.8e-8 allowed; measured 1.8e-11
  finite difference  fourth order at h = 1e-3 (theta) and 1e-4 length scales (Z): truncation h^4 / 30 x |d^5 F| and
                     rounding 2^-52 |F| / h; with the fifth derivative bounded by 1e3 x the gradient, 1e-12 x 1e3 / 30 of it
                     -> 1e-7 x the largest gradient component allowed; measured 3.9e-8 on 7.4e2 (theta, ln s, mean) and
                     8.8e-7 on 3e2 (Z: rounding 2^-52 x 1.7e2 / 5e-6 = 8e-9 per evaluation, four of them weighted 8 / 12)
"""
import ctypes as C

import numpy as np
import pytest

import sparse_host as sh
import sparse_z_host as szh

GPMI_OK, GPMI_ERR_ARG = 0, -1
QUANTITIES = ("F", "grad", "gz", "alpha", "mean", "var")  # the order of <case>/allow in the fixture
RUN_TILES = {"run4": 4, "run8": 8, "run16": 16, "max_m": 8}  # what the fixture's maker assumed


def schedule(n, m, panel):
    from inference_amd._engine import sgp_schedule

    return sgp_schedule(n, m, panel)


@pytest.mark.parametrize("name", sh.SCALE_NAMES)
def test_every_case_is_on_its_branch_and_its_neighbour_is_not(name):
    kind, n, d, m, panel, white, ell = sh.SCALE_CASES[name]
    want, neighbour, other = sh.SCALE_SCHEDULE[name]
    got = schedule(n, m, panel)
    assert {k: got[k] for k in want} == want, got
    near = schedule(*neighbour)
    assert {k: near[k] for k in other} == other, near
    if name in RUN_TILES:
        assert got["kmm_run_tiles" if name == "max_m" else "data_run_tiles"] == RUN_TILES[name]
    if name == "long":  # 1024 workgroups of 256 threads: the second trip of the grid-stride loop starts at row 262144
        assert n > 256 * got["weight_blocks"] and neighbour[0] == 256 * near["weight_blocks"]
        assert n - (got["panels"] - 1) * got["panel"] == 300
    if name == "tiles3":
        assert n - 2 * got["panel"] == 188 and got["m_pad"] // 128 == 3
    if name == "bench_like":
        assert n - 2 * got["panel"] == 1


def test_the_table_of_run_lengths():
    """zrun_tiles: 16, halved (not below 2) while (columns / 64) x ceil(rows / 64 / r) < 512."""
    def rule(rows, cols):
        r = 16
        while r > 2 and (cols // 64) * -(-(rows // 64) // r) < 512:
            r //= 2
        return r

    assert schedule(32700, 128, 32768)["data_run_tiles"] == 2  # m_pad = 128 at the largest panel
    assert [schedule(32700, m, 32768)["data_run_tiles"] for m in (129, 256, 385, 512, 897, 1024)] == [4, 4, 8, 8, 16, 16]
    assert [schedule(32700, m, 8192)["data_run_tiles"] for m in (200, 450, 1000)] == [2, 2, 4]  # the cross-check's shorter runs
    assert [schedule(300, m, 0)["kmm_run_tiles"] for m in (2816, 2817, 3968, 3969, 4096)] == [2, 4, 4, 8, 8]
    for m in range(64, 4097, 64):
        for n, panel in ((300, 0), (5000, 1024), (32700, 8192), (32700, 16384), (40000, 32768)):
            s = schedule(n, m, panel)
            assert s["m_pad"] == -(-m // 128) * 128 and s["panel"] == min(-(-(panel or 8192) // 128) * 128, -(-n // 128) * 128)
            assert s["data_run_tiles"] == rule(s["panel"], s["m_pad"]) and s["kmm_run_tiles"] == rule(s["m_pad"], s["m_pad"])
            assert s["panels"] == -(-n // s["panel"]) and s["weight_blocks"] == min(1024, -(-n // 256))
    assert schedule(262144, 5, 0)["weight_blocks"] == 1024 and schedule(262143, 5, 0)["weight_blocks"] == 1024
    assert schedule(261888, 5, 0)["weight_blocks"] == 1023
    assert schedule(10**6, 5, 0)["weight_blocks"] == 1024 and schedule(10**6, 5, 0)["panels"] == 123
    assert schedule(300, 5, 32768)["panel"] == 384  # (at most all of x, in whole tiles)
    assert schedule(100000, 5, 100)["panel"] == 128 and schedule(100000, 5, 32768)["panels"] == 4


def test_select_schedule():
    from inference_amd._engine import select_schedule

    assert select_schedule(sh.SELECT_N) == 258 and select_schedule(sh.SELECT_N + sh.SELECT_EXTRA) == 261
    assert select_schedule(65536) == 256 and select_schedule(65537) == 257  # one partial per thread up to 65536 points
    assert select_schedule(2800) == 11 and select_schedule(1) == 1
    for bad in (0, -1, 2**30 + 1):
        with pytest.raises(ValueError):
            select_schedule(bad)


def test_argument_errors_of_the_queries():
    from inference_amd import _lib
    from inference_amd._engine import sgp_schedule

    lib = _lib.load()
    out = (C.c_int64 * 6)(*([-7] * 6))
    one = (C.c_int64 * 1)(-7)
    limits = [(2, 1, 0), (2**30, _lib.SGP_MAX_M, 32768)]
    for n, m, panel in limits:
        assert lib.gpmi_sgp_schedule(n, m, panel, out) == GPMI_OK
    assert list(out) == [32768, 4096, 16, 8, 1024, 32768]
    out = (C.c_int64 * 6)(*([-7] * 6))
    for n, m, panel in ((1, 5, 0), (2**30 + 1, 5, 0), (300, 0, 0), (300, _lib.SGP_MAX_M + 1, 0), (300, 5, -1), (300, 5, 32769)):
        assert lib.gpmi_sgp_schedule(n, m, panel, out) == GPMI_ERR_ARG, (n, m, panel)
        assert list(out) == [-7] * 6
        with pytest.raises(ValueError):
            sgp_schedule(n, m, panel)
    assert lib.gpmi_sgp_schedule(300, 5, 0, None) == GPMI_ERR_ARG
    assert lib.gpmi_select_schedule(300, None) == GPMI_ERR_ARG
    for n in (0, 2**30 + 1):
        assert lib.gpmi_select_schedule(n, one) == GPMI_ERR_ARG and one[0] == -7
    assert lib.gpmi_select_schedule(2**30, one) == GPMI_OK and one[0] == 2**22


@pytest.mark.parametrize("name", sh.SCALE_NAMES)
def test_fixture_inputs_regenerate_bit_for_bit(golden, name):
    g = golden("sparse_scale")
    case = sh.scale_case(name)
    kind, n, d, m, panel, white, ell = sh.SCALE_CASES[name]
    assert case["x"].shape == (n, d) and case["z"].shape == (m, d) and case["e"] is not None and case["panel"] == panel
    assert np.array_equal(g[f"{name}/x_ends"], case["x"][[0, -1]])
    assert np.array_equal(g[f"{name}/z_ends"], case["z"][[0, -1]])
    assert g[f"{name}/gz"].shape == (m, d) and g[f"{name}/grad"].shape == (len(sh.full_theta(case)),)
    assert g[f"{name}/alpha"].shape == g[f"{name}/alpha_idx"].shape == (min(512, n),) and g[f"{name}/alpha_idx"].max() < n
    assert g[f"{name}/mean"].shape == g[f"{name}/var"].shape == (17,)


@pytest.mark.parametrize("name", sh.SCALE_NAMES)
def test_fixture_holds_the_makers_conditions(golden, name):
    g = golden("sparse_scale")
    allow = dict(zip(QUANTITIES, g[f"{name}/allow"]))
    spread = dict(zip(QUANTITIES, g[f"{name}/spread"]))
    ripples, cond = int(g[f"{name}/ripples"]), float(g[f"{name}/cond"])
    assert ripples == (8 if name == "run16" else 6 if name == "max_m" else sh.N_RIPPLES)
    print(f"{name}: cond {cond:.3g}, {ripples} ripples, allowances " + ", ".join(f"{k} {allow[k]:.2e}" for k in QUANTITIES))
    # the allowance rule from the stored spreads and scales
    scale = dict(F=abs(g[f"{name}/F"][0]), grad=np.abs(g[f"{name}/grad"]).max(), gz=np.abs(g[f"{name}/gz"]).max(),
                 mean=np.abs(g[f"{name}/mean"]).max(), var=float(np.exp(2.0 * 0.1)))
    for k, s in scale.items():
        assert allow[k] == max(10.0 * spread[k], 1e-10 * s), k
    assert allow["alpha"] >= max(10.0 * spread["alpha"], 1e-10 * np.abs(g[f"{name}/alpha"]).max())
    if name == "bench_like":
        assert cond > 1e5  # the ill-conditioned regime, recorded and not bounded
    else:
        assert cond <= 1e4
    if name in RUN_TILES:
        part = g[f"{name}/later_tiles_part"]
        assert part.shape == (-(-sh.SCALE_CASES[name][3] // 64),)
        print(f"  dF/dZ from the later tiles of a run: smallest tile maximum {part.min():.3e} against {allow['gz']:.3e}")
        assert part.min() > 1e3 * allow["gz"]
    if name == "long":
        moves, floors = g["long/tail_moves"], g["long/tail_allow"]
        print("  rows >= 262144 move F, sum w and the noise gradient by", moves, "against", floors)
        assert (moves > 1e3 * floors).all()
        case = sh.scale_case("long")  # (sum w over the tail is cheap to recompute)
        assert moves[1] == (1.0 / (case["e"][262144:] ** 2 + case["white"])).sum()


def test_fixture_selection_conditions(golden):
    g = golden("sparse_scale")
    x, theta, w = sh.select_case()
    assert x.shape == (sh.SELECT_N, 2) and np.array_equal(g["select/x_ends"], x[[0, -1]])
    for label in ("weighted", "unweighted"):
        index, margin, pv = g[f"select/{label}_index"], g[f"select/{label}_margin"], g[f"select/{label}_pivot_var"]
        assert len(index) == len(set(index.tolist())) == sh.SELECT_M and g[f"select/{label}_trace"].shape == (sh.SELECT_M + 1,)
        deviation = (sh.SELECT_M + 2 + 40) * 2.0**-53 / pv.min()
        print(f"selection {label}: smallest margin {margin[1:].min():.2e}, smallest pivot variance {pv.min():.3f}, "
              f"deviation bound {deviation:.1e}")
        assert margin[1:].min() >= 1e-9 and pv.min() >= 1e-2 and 1e4 * deviation <= margin[1:].min()
    assert g["select/unweighted_index"][0] == 0  # (a tie of ones: row 0)


def test_tiles3_mirror_against_the_dense_definition_and_finite_differences(golden):
    """The mirror at m_pad = 384: the fixture's F is the dense definition's, the analytic gradients are the differences'."""
    g = golden("sparse_scale")
    case = sh.scale_case("tiles3")
    mir = sh.SparseMirror(case["kind"], case["x"], case["z"])
    theta, white, r, nv = case["theta"], case["white"], case["y"] - sh.MU, case["e"] ** 2
    base = szh.all_quantities(case, mir)
    for k in ("F", "grad", "gz", "mean", "var"):  # the fixture is this mirror's output (not bit for bit across BLAS builds)
        assert np.abs(base[k] - g[f"tiles3/{k}"]).max() <= dict(zip(QUANTITIES, g["tiles3/allow"]))[k], k
    F, cond = base["F"][0], mir.cond_kmm(theta)
    dense = mir.dense_bound(theta, white, r, nv)
    print(f"tiles3: cond {cond:.3g}  F {F:.6f}  |F - dense| {abs(F - dense):.3g}")
    assert abs(F - dense) <= 1e-13 * cond * abs(F)
    fd = sh.fd4(lambda t: mir.bound(t, white, r, nv), theta)
    fd_s = sh.fd4(lambda t: mir.bound(theta, float(np.exp(2.0 * t[0])), r, nv), [0.5 * np.log(white)])[0]
    fd_mu = sh.fd4(lambda t: mir.bound(theta, white, r - t[0], nv), [0.0])[0]
    err = np.abs(np.concatenate([[fd_mu], fd, [fd_s]]) - base["grad"]).max()
    print(f"tiles3: max |gradient| {np.abs(base['grad']).max():.4g}  |analytic - fd| {err:.3g}")
    assert err <= 1e-7 * np.abs(base["grad"]).max()
    # dF/dZ at the three inducing points with the largest gradient, one per 128-row tile of Z, both coordinates
    d = case["z"].shape[1]
    f_of_z = szh.bound_of_z(case["kind"], case["x"], theta, white, r, nv)
    z0 = case["z"].ravel()
    for tile in range(3):
        i = 128 * tile + int(np.abs(base["gz"][128 * tile:128 * (tile + 1)]).max(axis=1).argmax())
        for k in range(d):
            e = np.zeros(z0.size)
            e[i * d + k] = 1e-4 * 0.05  # (a step of 1e-4 length scales)
            fdz = (-f_of_z(z0 + 2 * e) + 8.0 * f_of_z(z0 + e) - 8.0 * f_of_z(z0 - e) + f_of_z(z0 - 2 * e)) / (12.0 * e[i * d + k])
            print(f"tiles3: dF/dz[{i}][{k}] {base['gz'][i, k]:.6g}  |analytic - fd| {abs(fdz - base['gz'][i, k]):.3g}")
            assert abs(fdz - base["gz"][i, k]) <= 1e-7 * np.abs(base["gz"]).max()
