"""
CPU tests of the posterior-draw generator (include/gpmi.h: gpmi_draws_normals and the argument checks of
gpmi_posterior_draws / gpmi_mvn_draws): the NumPy mirror of tests/draws_host.py against the published Philox4x32-10 known
answers, the library's host entry point against the mirror, the stream's independence of where a call starts, and its
moments.  No device call is made.
"""
import ctypes as C

import numpy as np
import pytest

import draws_host as dh

ERR_ARG = -1
SEEDS = (0, -1, 0x0123456789ABCDEF)
HIGH = 2**32 + 3  # a first draw in the counter's high word


@pytest.fixture(scope="module")
def lib():
    from inference_amd import _lib

    return _lib.load()


def lib_normals(lib, seed, first_draw, n, m):
    from inference_amd._engine import _seed_i64

    z = np.full((n, m), np.nan)
    rc = lib.gpmi_draws_normals(_seed_i64(seed), first_draw, n, m, z.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, rc
    return z


# Random123's kat_vectors for philox4x32-10: (counter, key, result)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_mirror_reproduces_the_published_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = dh.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]
    # vectorised over counters: the three at once, keys broadcast per row
    got = dh.philox4x32_10(np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64),
                           np.array([k[1] for k in KNOWN_ANSWERS], dtype=np.uint64))
    assert got.tolist() == [list(k[2]) for k in KNOWN_ANSWERS]


@pytest.mark.parametrize("m", [1, 2, 3, 129])
def test_host_entry_point_against_the_mirror(lib, m):
    """gpmi_draws_normals against tests/draws_host.normals within |dz| <= 32 . 2^-53 . r (draws_host.NORMAL_ULPS), for
    every seed and for a first draw in the counter's high word; the uniforms are integers, so a wrong word order or key
    shows as an O(1) difference, not as a few ulp."""
    n = 7
    worst = 0.0
    for seed in SEEDS:
        for first in (0, HIGH):
            got = lib_normals(lib, seed, first, n, m)
            want, r = dh.normals(seed, first, n, m, with_radius=True)
            assert np.isfinite(got).all()
            ratio = np.abs(got - want) / (2.0**-53 * r)
            worst = max(worst, float(ratio.max()))
    print(f"m = {m}: worst |dz| / (2^-53 r) = {worst:.2f} (bound {dh.NORMAL_ULPS})")
    assert worst <= dh.NORMAL_ULPS


def test_rows_do_not_depend_on_where_the_call_starts(lib):
    for seed in SEEDS:
        for base in (0, HIGH - 2):  # (the second window crosses into the high word)
            whole = lib_normals(lib, seed, base, 12, 5)
            for k, n in ((0, 12), (1, 4), (5, 7), (11, 1)):
                assert np.array_equal(lib_normals(lib, seed, base + k, n, 5), whole[k:k + n])
    # and the mirror agrees with itself in the same way
    assert np.array_equal(dh.normals(7, 3, 4, 5), dh.normals(7, 0, 9, 5)[3:7])


@pytest.mark.parametrize("seed", [2026, 0, -1])
def test_moments_of_the_stream(lib, seed):
    """512 x 128 normals: mean, variance, fourth moment and the correlation of the two members of a Box-Muller pair, each
    standardised to N(0, 1) under the hypothesis, within +-4 (the mirror gives at most 1.6 for all twelve)."""
    z = lib_normals(lib, seed, 0, 512, 128)
    stats = dh.moment_statistics(z)
    print(f"seed {seed}: mean, variance, kurtosis, pair correlation (standardised) = {np.round(stats, 3).tolist()}")
    assert np.abs(stats).max() <= 4.0, stats
    assert np.abs(dh.moment_statistics(dh.normals(seed, 0, 512, 128))).max() <= 4.0


def test_argument_validation_without_a_device(lib):
    dp = C.POINTER(C.c_double)
    buf = np.zeros(16)
    ptr = buf.ctypes.data_as(dp)
    info = C.c_int(7)
    # a NULL handle: GPMI_ERR_ARG whatever else is passed
    assert lib.gpmi_posterior_draws(None, ptr, 2, 1e-9, 2, None, 0, 0, None, ptr, None, C.byref(info)) == ERR_ARG
    assert lib.gpmi_mvn_draws(None, 2, ptr, ptr, 1e-9, 2, None, 0, 0, ptr, None, C.byref(info)) == ERR_ARG
    assert lib.gpmi_posterior_draws(None, None, 0, 0.0, 0, None, 0, 0, None, None, None, None) == ERR_ARG
    assert lib.gpmi_mvn_draws(None, 0, None, None, 0.0, 0, None, 0, 0, None, None, None) == ERR_ARG
    assert info.value == 7
    # the host-only entry point: sizes, a negative first draw, a NULL output
    assert lib.gpmi_draws_normals(1, 0, 2, 2, ptr) == 0
    for seed, first, n, m, out in ((1, 0, 0, 2, ptr), (1, 0, 2, 0, ptr), (1, -1, 2, 2, ptr), (1, 0, -3, 2, ptr), (1, 0, 2, -1, ptr),
                                   (1, 0, 2, 2, None), (1, 2**63 - 1, 2, 2, ptr)):
        assert lib.gpmi_draws_normals(seed, first, n, m, out) == ERR_ARG, (seed, first, n, m)


def test_python_argument_errors_need_no_device():
    from inference_amd.gp._draws import draw_arguments

    z = np.zeros((3, 4))
    assert draw_arguments("GpRegressor", 4, 3, None, z, 1e-9, 0)[1] is None
    for kwargs in (dict(seed=1, z=z, first_draw=0), dict(seed=None, z=z, first_draw=2), dict(seed=None, z=z[:2], first_draw=0),
                   dict(seed=None, z=z[:, :3], first_draw=0), dict(seed=None, z=z.ravel(), first_draw=0)):
        with pytest.raises(ValueError):
            draw_arguments("GpRegressor", 4, 3, kwargs["seed"], kwargs["z"], 1e-9, kwargs["first_draw"])
    with pytest.raises(ValueError):
        draw_arguments("GpRegressor", 4, 0, 1, None, 1e-9, 0)
    with pytest.raises(ValueError):
        draw_arguments("GpRegressor", 4, 1, 1, None, -1.0, 0)
    n, seed, zz, jitter, first = draw_arguments("GpRegressor", 4, 2, None, None, 1e-9, 5)
    assert (n, zz, jitter, first) == (2, None, 1e-9, 5) and 0 <= seed < 2**64
    assert draw_arguments("GpRegressor", 4, 2, -1, None, 0.0, 0)[1] == -1
