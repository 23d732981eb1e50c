"""
GPU tests of who owns the library's device and pinned memory (csrc/gpmi_internal.h: DevBuf): a handle that has been
through every regrowth - a second and third data set, a larger lockstep batch, more hyper-parameters, more query points,
more and fewer lanes, larger sparse-GP panels - computes what a fresh handle computes that makes the same call with
nothing to regrow, bit for bit (a value depends neither on the batch nor on the workspace it shares),
and gpmi_destroy gives back every byte the handle took (gpmi_live_bytes: the library's own two counters, never the
device's free memory, which other processes on a shared device change).

The C entry points are driven through _lib.Handle objects the tests create themselves (with the argument marshalling of
inference_amd._engine); d = 2 and the squared-exponential kernel unless a case says otherwise.  No tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 2
SE_THETA = np.array([0.1, -1.5, -1.3])       # ln a, ln l_1, ln l_2
RQ_THETA = np.array([0.1, 0.4, -1.5, -1.3])  # ln a, ln kappa, ln l_1, ln l_2


def live():
    """(device bytes, pinned bytes) the library holds now."""
    from inference_amd import _lib

    out = (C.c_int64 * 2)()
    assert _lib.load().gpmi_live_bytes(out) == 0
    return out[0], out[1]


def expect_live(cond, what):
    assert cond, what


def same_bits(got, want, what):
    assert got.keys() == want.keys(), what
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}: {key} differs in its bits"


def data_set(n, seed=5):
    rng = np.random.default_rng(seed + n)
    x = rng.uniform(0.0, 1.0, (n, D))
    y = np.sin(5.0 * x[:, 0]) * np.cos(3.0 * x[:, 1]) + 0.1 * rng.standard_normal(n)
    return x, y, np.full(n, 0.01) + 0.01 * rng.uniform(size=n)


def thetas(base, T):
    return base[None, :] + 0.05 * np.sin(np.arange(T * base.size, dtype=float)).reshape(T, base.size)


def query_points(m):
    return np.random.default_rng(100 + m).uniform(0.05, 0.95, (m, D))


def engine():
    """A GpEngine around a handle of the test's own, without a data set."""
    from inference_amd import _lib
    from inference_amd._engine import GpEngine

    e = GpEngine.__new__(GpEngine)
    e.h = _lib.Handle()
    return e


def set_data(e, x, y, noise_var):
    from inference_amd._lib import as_f64, dptr

    e.x, e.y = as_f64(x), as_f64(y)
    e.n, e.d = e.x.shape
    e.h.call("gpmi_set_data", dptr(e.x), dptr(e.y), dptr(as_f64(noise_var)), None, e.n, e.d)


def fit(e):
    from inference_amd import _lib

    alpha, logdet, info = e.fit(_lib.KERNEL_SE, SE_THETA, 0.0, np.zeros(e.n))
    assert info == 0
    return {"alpha": alpha, "logdet": logdet}


# ------------------------------------------------------------------------------------- one handle, three data sets
def batch_calls(e):
    """name -> call for the lockstep entry points, in the order that makes every workspace grow on the way: T = 3 before
    T = 40, SE (d + 1 parameters) before RQ (d + 2)."""
    from inference_amd import _lib

    SE, RQ = _lib.KERNEL_SE, _lib.KERNEL_RQ
    zeros3 = np.zeros(3)
    noise3 = np.stack([np.full(e.n, 0.01 * (t + 1)) for t in range(3)])

    def named(names, values):
        assert len(names) == len(values)
        if names[-1] == "info":
            assert not np.any(values[-1]), "a matrix did not factorise"
        return dict(zip(names, values))

    return {
        "fit": lambda: fit(e),
        "predict 5": lambda: named(("mu", "var"), e.predict(query_points(5))),
        "lml_batch 3": lambda: named(("lml", "info"), e.lml_batch(SE, thetas(SE_THETA, 3), mu_const=zeros3)),
        "lml_batch 40": lambda: named(("lml", "info"), e.lml_batch(SE, thetas(SE_THETA, 40), mu_const=np.zeros(40))),
        "grad_batch SE": lambda: named(("lml", "grad", "trq", "alpha", "info"),
                                       e.lml_grad_batch(SE, thetas(SE_THETA, 3), 0.0, mu_const=0.0)),
        "grad_batch RQ": lambda: named(("lml", "grad", "trq", "alpha", "info"),
                                       e.lml_grad_batch(RQ, thetas(RQ_THETA, 3), 0.0, mu_const=0.0)),
        "grad_batch_noise": lambda: named(("lml", "grad", "trq", "alpha", "qdiag", "info"),
                                          e.lml_grad_batch_noise(SE, thetas(SE_THETA, 3), 0.0, noise3, mu_const=0.0)),
        "loo_grad_batch": lambda: named(("alpha", "ikdiag", "p", "grad", "trq", "info"),
                                        e.loo_grad_batch(SE, thetas(SE_THETA, 3), 0.0, mu_const=0.0)),
        "predict_batch": lambda: named(("mean_t", "var_t", "mix_mean", "mix_var", "info"),
                                       e.predict_batch(SE, thetas(SE_THETA, 3), 0.0, query_points(5), mu_const=0.0)),
    }


GROWING = ("fit", "predict 5", "lml_batch 3", "lml_batch 40", "grad_batch SE", "grad_batch RQ", "grad_batch_noise",
           "loo_grad_batch", "predict_batch")
# the same calls with the largest request of each workspace first: nothing regrows behind them
LARGEST_FIRST = ("fit", "predict 5", "lml_batch 40", "lml_batch 3", "grad_batch RQ", "grad_batch SE", "grad_batch_noise",
                 "loo_grad_batch", "predict_batch")


def run_data_sets(used, sizes=(130, 70, 300)):
    """The data sets in turn on `used`, each against a fresh handle; the device total drops at the smaller one."""
    for n in sizes:
        x, y, nv = data_set(n)
        before = live()
        set_data(used, x, y, nv)
        if n < used_n(sizes, n):
            expect_live(live()[0] < before[0], f"gpmi_set_data with n = {n} after a larger data set holds no less")
        calls = batch_calls(used)
        got = {name: calls[name]() for name in GROWING}
        fresh = engine()
        try:
            set_data(fresh, x, y, nv)
            calls = batch_calls(fresh)
            want = {name: calls[name]() for name in LARGEST_FIRST}
        finally:
            fresh.close()
        for name in GROWING:
            same_bits(got[name], want[name], f"n = {n}, {name}")


def used_n(sizes, n):
    i = sizes.index(n)
    return sizes[i - 1] if i else 0


def test_one_handle_three_data_sets():
    """n = 130 (two tiles), 70 (one), 300 (three) on one handle: after each gpmi_set_data the fit, a predict and every
    lockstep batch entry point, with the lockstep workspace growing from 3 to 40 problems and the gradient workspace from
    d + 1 to d + 2 parameters on the way."""
    used = engine()
    try:
        run_data_sets(used)
    finally:
        used.close()


# ------------------------------------------------------------------------------------------------- query workspace
def mix_model(e):
    """Two SE sub-kernels with sigmoid window weights along x_0 (ChangePoint), and the weights at m query points."""
    from inference_amd import _lib

    def windows(pts):
        f = 1.0 / (1.0 + np.exp(-(pts[:, 0] - 0.5) / 0.1))
        return np.stack([1.0 - f, f])

    kernels, th = [_lib.KERNEL_SE, _lib.KERNEL_SE], [SE_THETA, SE_THETA + np.array([0.2, 0.3, -0.2])]
    return kernels, th, windows


def query_calls(e, m):
    pts = query_points(m)
    out = {}
    fit(e)
    out["predict"] = dict(zip(("mu", "var"), e.predict(pts)))
    out["posterior"] = dict(zip(("mu", "cov"), e.posterior(pts)))
    out["spatial_derivatives"] = dict(zip(("dmu", "dvar"), e.spatial_derivatives(pts)))
    out["gradient"] = dict(zip(("gmu", "gcov"), e.gradient(pts)))
    kernels, th, windows = mix_model(e)
    alpha, logdet, info = e.fit_mix(kernels, th, windows(e.x), 0.0, np.zeros(e.n))
    assert info == 0
    out["predict_mix"] = dict(zip(("alpha", "mu", "negsumsq"), (alpha,) + e.predict_mix(pts, windows(pts))))
    return out


def run_queries(used):
    """m = 5, 200, 5 on a fitted n = 130 handle: the query workspace grows once (one tile of rows, then two), and the
    mixture's third panel, first allocated at the small size, grows behind it."""
    x, y, nv = data_set(130)
    set_data(used, x, y, nv)
    want = {}
    for m in (5, 200):
        fresh = engine()
        try:
            set_data(fresh, x, y, nv)
            want[m] = query_calls(fresh, m)
        finally:
            fresh.close()
    for m in (5, 200, 5):
        got = query_calls(used, m)
        for name in want[m]:
            same_bits(got[name], want[m][name], f"m = {m}, {name}")


def test_query_workspace():
    used = engine()
    try:
        run_queries(used)
    finally:
        used.close()


# ------------------------------------------------------------------------------------------------------------ lanes
def lane_calls(e):
    from inference_amd import _lib

    out = {}
    for T in (1, 4):
        lml, info = e.lml_batch(_lib.KERNEL_SE, thetas(SE_THETA, T), mu_const=np.zeros(T))
        assert not np.any(info)
        out[f"lml_batch {T}"] = {"lml": lml}
    return out


def async_calls(e):
    from inference_amd import _lib

    out = {}
    for slot in (0, 1):
        e.lml_batch_submit(slot, _lib.KERNEL_SE, thetas(SE_THETA, 4 + slot), mu_const=np.zeros(4 + slot))
        lml, info = e.lml_batch_wait(slot)
        assert not np.any(info)
        out[f"slot {slot}"] = {"lml": lml}
    return out


def run_lanes(used):
    """gpmi_set_streams 1, 3, 1 (lanes are created, moved inside their vector and released), a single evaluation and a
    lockstep batch after each, then one asynchronous submit / wait pair per slot."""
    x, y, nv = data_set(130)
    set_data(used, x, y, nv)
    fresh = engine()
    try:
        set_data(fresh, x, y, nv)
        want = lane_calls(fresh)
        want_async = async_calls(fresh)
    finally:
        fresh.close()
    for streams in (1, 3, 1):
        used.set_streams(streams)
        got = lane_calls(used)
        for name in want:
            same_bits(got[name], want[name], f"{streams} streams, {name}")
    got = async_calls(used)
    for name in want_async:
        same_bits(got[name], want_async[name], name)


def test_lanes():
    used = engine()
    try:
        run_lanes(used)
    finally:
        used.close()


# -------------------------------------------------------------------------------------------------------- sparse GP
class Sparse:
    """A gpmi_sgp object on a handle of the caller's (SparseEngine makes its own)."""

    def __init__(self, h, x, z):
        from inference_amd._engine import SparseEngine
        from inference_amd._lib import as_f64, dptr

        s = self.s = SparseEngine.__new__(SparseEngine)
        s.x, s.z, s.h = as_f64(x), as_f64(z), h
        (s.n, s.d), s.m = s.x.shape, s.z.shape[0]
        s.ptr = C.c_void_p()
        h.call("gpmi_sgp_create", s.n, s.d, dptr(s.x), s.m, dptr(s.z), C.byref(s.ptr))

    def bound(self, panel_rows, want_zgrad=False):
        from inference_amd import _lib

        res = self.s.bound(_lib.KERNEL_SE, SE_THETA, 0.01, 1e-6, panel_rows, want_grad=True, want_alpha=True,
                           want_zgrad=want_zgrad)
        assert res[3] == 0
        return dict(zip(("F", "grad", "alpha", "info", "zgrad"), res))

    def destroy(self):
        assert self.s.h.lib.gpmi_sgp_destroy(self.s.ptr) == 0
        self.s.ptr = C.c_void_p()


SPARSE_CALLS = ((128, False), (256, False), (256, True))  # panel_rows (the panels regrow), then dF/dZ (allocated late)


def run_sparse(h):
    """n = 300 data, m = 130 inducing points on the caller's handle; the object is destroyed while the handle lives on, and
    takes with it what it took."""
    x, y, nv = data_set(300)
    z = x[:130].copy()
    before = live()
    used = Sparse(h, x, z)
    used.s.set_targets(y, nv)
    got = [used.bound(rows, zgrad) for rows, zgrad in SPARSE_CALLS]
    expect_live(live()[0] > before[0], "a sparse model holds device memory")
    used.destroy()
    expect_live(live() == before, "gpmi_sgp_destroy gives back what the object took")
    from inference_amd import _lib

    for (rows, zgrad), g in zip(SPARSE_CALLS, got):
        fh = _lib.Handle()
        try:
            fresh = Sparse(fh, x, z)
            fresh.s.set_targets(y, nv)
            same_bits(g, fresh.bound(rows, zgrad), f"panel_rows = {rows}, zgrad = {zgrad}")
        finally:
            fh.close()


def test_sparse_model_on_a_living_handle():
    from inference_amd import _lib

    h = _lib.Handle()
    try:
        run_sparse(h)
    finally:
        h.close()


# -------------------------------------------------------------------------------------------------------- give-back
def density_objects(h):
    """A KDE, a 2-D KDE and a unimodal object with their shared staging in use, left alive for gpmi_destroy."""
    from inference_amd._lib import as_f64, dptr

    rng = np.random.default_rng(9)
    n = 1000
    s = as_f64(np.sort(rng.standard_normal(n)))
    lo, hi = (C.c_int64 * 1)(0), (C.c_int64 * 1)(n)
    ptr = C.c_void_p()
    h.call("gpmi_kde_create", n, dptr(s), 1, lo, hi, C.byref(ptr))
    a, b = as_f64(rng.standard_normal(n)), as_f64(rng.standard_normal(n))
    k2 = C.c_void_p()
    h.call("gpmi_kde2d_create", n, dptr(a), dptr(b), C.byref(k2))
    out = np.empty(7)
    h.call("gpmi_kde2d_eval", k2, 7, dptr(a[:7].copy()), dptr(b[:7].copy()), 1.5, 1.5, dptr(out))
    assert np.all(out >= 1.0)  # every point is a sample: its own term is e^0
    uni = C.c_void_p()
    h.call("gpmi_unimodal_create", n, dptr(s), C.byref(uni))
    theta = as_f64([0.0, 1.0, 1.0, 0.1, 1.0, 2.0])
    val = np.empty(1)
    h.call("gpmi_unimodal_logpdf_sums", uni, 1, 1, dptr(theta), dptr(val))
    assert np.isfinite(val[0])


def test_destroy_gives_everything_back():
    """A handle that has done all of the above, with live density objects on it: after gpmi_destroy both totals are where
    they were before gpmi_create, exactly."""
    start = live()
    e = engine()
    try:
        expect_live(live() == start, "gpmi_create allocates nothing")
        run_data_sets(e)
        run_queries(e)
        run_lanes(e)
        run_sparse(e.h)
        density_objects(e.h)
        held = live()
        expect_live(held[0] > start[0] and held[1] > start[1], "the handle holds device and pinned memory")
    finally:
        e.close()
    expect_live(live() == start, f"after gpmi_destroy the library holds {live()} bytes, {start} before gpmi_create")
