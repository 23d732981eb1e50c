"""Device side of the density estimators: one lazily created `_lib.Handle` per device for the whole module (thousands
of KDEs from a tempering run share its stream and workspaces), the density objects of csrc/kde.hip, csrc/kde2d.hip
and csrc/unimodal.hip and the leave-one-out log-probability.  No CPU fallback: without the library or a GPU, `GpmiUnavailable` is raised.

The library expects the calls on one handle to be serialised (include/gpmi.h), and ctypes releases the GIL during a
call, so every gpmi_kde_* / gpmi_kde2d_* / gpmi_unimodal_* call - with the read of its error text - holds the handle's lock: KDEs built
and evaluated on several threads at once share the handle safely.  The lock is re-entrant, because a density object's finaliser
(which releases it on the device) can run inside a locked region of the same thread."""
import ctypes as C
import sys
import threading

import numpy as np

from inference_amd import _lib

COV_CHUNK_ROWS = _lib.COV_CHUNK_ROWS
COV_MAX_COLUMNS = _lib.COV_MAX_COLUMNS

_handles = {}
_handles_lock = threading.Lock()


def resolve_device(device=None) -> int:
    """The device index a call binds to: None means the default device of `_lib.Handle`."""
    return _lib.default_device() if device is None else int(device)


def handle(device=None) -> "_lib.Handle":
    """The module's handle for `device`, created on first use and again after it has been closed.  It carries the
    lock (`kde_lock`) that serialises the density calls made on it."""
    dev = resolve_device(device)
    with _handles_lock:
        h = _handles.get(dev)
        if h is None or not h.ctx:
            h = _lib.Handle(dev)
            h.kde_lock = threading.RLock()
            _handles[dev] = h
        return h


def _call(h, name, *args):
    """One gpmi_kde_* call on handle h, serialised with every other call on it; a non-zero status raises GpmiError
    with the handle's error text of that very call."""
    with h.kde_lock:
        if not h.ctx:
            raise _lib.GpmiUnavailable("the device handle of this density has been closed")
        rc = getattr(h.lib, name)(*args)
        if rc != 0:
            text = h.lib.gpmi_last_error(h.ctx).decode()
            raise _lib.GpmiError(f"{name} failed with status {rc}: {text}")


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class DeviceDensity:
    """A sorted sample and its region table [lo[r], hi[r]) on the device (gpmi_kde_create)."""

    def __init__(self, sorted_sample, lo, hi, device=None):
        self.h = handle(device)
        s = np.ascontiguousarray(sorted_sample, dtype=np.float64)
        lo = np.ascontiguousarray(lo, dtype=np.int64)
        hi = np.ascontiguousarray(hi, dtype=np.int64)
        self.n_regions = lo.size
        self.ptr = C.c_void_p()
        _call(self.h, "gpmi_kde_create", self.h.ctx, s.size, _lib.dptr(s), lo.size, _i64(lo), _i64(hi), C.byref(self.ptr))

    def sums(self, x, regions, q, pdf=True, cdf=True):
        """Raw slice sums at the points x of the given regions: (pdf_sum or None, cdf_sum or None)."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        r = np.ascontiguousarray(regions, dtype=np.int64).ravel()
        ps = np.empty(x.size) if pdf else None
        cs = np.empty(x.size) if cdf else None
        _call(self.h, "gpmi_kde_eval", self.ptr, x.size, _lib.dptr(x), _i64(r), float(q), _lib.dptr(ps), _lib.dptr(cs))
        return ps, cs

    def __del__(self):
        # a handle that has been closed (interpreter exit, _close_all_handles) has released its density objects already
        if sys.is_finalizing():
            return
        h = getattr(self, "h", None)
        if h is None or not getattr(self, "ptr", None):
            return
        with h.kde_lock:
            if h.ctx and self.ptr:
                h.lib.gpmi_kde_destroy(self.ptr)
            self.ptr = C.c_void_p()


class DeviceDensity2D:
    """The samples (x_j, y_j) of a 2-D estimate on the device (gpmi_kde2d_create, csrc/kde2d.hip).  Every method returns
    raw sums S(a, b) = sum_j exp(-((x_j - a) q_x)^2 - ((y_j - b) q_y)^2); the caller applies the normalisation."""

    def __init__(self, x, y, device=None):
        self.h = handle(device)
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        self.n = x.size
        self.ptr = C.c_void_p()
        _call(self.h, "gpmi_kde2d_create", self.h.ctx, x.size, _lib.dptr(x), _lib.dptr(y), C.byref(self.ptr))

    def sums(self, a, b, q_x, q_y):
        """S at the scattered points (a_i, b_i): the direct sum (gpmi_kde2d_eval)."""
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        out = np.empty(a.size)
        _call(self.h, "gpmi_kde2d_eval", self.h.ctx, self.ptr, a.size, _lib.dptr(a), _lib.dptr(b), float(q_x), float(q_y),
              _lib.dptr(out))
        return out

    def self_sums(self, q_x, q_y, count_tiles=False):
        """S at every sample, in the order given (gpmi_kde2d_self); with count_tiles also (tile pairs computed, tile
        pairs in all) of its skip rule."""
        out = np.empty(self.n)
        tiles = np.zeros(2, dtype=np.int64)
        _call(self.h, "gpmi_kde2d_self", self.h.ctx, self.ptr, float(q_x), float(q_y), _lib.dptr(out),
              _i64(tiles) if count_tiles else None)
        return (out, (int(tiles[0]), int(tiles[1]))) if count_tiles else out

    def grid_sums(self, x_axis, y_axis, q_x, q_y):
        """S on the grid of the two axes, shape (len(y_axis), len(x_axis)): the factorised product (gpmi_kde2d_grid)."""
        xa = np.ascontiguousarray(x_axis, dtype=np.float64).ravel()
        ya = np.ascontiguousarray(y_axis, dtype=np.float64).ravel()
        out = np.empty((ya.size, xa.size))
        _call(self.h, "gpmi_kde2d_grid", self.h.ctx, self.ptr, xa.size, _lib.dptr(xa), ya.size, _lib.dptr(ya), float(q_x),
              float(q_y), _lib.dptr(out))
        return out

    def __del__(self):
        if sys.is_finalizing():
            return
        h = getattr(self, "h", None)
        if h is None or not getattr(self, "ptr", None):
            return
        with h.kde_lock:
            if h.ctx and self.ptr:
                h.lib.gpmi_kde2d_destroy(h.ctx, self.ptr)
            self.ptr = C.c_void_p()


class DeviceUnimodal:
    """A sample on the device in the order given (gpmi_unimodal_create, csrc/unimodal.hip), for the sums of the
    UnimodalPdf model's log-density over it."""

    def __init__(self, sample, device=None):
        self.h = handle(device)
        s = np.ascontiguousarray(sample, dtype=np.float64).ravel()
        self.n = s.size
        self.ptr = C.c_void_p()
        _call(self.h, "gpmi_unimodal_create", self.h.ctx, s.size, _lib.dptr(s), C.byref(self.ptr))

    def sums(self, thetas, stride=1):
        """Sum of log_pdf_model(sample[::stride], theta) for every row theta of `thetas` (T x 6), in one call."""
        th = np.ascontiguousarray(thetas, dtype=np.float64).reshape(-1, 6)
        out = np.empty(th.shape[0])
        _call(self.h, "gpmi_unimodal_logpdf_sums", self.h.ctx, self.ptr, int(stride), th.shape[0], _lib.dptr(th),
              _lib.dptr(out))
        return out

    def __del__(self):
        if sys.is_finalizing():
            return
        h = getattr(self, "h", None)
        if h is None or not getattr(self, "ptr", None):
            return
        with h.kde_lock:
            if h.ctx and self.ptr:
                h.lib.gpmi_unimodal_destroy(h.ctx, self.ptr)
            self.ptr = C.c_void_p()


def _dense_columns(sample2d, who):
    """`sample2d` as a float64 array the column entry points can read in place - dense in C order (also a view of some
    of its columns) or as the transpose of such an array; any other view is made C-contiguous first - with its shape and
    its strides in elements."""
    s = np.asarray(sample2d, dtype=np.float64)
    if s.ndim != 2:
        raise ValueError(f"{who} takes a two-dimensional sample")
    n, m = s.shape
    item = s.itemsize
    rs, cs = s.strides

    def dense(a, b, count):  # strides (ld, 1) in elements with ld >= count
        return b == item and a % item == 0 and a // item >= count

    if not s.flags.aligned or not (dense(rs, cs, m) or dense(cs, rs, n) or (m == 1 and rs == item)):
        s = np.ascontiguousarray(s)
        rs, cs = s.strides
    return s, n, m, rs // item, cs // item


def hdi_columns(sample2d, Ls, device=None, ws_bytes=0):
    """The narrowest windows of the columns of `sample2d` (n x m, float64) for every window length of `Ls`
    (gpmi_hdi_columns, csrc/hdi.hip): `hdi` of shape (len(Ls), 2, m) and `flags` (m, bool), set for the columns that
    hold a NaN or an infinity, whose numbers in `hdi` mean nothing.  The array is read in place through its own strides
    when it is dense in either order (C order, also a view of some of its columns, or the transpose of such an array);
    any other view is made C-contiguous first.  `ws_bytes` caps the device workspace (0: the library's default)."""
    s, n, m, rs, cs = _dense_columns(sample2d, "hdi_columns")
    L = np.ascontiguousarray(Ls, dtype=np.int64).ravel()
    hdi = np.empty((L.size, 2, m))
    flags = np.zeros(m, dtype=np.int32)
    h = handle(device)
    _call(h, "gpmi_hdi_columns", h.ctx, n, m, rs, cs, s.ctypes.data_as(C.POINTER(C.c_double)), L.size, _i64(L), int(ws_bytes),
          _lib.dptr(hdi), flags.ctypes.data_as(C.POINTER(C.c_int32)))
    return hdi, flags.astype(bool)


def acf_columns(sample2d, device=None, ws_bytes=0):
    """The autocorrelation sums of the columns of `sample2d` (n x m, float64) up to their first negative lag
    (gpmi_acf_columns, csrc/acf.hip): `f0`, `sum` (m, float64), `cut` (m, int64) and `flags` (m, int32): 0 for an
    answered column, 1 for one that holds a NaN or an infinity, 2 for one without a negative lag below n // 2; the
    numbers of a flagged column mean nothing.  The array is read in place under the rules of `hdi_columns`."""
    s, n, m, rs, cs = _dense_columns(sample2d, "acf_columns")
    f0 = np.zeros(m)
    total = np.zeros(m)
    cut = np.zeros(m, dtype=np.int64)
    flags = np.zeros(m, dtype=np.int32)
    h = handle(device)
    _call(h, "gpmi_acf_columns", h.ctx, n, m, rs, cs, s.ctypes.data_as(C.POINTER(C.c_double)), int(ws_bytes),
          _lib.dptr(f0), _lib.dptr(total), _i64(cut), flags.ctypes.data_as(C.POINTER(C.c_int32)))
    return f0, total, cut, flags


def cov_columns(sample2d, device=None, ws_bytes=0):
    """The column means and the covariance matrix of the columns of `sample2d` (n x m, float64, m <= 512), as
    numpy.cov(sample2d.T) defines it (gpmi_cov_columns, csrc/cov.hip): `mean` (m), `cov` (m, m) and `flags` (m, int32),
    1 for a column that holds a NaN or an infinity, whose rows and columns of `cov` mean nothing.  The array is read in
    place under the rules of `hdi_columns`; `ws_bytes` caps the partial tiles on the device (0: the library's default)."""
    s, n, m, rs, cs = _dense_columns(sample2d, "cov_columns")
    mean = np.zeros(m)
    cov = np.zeros((m, m))
    flags = np.zeros(m, dtype=np.int32)
    h = handle(device)
    _call(h, "gpmi_cov_columns", h.ctx, n, m, rs, cs, s.ctypes.data_as(C.POINTER(C.c_double)), int(ws_bytes),
          _lib.dptr(mean), _lib.dptr(cov), flags.ctypes.data_as(C.POINTER(C.c_int32)))
    return mean, cov, flags


def acf_lag_blocks(n):
    """The first lags of the blocks in which gpmi_acf_columns walks the lags of a column of n rows (host-only)."""
    lib = _lib.load()
    count = C.c_int64(0)
    if lib.gpmi_acf_lag_blocks(int(n), 0, None, C.byref(count)) != 0:
        raise ValueError("acf_lag_blocks takes n >= 2")
    starts = np.zeros(count.value, dtype=np.int64)
    if lib.gpmi_acf_lag_blocks(int(n), starts.size, _i64(starts), C.byref(count)) != 0:
        raise _lib.GpmiError("gpmi_acf_lag_blocks failed")
    return [int(k) for k in starts]


def cv_logprob(samples, widths, c=0.99, device=None):
    """Leave-one-out log-probabilities of `samples` for every width (gpmi_kde_cv_logprob, one call).  A width that is
    not finite and positive gives NaN without a device call, as the reference's arithmetic does for width = inf."""
    widths = np.asarray(widths, dtype=np.float64).ravel()
    out = np.full(widths.size, np.nan)
    ok = np.isfinite(widths) & (widths > 0)
    if ok.any():
        h = handle(device)
        s = np.ascontiguousarray(samples, dtype=np.float64).ravel()
        w = np.ascontiguousarray(widths[ok])
        lp = np.empty(w.size)
        _call(h, "gpmi_kde_cv_logprob", h.ctx, s.size, _lib.dptr(s), w.size, _lib.dptr(w), float(c), _lib.dptr(lp))
        out[ok] = lp
    return out
