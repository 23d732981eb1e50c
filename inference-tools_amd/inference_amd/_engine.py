"""
NumPy-facing wrapper around one gpmi handle: uploads the data once and exposes
the device operations of the GP hot path with ndarray arguments / results.
Used by `inference_amd.gp.regression.GpRegressor` and the covariance classes.
"""
import ctypes as C
import os

import numpy as np

from inference_amd import _lib
from inference_amd._lib import as_f64, dptr


class _DeviceCommMixin:
    """The library's RCCL communicator on the handle `self.h` (gpmi_comm_*): the start-up broadcast of the data set
    and the result gather of the sharded drivers (inference_amd.sharding)."""

    comm_world = 0

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = _lib.load().gpmi_comm_unique_id(buf)
        if rc != 0:
            raise _lib.GpmiError(f"gpmi_comm_unique_id failed with status {rc} (librccl missing?)")
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        # RCCL prints a version banner on stdout from rank 0; keep stdout clean for callers that
        # emit machine-readable output (bench.py prints one JSON line) by sending it to stderr
        import os
        import sys

        libc = C.CDLL(None)
        sys.stdout.flush()
        libc.fflush(None)
        saved = os.dup(1)
        try:
            os.dup2(2, 1)
            self.h.call("gpmi_comm_init", int(rank), int(world), unique_id)
        finally:
            # the banner sits in C stdio's buffer when stdout is not a terminal: flush it while fd 1 still points
            # at stderr, or it would come out after the caller's own output at process exit
            libc.fflush(None)
            os.dup2(saved, 1)
            os.close(saved)
        self.comm_world = world

    def comm_allgather(self, values):
        send = as_f64(values).ravel()
        recv = np.empty(send.size * self.comm_world)
        self.h.call("gpmi_comm_allgather", dptr(send), dptr(recv), send.size)
        return recv.reshape(self.comm_world, send.size)

    def comm_broadcast(self, values, root: int = 0):
        """`values` of rank `root` on every rank (one ncclBroadcast); the other ranks pass an array of the same shape."""
        buf = as_f64(values).copy()
        self.h.call("gpmi_comm_broadcast", dptr(buf.ravel()), buf.size, int(root))
        return buf

    def comm_count(self) -> int:
        """Ranks RCCL itself sees in the communicator (ncclCommCount)."""
        n = C.c_int(0)
        self.h.call("gpmi_comm_count", C.byref(n))
        return n.value

    def comm_destroy(self):
        self.h.call("gpmi_comm_destroy")
        self.comm_world = 0


def _seed_i64(seed):
    """The 64-bit pattern of `seed` as the signed integer the C-ABI takes."""
    return ((int(seed) + (1 << 63)) % (1 << 64)) - (1 << 63)


class _DrawsMixin:
    """gpmi_mvn_draws on the handle `self.h`: joint normal draws from a mean vector and a covariance matrix."""

    def mvn_draws(self, mean, cov, n_draws=1, seed=0, z=None, jitter=1e-9, first_draw=0):
        """`n_draws` rows mean + z_s L^T with L L^T = cov + eps I, eps = jitter * max diag(cov) (the lower triangle of
        `cov` is read).  z: (n_draws, m) normals of the caller, or None: rows first_draw .. of the stream of `seed`.
        Returns (draws (n_draws, m) - None if info != 0 -, eps, info)."""
        mean, cov = as_f64(mean), as_f64(cov)
        m = mean.size
        if cov.shape != (m, m):
            raise ValueError(f"cov must be ({m}, {m}), got {cov.shape}")
        z = None if z is None else as_f64(z).reshape(int(n_draws), m)
        draws = np.empty((int(n_draws), m))
        eps, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_mvn_draws", m, dptr(mean), dptr(cov), float(jitter), int(n_draws), dptr(z), _seed_i64(seed),
                    int(first_draw), dptr(draws), C.byref(eps), C.byref(info))
        return (draws if info.value == 0 else None), eps.value, info.value


class DeviceComm(_DeviceCommMixin):
    """A communicator on a handle of its own, for what happens before a rank has any data: rank 0 broadcasts x, y,
    y_err (sharding.broadcast_dataset; the reference pickles the whole regressor into its worker processes,
    regression.py:597-601, mcmc/parallel.py:127-136), every rank then builds its own regressor.  The same object can
    serve the result gathers (`engine=` of the sharded drivers)."""

    def __init__(self, device=None):
        self.h = _lib.Handle(device)

    def close(self):
        self.h.close()


class GpEngine(_DeviceCommMixin, _DrawsMixin):
    def __init__(self, x, y, noise_var=None, y_cov=None, device=None, reserve=0):
        self.h = _lib.Handle(device)
        self.x = as_f64(x)
        self.y = as_f64(y)
        self.n, self.d = self.x.shape
        if reserve:
            self.h.call("gpmi_set_option", _lib.OPT_RESERVE_POINTS, int(reserve))
        nv = None if noise_var is None else as_f64(noise_var)
        yc = None if y_cov is None else as_f64(y_cov)
        self.h.call("gpmi_set_data", dptr(self.x), dptr(self.y), dptr(nv), dptr(yc), self.n, self.d)

    # -- fit / likelihood -----------------------------------------------------------
    def fit(self, kernel, theta_cov, extra_diag, mu):
        theta = as_f64(theta_cov)
        mu = as_f64(mu)
        alpha = np.empty(self.n)
        logdet = C.c_double(0.0)
        info = C.c_int(0)
        self.h.call("gpmi_fit", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    dptr(alpha), C.byref(logdet), C.byref(info))
        return alpha, logdet.value, info.value

    def lml(self, kernel, theta_cov, extra_diag, mu):
        theta = as_f64(theta_cov)
        mu = as_f64(mu)
        out = C.c_double(0.0)
        info = C.c_int(0)
        self.h.call("gpmi_lml", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    C.byref(out), C.byref(info))
        return out.value, info.value

    def lml_batch(self, kernel, thetas_cov, extra_diag=None, mus=None, mu_const=None):
        thetas = as_f64(thetas_cov)
        if thetas.size == 0:
            return np.empty(0), np.zeros(0, dtype=np.int32)
        T, nt = thetas.shape
        ex = None if extra_diag is None else as_f64(extra_diag)
        mus = None if mus is None else as_f64(mus)
        mc = None if mu_const is None else as_f64(mu_const)
        out = np.empty(T)
        info = np.zeros(T, dtype=np.int32)
        self.h.call("gpmi_lml_batch", kernel, T, dptr(thetas), nt, dptr(ex), dptr(mus), dptr(mc),
                    dptr(out), info.ctypes.data_as(C.POINTER(C.c_int)))
        return out, info

    # evaluations per slot of the asynchronous form (gpmi.h); the library reads the same three environment variables
    ASYNC_MAX = int(os.environ.get("GPMI_ASYNC_SLOT_MAX", "256"))
    _BATCH_GIB = int(os.environ.get("GPMI_BATCH_GIB", "24"))
    _BATCH_MAX = int(os.environ.get("GPMI_BATCH_MAX", "512"))

    def async_slot_capacity(self):
        """Evaluations one asynchronous slot can hold: half of the lockstep workspace (api.hip: ensure_batch_ws keeps it
        below 512 matrices and 24 GiB; GPMI_BATCH_MAX / GPMI_BATCH_GIB)."""
        cap = self.capacity()
        per = cap * (cap + 32) * 8
        return max(0, min(self.ASYNC_MAX, min(self._BATCH_MAX, (self._BATCH_GIB << 30) // per) // 2))

    def lml_batch_submit(self, slot, kernel, thetas_cov, extra_diag=None, mus=None, mu_const=None):
        """gpmi_lml_batch_submit: enqueue the evaluations of `slot` (0 / 1) and return; `lml_batch_wait(slot)` delivers."""
        thetas = as_f64(thetas_cov)
        T, nt = thetas.shape
        ex = None if extra_diag is None else as_f64(extra_diag)
        mus = None if mus is None else as_f64(mus)
        mc = None if mu_const is None else as_f64(mu_const)
        self.h.call("gpmi_lml_batch_submit", kernel, T, dptr(thetas), nt, dptr(ex), dptr(mus), dptr(mc), int(slot))
        self._pending = getattr(self, "_pending", {})
        self._pending[int(slot)] = T

    def lml_batch_wait(self, slot):
        T = self._pending.pop(int(slot))
        out = np.empty(T)
        info = np.zeros(T, dtype=np.int32)
        self.h.call("gpmi_lml_batch_wait", int(slot), dptr(out), info.ctypes.data_as(C.POINTER(C.c_int)))
        return out, info

    # -- mixture covariance (ChangePoint): sub-kernel ids / parameter vectors + per-point weights ------------
    @staticmethod
    def _mix_args(kernels, thetas, weights):
        ks = np.ascontiguousarray(kernels, dtype=np.int32)
        nts = np.ascontiguousarray([len(t) for t in thetas], dtype=np.int32)
        th = as_f64(np.concatenate([np.asarray(t, dtype=float) for t in thetas]))
        g = as_f64(weights)
        ip = C.POINTER(C.c_int)
        return len(ks), ks, ks.ctypes.data_as(ip), th, nts, nts.ctypes.data_as(ip), g

    def fit_mix(self, kernels, thetas, weights, extra_diag, mu):
        nk, ks, kp, th, nts, ntp, g = self._mix_args(kernels, thetas, weights)
        mu = as_f64(mu)
        alpha = np.empty(self.n)
        logdet, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_fit_mix", nk, kp, dptr(th), ntp, dptr(g), float(extra_diag), dptr(mu), dptr(alpha),
                    C.byref(logdet), C.byref(info))
        return alpha, logdet.value, info.value

    def lml_mix(self, kernels, thetas, weights, extra_diag, mu):
        nk, ks, kp, th, nts, ntp, g = self._mix_args(kernels, thetas, weights)
        mu = as_f64(mu)
        out, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_lml_mix", nk, kp, dptr(th), ntp, dptr(g), float(extra_diag), dptr(mu), C.byref(out),
                    C.byref(info))
        return out.value, info.value

    def lml_grad_mix(self, kernels, thetas, weights, extra_diag, mu, row_weights=None):
        """row_weights (nk, 2, n): the caller's own row-sum weights (include/gpmi.h: hw); hrows then is (nk, 2, n)."""
        nk, ks, kp, th, nts, ntp, g = self._mix_args(kernels, thetas, weights)
        mu = as_f64(mu)
        lml, info = C.c_double(0.0), C.c_int(0)
        grad = np.empty(th.size)
        hw = None if row_weights is None else as_f64(np.asarray(row_weights, dtype=float).reshape(nk, 2, self.n))
        hrows = np.empty((nk, self.n) if hw is None else (nk, 2, self.n))
        alpha = np.empty(self.n)
        self.h.call("gpmi_lml_grad_mix", nk, kp, dptr(th), ntp, dptr(g), dptr(hw), float(extra_diag), dptr(mu),
                    C.byref(lml), dptr(grad), dptr(hrows), dptr(alpha), C.byref(info))
        return lml.value, grad, hrows, alpha, info.value

    def lml_grad_batch_mix(self, kernels, thetas, weights, extra_diag=None, mus=None, mu_const=None, want_qdiag=False,
                           row_weights=None):
        """gpmi_lml_grad_batch_mix: T evaluations of the mixture likelihood and its gradient pieces in one call.
        kernels: the nk sub-kernel ids; thetas: T lists of nk parameter vectors; weights: (T, nk, n) window weights;
        row_weights: None or (T, nk, 2, n) (include/gpmi.h: hw).
        Returns (lml (T,), grad (T, sum n_thetas), hrows (T, nk, n) - (T, nk, 2, n) with row_weights -, alpha (T, n),
        qdiag (T, n) or None, info (T,))."""
        ks = np.ascontiguousarray(kernels, dtype=np.int32)
        nk = len(ks)
        T = len(thetas)
        nts = np.ascontiguousarray([len(t) for t in thetas[0]], dtype=np.int32)
        th = as_f64(np.array([np.concatenate([np.asarray(v, dtype=float) for v in row]) for row in thetas]))
        g = as_f64(np.asarray(weights, dtype=float).reshape(T, nk, self.n))
        ex = None if extra_diag is None else as_f64(extra_diag)
        mus = None if mus is None else as_f64(mus)
        mc = None if mu_const is None else as_f64(mu_const)
        lml = np.empty(T)
        grad = np.empty((T, int(nts.sum())))
        hw = None if row_weights is None else as_f64(np.asarray(row_weights, dtype=float).reshape(T, nk, 2, self.n))
        hrows = np.empty((T, nk, self.n) if hw is None else (T, nk, 2, self.n))
        alpha = np.empty((T, self.n))
        qdiag = np.empty((T, self.n)) if want_qdiag else None
        info = np.zeros(T, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self.h.call("gpmi_lml_grad_batch_mix", nk, ks.ctypes.data_as(ip), T, dptr(th), nts.ctypes.data_as(ip), dptr(g),
                    dptr(hw), dptr(ex), dptr(mus), dptr(mc), dptr(lml), dptr(grad), dptr(hrows), dptr(alpha), dptr(qdiag),
                    info.ctypes.data_as(ip))
        return lml, grad, hrows, alpha, qdiag, info

    def loo_grad_batch_mix(self, kernels, thetas, weights, extra_diag=None, mus=None, mu_const=None, row_weights=None):
        """gpmi_loo_grad_batch_mix: T evaluations of the mixture's leave-one-out pieces in one call (lockstep sizes only).
        Arguments as `lml_grad_batch_mix`.  Returns (alpha, ikdiag, pvec, mdiag (T, n each), grad (T, sum n_thetas),
        hrows (T, nk, n) - (T, nk, 2, n) with row_weights -, info (T,))."""
        ks = np.ascontiguousarray(kernels, dtype=np.int32)
        nk = len(ks)
        T = len(thetas)
        nts = np.ascontiguousarray([len(t) for t in thetas[0]], dtype=np.int32)
        th = as_f64(np.array([np.concatenate([np.asarray(v, dtype=float) for v in row]) for row in thetas]))
        g = as_f64(np.asarray(weights, dtype=float).reshape(T, nk, self.n))
        ex = None if extra_diag is None else as_f64(extra_diag)
        mus = None if mus is None else as_f64(mus)
        mc = None if mu_const is None else as_f64(mu_const)
        alpha, ikdiag, pvec, mdiag = (np.empty((T, self.n)) for _ in range(4))
        grad = np.empty((T, int(nts.sum())))
        hw = None if row_weights is None else as_f64(np.asarray(row_weights, dtype=float).reshape(T, nk, 2, self.n))
        hrows = np.empty((T, nk, self.n) if hw is None else (T, nk, 2, self.n))
        info = np.zeros(T, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self.h.call("gpmi_loo_grad_batch_mix", nk, ks.ctypes.data_as(ip), T, dptr(th), nts.ctypes.data_as(ip), dptr(g),
                    dptr(hw), dptr(ex), dptr(mus), dptr(mc), dptr(alpha), dptr(ikdiag), dptr(pvec), dptr(mdiag), dptr(grad),
                    dptr(hrows), info.ctypes.data_as(ip))
        return alpha, ikdiag, pvec, mdiag, grad, hrows, info

    def loo_terms_mix(self, kernels, thetas, weights, extra_diag, mu):
        nk, ks, kp, th, nts, ntp, g = self._mix_args(kernels, thetas, weights)
        mu = as_f64(mu)
        alpha, ikdiag = np.empty(self.n), np.empty(self.n)
        info = C.c_int(0)
        self.h.call("gpmi_loo_terms_mix", nk, kp, dptr(th), ntp, dptr(g), float(extra_diag), dptr(mu),
                    dptr(alpha), dptr(ikdiag), C.byref(info))
        return alpha, ikdiag, info.value

    def predict_mix(self, pts, query_weights):
        p = as_f64(pts)
        gq = as_f64(query_weights)
        m = p.shape[0]
        mu, nss = np.empty(m), np.empty(m)
        self.h.call("gpmi_predict_mix", dptr(p), m, dptr(gq), dptr(mu), dptr(nss))
        return mu, nss

    def posterior_mix(self, pts, query_weights, mean_only=False):
        p = as_f64(pts)
        gq = as_f64(query_weights)
        m = p.shape[0]
        mu = np.empty(m)
        cov = None if mean_only else np.empty((m, m))
        self.h.call("gpmi_posterior_mix", dptr(p), m, dptr(gq), dptr(mu), dptr(cov))
        return mu, cov

    def set_sum(self, kernels):
        """gpmi_set_sum: the components (GPMI_KERNEL_SE / _RQ / _M32 / _M52 / _PER ids, in order) of this handle's GPMI_KERNEL_SUM."""
        ks = np.ascontiguousarray(kernels, dtype=np.int32)
        self.h.call("gpmi_set_sum", int(ks.size), ks.ctypes.data_as(C.POINTER(C.c_int)))

    def set_periodic(self, dims):
        """gpmi_set_periodic: the dimensions (strictly ascending) in which this handle's GPMI_KERNEL_PER is periodic."""
        ds = np.ascontiguousarray(dims, dtype=np.int32)
        self.h.call("gpmi_set_periodic", int(ds.size), ds.ctypes.data_as(C.POINTER(C.c_int)))

    def set_noise(self, noise_var):
        self.h.call("gpmi_set_noise", dptr(as_f64(noise_var)))

    def lml_grad_qdiag(self):
        q = np.empty(self.n)
        self.h.call("gpmi_lml_grad_qdiag", dptr(q))
        return q

    def prepare_gradient(self, n_theta: int):
        """gpmi_prepare_gradient: the gradient path's lazily allocated workspaces, now."""
        self.h.call("gpmi_prepare_gradient", int(n_theta))

    def capacity(self):
        cap = C.c_int64(0)
        self.h.call("gpmi_capacity", C.byref(cap))
        return cap.value

    def append_point(self, x_new, y_new, noise_var_new, mu):
        """Append one training point at the fitted hyper-parameters (gpmi_append_point): (alpha, logdet, info)."""
        xn, mu = as_f64(np.ravel(x_new)), as_f64(mu)
        alpha = np.empty(self.n + 1)
        logdet, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_append_point", dptr(xn), float(y_new), float(noise_var_new), dptr(mu), dptr(alpha),
                    C.byref(logdet), C.byref(info))
        if info.value == 0:
            self.x = np.vstack([self.x, xn[None, :]])
            self.y = np.append(self.y, float(y_new))
            self.n += 1
        return alpha, logdet.value, info.value

    def set_option(self, option, value):
        self.h.call("gpmi_set_option", int(option), int(value))

    def set_streams(self, n):
        self.h.call("gpmi_set_streams", int(n))

    def lml_grad(self, kernel, theta_cov, extra_diag, mu):
        theta = as_f64(theta_cov)
        mu = as_f64(mu)
        lml = C.c_double(0.0)
        trq = C.c_double(0.0)
        info = C.c_int(0)
        grad = np.empty(theta.size)
        alpha = np.empty(self.n)
        self.h.call("gpmi_lml_grad", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    C.byref(lml), dptr(grad), C.byref(trq), dptr(alpha), C.byref(info))
        return lml.value, grad, trq.value, alpha, info.value

    def lml_hessian(self, kernel, theta_cov, extra_diag, mu, phi=None):
        """gpmi_lml_hessian: the LML, its gradient and its exact Hessian from one factorisation.  phi: (n_mean, n) rows
        d mu / d (mean parameter), or None.  Returns (lml, grad (n_theta + 1,): the kernel's parameters then ln sigma
        of `extra_diag`, hess (n_mean + n_theta + 1,) squared: mean, kernel, ln sigma, alpha (n,), info); with
        info != 0 the arrays are None."""
        theta = as_f64(theta_cov)
        mu = as_f64(mu)
        phi = None if phi is None or len(phi) == 0 else as_f64(np.atleast_2d(phi))
        n_mean = 0 if phi is None else phi.shape[0]
        if phi is not None and phi.shape[1] != self.n:
            raise ValueError(f"phi must be (n_mean, {self.n}), got {phi.shape}")
        nh = n_mean + theta.size + 1
        lml, info = C.c_double(0.0), C.c_int(0)
        grad, hess = np.zeros(theta.size + 1), np.zeros((nh, nh))
        self.h.call("gpmi_lml_hessian", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu), dptr(phi), n_mean,
                    C.byref(lml), dptr(grad), dptr(hess), C.byref(info))
        if info.value != 0:
            return None, None, None, None, info.value
        alpha = np.empty(self.n)
        self.h.call("gpmi_lml_hessian_alpha", dptr(alpha))
        return lml.value, grad, hess, alpha, 0

    def lml_grad_batch(self, kernel, thetas_cov, extra_diag, mus=None, mu_const=None):
        """T evaluations of `lml_grad` in one call (gpmi_lml_grad_batch: lockstep for padded N <= 4096):
        (lml (T,), grad (T, n_theta), trace_q (T,), alpha (T, n), info (T,))."""
        th = as_f64(np.atleast_2d(thetas_cov))
        T, nth = th.shape
        ex = as_f64(np.broadcast_to(np.asarray(extra_diag, dtype=float), (T,)))
        lml, trq = np.empty(T), np.empty(T)
        grad, alpha = np.empty((T, nth)), np.empty((T, self.n))
        info = np.zeros(T, dtype=np.int32)
        mus_p = dptr(as_f64(mus)) if mus is not None else None
        muc_p = dptr(as_f64(np.broadcast_to(np.asarray(mu_const, dtype=float), (T,)))) if mus is None else None
        self.h.call("gpmi_lml_grad_batch", kernel, T, dptr(th), nth, dptr(ex), mus_p, muc_p, dptr(lml), dptr(grad),
                    dptr(trq), dptr(alpha), info.ctypes.data_as(C.POINTER(C.c_int)))
        return lml, grad, trq, alpha, info

    def lml_grad_batch_noise(self, kernel, thetas_cov, extra_diag, noise_vars, mus=None, mu_const=None):
        """`lml_grad_batch` with noise variances of their own for every evaluation (gpmi_lml_grad_batch_noise):
        (lml, grad, trace_q, alpha, qdiag (T, n), info)."""
        th = as_f64(np.atleast_2d(thetas_cov))
        T, nth = th.shape
        ex = as_f64(np.broadcast_to(np.asarray(extra_diag, dtype=float), (T,)))
        nv = as_f64(np.atleast_2d(noise_vars))
        lml, trq = np.empty(T), np.empty(T)
        grad, alpha, qdiag = np.empty((T, nth)), np.empty((T, self.n)), np.empty((T, self.n))
        info = np.zeros(T, dtype=np.int32)
        mus_p = dptr(as_f64(mus)) if mus is not None else None
        muc_p = dptr(as_f64(np.broadcast_to(np.asarray(mu_const, dtype=float), (T,)))) if mus is None else None
        self.h.call("gpmi_lml_grad_batch_noise", kernel, T, dptr(th), nth, dptr(ex), mus_p, muc_p, dptr(nv), dptr(lml),
                    dptr(grad), dptr(trq), dptr(alpha), dptr(qdiag), info.ctypes.data_as(C.POINTER(C.c_int)))
        return lml, grad, trq, alpha, qdiag, info

    # -- prediction -------------------------------------------------------------------
    def predict(self, pts, want_var=True):
        p = as_f64(pts)
        m = p.shape[0]
        mu = np.empty(m)
        var = np.empty(m) if want_var else None
        self.h.call("gpmi_predict", dptr(p), m, dptr(mu), dptr(var))
        return mu, var

    def predict_batch(self, kernel, thetas_cov, extra_diag, pts, mus=None, mu_const=None, mu_q=None, weights=None,
                      want_var=True, want_samples=True, want_mix=True):
        """gpmi_predict_batch: prediction at `pts` under the T rows of `thetas_cov` in lockstep, and its mixture.
        mus (T, n) with mu_q (T, m) - the prior means at the data and at the points -, or mu_const (T,).
        Returns (mean_t (T, m) | None, var_t (T, m) | None, mix_mean (m,) | None, mix_var (m,) | None, info (T,));
        var_t is |a^2 - |L^-1 k|^2|, rows with info != 0 are NaN and left out of the mixture."""
        th = as_f64(np.atleast_2d(thetas_cov))
        T, nth = th.shape
        p = as_f64(pts)
        m = p.shape[0]
        ex = as_f64(np.broadcast_to(np.asarray(extra_diag, dtype=float), (T,)))
        if mus is not None:
            mus_a, muq_a, muc_a = as_f64(mus).reshape(T, self.n), as_f64(mu_q).reshape(T, m), None
        else:
            mus_a, muq_a, muc_a = None, None, as_f64(np.broadcast_to(np.asarray(mu_const, dtype=float), (T,)))
        w = None if weights is None else as_f64(weights).reshape(T)
        mean_t = np.empty((T, m)) if want_samples else None
        var_t = np.empty((T, m)) if want_samples and want_var else None
        mix_mean = np.empty(m) if want_mix else None
        mix_var = np.empty(m) if want_mix and want_var else None
        info = np.zeros(T, dtype=np.int32)
        self.h.call("gpmi_predict_batch", kernel, T, dptr(th), nth, dptr(ex), dptr(mus_a), dptr(muc_a), dptr(p), m,
                    dptr(muq_a), dptr(w), dptr(mean_t), dptr(var_t), dptr(mix_mean), dptr(mix_var),
                    info.ctypes.data_as(C.POINTER(C.c_int)))
        return mean_t, var_t, mix_mean, mix_var, info

    def posterior(self, pts, mean_only=False):
        p = as_f64(pts)
        m = p.shape[0]
        mu = np.empty(m)
        cov = None if mean_only else np.empty((m, m))
        self.h.call("gpmi_posterior", dptr(p), m, dptr(mu), dptr(cov))
        return mu, cov

    def posterior_draws(self, pts, n_draws=1, seed=0, z=None, jitter=1e-9, first_draw=0):
        """gpmi_posterior_draws: `n_draws` joint draws of the latent function at `pts` from the fitted model, without the
        mean function.  Arguments as `mvn_draws`.  Returns (draws | None, mu (m,), eps, info)."""
        p = as_f64(pts)
        m = p.shape[0]
        z = None if z is None else as_f64(z).reshape(int(n_draws), m)
        mu, draws = np.empty(m), np.empty((int(n_draws), m))
        eps, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_posterior_draws", dptr(p), m, float(jitter), int(n_draws), dptr(z), _seed_i64(seed),
                    int(first_draw), dptr(mu), dptr(draws), C.byref(eps), C.byref(info))
        return (draws if info.value == 0 else None), mu, eps.value, info.value

    def spatial_derivatives(self, pts):
        p = as_f64(pts)
        m = p.shape[0]
        dmu = np.empty((m, self.d))
        dvar = np.empty((m, self.d))
        self.h.call("gpmi_spatial_derivatives", dptr(p), m, dptr(dmu), dptr(dvar))
        return dmu, dvar

    def gradient(self, pts):
        p = as_f64(pts)
        m = p.shape[0]
        gmu = np.empty((m, self.d))
        gcov = np.empty((m, self.d, self.d))
        self.h.call("gpmi_gradient", dptr(p), m, dptr(gmu), dptr(gcov))
        return gmu, gcov

    def covariance(self, kernel, theta_cov, extra_diag=0.0, with_noise=False):
        theta = as_f64(theta_cov)
        K = np.empty((self.n, self.n))
        self.h.call("gpmi_covariance", kernel, dptr(theta), theta.size, float(extra_diag),
                    int(bool(with_noise)), dptr(K))
        return K

    def cross_covariance(self, kernel, theta_cov, pts):
        theta = as_f64(theta_cov)
        p = as_f64(pts)
        out = np.empty((p.shape[0], self.n))
        self.h.call("gpmi_cross_covariance", kernel, dptr(theta), theta.size, dptr(p), p.shape[0], dptr(out))
        return out

    def get_K(self):
        K = np.empty((self.n, self.n))
        self.h.call("gpmi_get_K", dptr(K))
        return K

    def get_L(self):
        L = np.empty((self.n, self.n))
        self.h.call("gpmi_get_L", dptr(L))
        return L

    def loo_diag(self):
        out = np.empty(self.n)
        self.h.call("gpmi_loo_diag", dptr(out))
        return out

    def loo_terms(self, kernel, theta_cov, extra_diag, mu):
        theta = as_f64(theta_cov)
        mu = as_f64(mu)
        alpha = np.empty(self.n)
        ikdiag = np.empty(self.n)
        info = C.c_int(0)
        self.h.call("gpmi_loo_terms", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    dptr(alpha), dptr(ikdiag), C.byref(info))
        return alpha, ikdiag, info.value

    def loo_grad(self, kernel, theta_cov, extra_diag, mu):
        theta = as_f64(theta_cov)
        mu = as_f64(mu)
        alpha, ikdiag, pvec = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        grad = np.empty(theta.size)
        trq = C.c_double(0.0)
        info = C.c_int(0)
        self.h.call("gpmi_loo_grad", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    dptr(alpha), dptr(ikdiag), dptr(pvec), dptr(grad), C.byref(trq), C.byref(info))
        return alpha, ikdiag, pvec, grad, trq.value, info.value

    def loo_grad_batch(self, kernel, thetas_cov, extra_diag, mus=None, mu_const=None, noise_var=None):
        """T evaluations of `loo_grad` in one call (gpmi_loo_grad_batch: lockstep for padded N <= 4096):
        (alpha (T, n), ikdiag (T, n), pvec (T, n), grad (T, n_theta), trace_q (T,), info (T,)).  With `noise_var`
        (T, n: HeteroscedasticNoise, every evaluation its own data variances; gpmi_loo_grad_batch_noise) the tuple gains
        mdiag (T, n) = diag(K^-1 diag(c2) K^-1) in front of info."""
        th = as_f64(np.atleast_2d(thetas_cov))
        T, nth = th.shape
        ex = as_f64(np.broadcast_to(np.asarray(extra_diag, dtype=float), (T,)))
        alpha, ikdiag, pvec = np.empty((T, self.n)), np.empty((T, self.n)), np.empty((T, self.n))
        grad, trq = np.empty((T, nth)), np.empty(T)
        info = np.zeros(T, dtype=np.int32)
        mus_p = dptr(as_f64(mus)) if mus is not None else None
        muc_p = dptr(as_f64(np.broadcast_to(np.asarray(mu_const, dtype=float), (T,)))) if mus is None else None
        if noise_var is not None:
            nv = as_f64(noise_var)
            assert nv.shape == (T, self.n)
            mdiag = np.empty((T, self.n))
            self.h.call("gpmi_loo_grad_batch_noise", kernel, T, dptr(th), nth, dptr(ex), mus_p, muc_p, dptr(nv), dptr(alpha),
                        dptr(ikdiag), dptr(pvec), dptr(mdiag), dptr(grad), dptr(trq), info.ctypes.data_as(C.POINTER(C.c_int)))
            return alpha, ikdiag, pvec, grad, trq, mdiag, info
        self.h.call("gpmi_loo_grad_batch", kernel, T, dptr(th), nth, dptr(ex), mus_p, muc_p, dptr(alpha), dptr(ikdiag),
                    dptr(pvec), dptr(grad), dptr(trq), info.ctypes.data_as(C.POINTER(C.c_int)))
        return alpha, ikdiag, pvec, grad, trq, info

    # -- dense entry points (covariance functions that only implement the plugin ABC) ------------------
    def fit_dense(self, K, mu):
        K, mu = as_f64(K), as_f64(mu)
        alpha = np.empty(self.n)
        logdet, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_fit_dense", dptr(K), dptr(mu), dptr(alpha), C.byref(logdet), C.byref(info))
        return alpha, logdet.value, info.value

    def lml_dense(self, K, mu, want_alpha=False, want_inverse=False):
        K, mu = as_f64(K), as_f64(mu)
        lml, info = C.c_double(0.0), C.c_int(0)
        alpha = np.empty(self.n) if want_alpha else None
        iK = np.empty((self.n, self.n)) if want_inverse else None
        self.h.call("gpmi_lml_dense", dptr(K), dptr(mu), C.byref(lml), dptr(alpha), dptr(iK), C.byref(info))
        return lml.value, alpha, iK, info.value

    def loo_dense(self, K, mu, want_gradient_pieces=False):
        K, mu = as_f64(K), as_f64(mu)
        alpha, ikdiag = np.empty(self.n), np.empty(self.n)
        pvec = np.empty(self.n) if want_gradient_pieces else None
        W = np.empty((self.n, self.n)) if want_gradient_pieces else None
        info = C.c_int(0)
        self.h.call("gpmi_loo_dense", dptr(K), dptr(mu), dptr(alpha), dptr(ikdiag), dptr(pvec), dptr(W), C.byref(info))
        return alpha, ikdiag, pvec, W, info.value

    def predict_dense(self, Kq, want_var=True):
        Kq = as_f64(Kq)
        m = Kq.shape[0]
        ka = np.empty(m)
        ss = np.empty(m) if want_var else None
        self.h.call("gpmi_predict_dense", dptr(Kq), m, dptr(ka), dptr(ss))
        return ka, ss

    def solve_rows(self, Q, want_rows=True, want_gram=False):
        Q = as_f64(Q)
        m = Q.shape[0]
        X = np.empty((m, self.n)) if want_rows else None
        G = np.empty((m, m)) if want_gram else None
        self.h.call("gpmi_solve_rows", dptr(Q), m, dptr(X), dptr(G))
        return X, G

    def solve_rows_kinv(self, Q):
        """Z = Q K^-1 for the rows of Q (m x n): the forward and the backward row solve with the fitted factor."""
        Q = as_f64(Q)
        m = Q.shape[0]
        Z = np.empty((m, self.n))
        self.h.call("gpmi_solve_rows_kinv", dptr(Q), m, dptr(Z))
        return Z

    # -- instrumentation ----------------------------------------------------------------
    def timer_start(self):
        self.h.call("gpmi_timer_start")

    def timer_stop(self):
        ms = C.c_float(0.0)
        self.h.call("gpmi_timer_stop", C.byref(ms))
        return ms.value

    def profile_enable(self, on=True):
        """True / 1: every class (HIP events around the launches: perturbs the overlap); 0: off;
        `2 << klass` (or an OR of them): only those classes — the trailing-update class PROF_SYRK is timed by
        in-kernel stamps and costs nothing."""
        self.h.call("gpmi_profile_enable", 1 if on is True else int(on))

    def profile_reset(self):
        self.h.call("gpmi_profile_reset")

    def profile_read(self, klass):
        n = C.c_int64(0)
        ms, fl, by = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        self.h.call("gpmi_profile_read", klass, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
        return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}

    def profile_clock(self):
        """Shader clock (GHz) over the stamped trailing-update launches since the last reset."""
        ghz = C.c_double(0.0)
        self.h.call("gpmi_profile_clock", C.byref(ghz))
        return ghz.value

    # -- many targets on one factorisation (gpmi_mt_*) --------------------------------------
    def mt_set_targets(self, residuals):
        """gpmi_mt_set_targets: the (n, T) residuals Y - 1 m^T, kept on the device as rows."""
        r = as_f64(residuals)
        if r.ndim != 2 or r.shape[0] != self.n:
            raise ValueError(f"residuals must be ({self.n}, T), got {r.shape}")
        self.h.call("gpmi_mt_set_targets", dptr(r), r.shape[1])
        self.mt_targets = r.shape[1]

    def _mt_values(self, name, kernel, theta_cov, extra_diag, per_target):
        theta = as_f64(theta_cov)
        lml_t = np.empty(self.mt_targets) if per_target else None
        lml, info = C.c_double(0.0), C.c_int(0)
        self.h.call(name, kernel, dptr(theta), theta.size, float(extra_diag), dptr(lml_t), C.byref(lml), C.byref(info))
        return lml.value, lml_t, info.value

    def mt_fit(self, kernel, theta_cov, extra_diag, per_target=True):
        """gpmi_mt_fit: (lml, lml_t (T,) | None, info); the factor stays in lane 0, A^T on the device."""
        return self._mt_values("gpmi_mt_fit", kernel, theta_cov, extra_diag, per_target)

    def mt_lml(self, kernel, theta_cov, extra_diag, per_target=False):
        """gpmi_mt_lml: (lml, lml_t (T,) | None, info) at other hyper-parameters; the fit is not touched."""
        return self._mt_values("gpmi_mt_lml", kernel, theta_cov, extra_diag, per_target)

    def mt_lml_grad(self, kernel, theta_cov, extra_diag):
        """gpmi_mt_lml_grad: (lml, grad (n_theta,), T * trace_q, info)."""
        theta = as_f64(theta_cov)
        grad = np.empty(theta.size + 1)
        lml, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_mt_lml_grad", kernel, dptr(theta), theta.size, float(extra_diag), C.byref(lml), dptr(grad),
                    C.byref(info))
        return lml.value, grad[:-1].copy(), float(grad[-1]), info.value

    def mt_loo_terms(self, kernel, theta_cov, extra_diag):
        """gpmi_mt_loo_terms: (a2 (n,) = sum_t A_it^2, diag K^-1 (n,), info)."""
        theta = as_f64(theta_cov)
        a2, ikdiag = np.empty(self.n), np.empty(self.n)
        info = C.c_int(0)
        self.h.call("gpmi_mt_loo_terms", kernel, dptr(theta), theta.size, float(extra_diag), dptr(a2), dptr(ikdiag),
                    C.byref(info))
        return a2, ikdiag, info.value

    def mt_alpha(self):
        """gpmi_mt_alpha: A = K^-1 R of the fit, (n, T)."""
        out = np.empty((self.n, self.mt_targets))
        self.h.call("gpmi_mt_alpha", dptr(out))
        return out

    def mt_predict(self, pts, want_var=True):
        """gpmi_mt_predict: (k(q)^T A (m, T) without the offsets, a^2 - |L^-1 k(q)|^2 (m,) | None)."""
        p = as_f64(pts)
        m = p.shape[0]
        mean = np.empty((m, self.mt_targets))
        var = np.empty(m) if want_var else None
        self.h.call("gpmi_mt_predict", dptr(p), m, dptr(mean), dptr(var))
        return mean, var

    def mt_loo(self):
        """gpmi_mt_loo: (A_it / (K^-1)_ii (n, T), diag K^-1 (n,)) of the fit."""
        resid = np.empty((self.n, self.mt_targets))
        ikdiag = np.empty(self.n)
        self.h.call("gpmi_mt_loo", dptr(resid), dptr(ikdiag))
        return resid, ikdiag

    # -- non-Gaussian likelihoods by Laplace's method (gpmi_ggp_*) ---------------------------
    def ggp_set_observations(self, likelihood, y, aux, offset):
        """gpmi_ggp_set_observations: the likelihood id, its y and per-point data (n each) and the constant prior mean."""
        y, aux = as_f64(y), as_f64(aux)
        if y.shape != (self.n,) or aux.shape != (self.n,):
            raise ValueError(f"y and aux must be ({self.n},), got {y.shape} and {aux.shape}")
        self.h.call("gpmi_ggp_set_observations", int(likelihood), dptr(y), dptr(aux), float(offset))

    def _ggp_value(self, name, kernel, theta_cov, tol, max_iter):
        theta = as_f64(theta_cov)
        logq, info, iters = C.c_double(0.0), C.c_int(0), (C.c_int * 2)(0, 0)
        self.h.call(name, kernel, dptr(theta), theta.size, float(tol), int(max_iter), C.byref(logq), iters, C.byref(info))
        return logq.value, (iters[0], iters[1]), info.value

    def ggp_fit(self, kernel, theta_cov, tol, max_iter):
        """gpmi_ggp_fit: (log q, (Newton steps, halvings), info); the factor of B at the mode stays in lane 0."""
        return self._ggp_value("gpmi_ggp_fit", kernel, theta_cov, tol, max_iter)

    def ggp_logq(self, kernel, theta_cov, tol, max_iter):
        """gpmi_ggp_logq: the same at other hyper-parameters on lane 1; the fit is not touched."""
        return self._ggp_value("gpmi_ggp_logq", kernel, theta_cov, tol, max_iter)

    def ggp_logq_grad(self, kernel, theta_cov, tol, max_iter):
        """gpmi_ggp_logq_grad: (log q, grad (n_theta,), (Newton steps, halvings), info)."""
        theta = as_f64(theta_cov)
        grad = np.zeros(theta.size)
        logq, info, iters = C.c_double(0.0), C.c_int(0), (C.c_int * 2)(0, 0)
        self.h.call("gpmi_ggp_logq_grad", kernel, dptr(theta), theta.size, float(tol), int(max_iter), C.byref(logq),
                    dptr(grad), iters, C.byref(info))
        return logq.value, grad, (iters[0], iters[1]), info.value

    def ggp_mode(self):
        """gpmi_ggp_mode: (f-hat (n,), g = grad log p(y | f-hat) (n,)) of the fit."""
        f, g = np.empty(self.n), np.empty(self.n)
        self.h.call("gpmi_ggp_mode", dptr(f), dptr(g))
        return f, g

    def ggp_predict(self, pts, want_var=True):
        """gpmi_ggp_predict: (latent mean (m,), latent variance (m,) | None)."""
        p = as_f64(pts)
        m = p.shape[0]
        mean = np.empty(m)
        var = np.empty(m) if want_var else None
        self.h.call("gpmi_ggp_predict", dptr(p), m, dptr(mean), dptr(var))
        return mean, var

    def ggp_kv(self, kernel, theta_cov, V, reps=1, timed=False):
        """gpmi_ggp_kv: K V^T row by row for 1 .. 4 vectors (rows of V) with the latent K at theta; with `timed` also
        the HIP-event milliseconds of the `reps` products."""
        theta = as_f64(theta_cov)
        V = np.atleast_2d(as_f64(V))
        if V.shape[1] != self.n:
            raise ValueError(f"V must be (nv, {self.n}), got {V.shape}")
        Y = np.empty_like(V)
        ms = C.c_float(0.0)
        self.h.call("gpmi_ggp_kv", kernel, dptr(theta), theta.size, dptr(V), V.shape[0], dptr(Y), int(reps),
                    C.byref(ms) if timed else None)
        return (Y, ms.value) if timed else Y

    def sync(self):
        self.h.call("gpmi_sync")

    def close(self):
        self.h.close()


class LinvEngine(_DrawsMixin):
    """Device side of `GpLinearInverter` (gpmi_linv_*): parameter positions, model matrix and data are
    uploaded once; every call evaluates one hyper-parameter vector."""

    def __init__(self, positions, model_matrix, y, y_err, device=None):
        self.h = _lib.Handle(device)
        self.x = as_f64(positions)
        self.n, self.d = self.x.shape
        self.A = as_f64(model_matrix)
        self.m = self.A.shape[0]
        zeros = np.zeros(self.n)
        self.h.call("gpmi_set_data", dptr(self.x), dptr(zeros), None, None, self.n, self.d)
        self.h.call("gpmi_linv_set", dptr(self.A), self.m, dptr(as_f64(y)), dptr(as_f64(y_err)))

    def lml(self, kernel, theta_cov, extra_diag, mu):
        theta, mu = as_f64(theta_cov), as_f64(mu)
        out, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_linv_lml", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    C.byref(out), C.byref(info))
        return out.value, info.value

    def lml_grad(self, kernel, theta_cov, extra_diag, mu):
        theta, mu = as_f64(theta_cov), as_f64(mu)
        lml, trq, info = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        grad, w = np.empty(theta.size), np.empty(self.n)
        self.h.call("gpmi_linv_lml_grad", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    C.byref(lml), dptr(grad), C.byref(trq), dptr(w), C.byref(info))
        return lml.value, grad, trq.value, w, info.value

    def posterior(self, kernel, theta_cov, extra_diag, mu, with_cov=True):
        theta, mu = as_f64(theta_cov), as_f64(mu)
        info = C.c_int(0)
        mean = np.empty(self.n)
        cov = np.empty((self.n, self.n)) if with_cov else None
        self.h.call("gpmi_linv_posterior", kernel, dptr(theta), theta.size, float(extra_diag), dptr(mu),
                    dptr(mean), dptr(cov), C.byref(info))
        return mean, cov, info.value

    # -- prior covariance evaluated by the caller (any CovarianceFunction object) ------------
    def _dense(self, K):
        K = as_f64(K)
        if K.shape != (self.n, self.n):
            raise ValueError(f"prior covariance must be ({self.n}, {self.n}), got {K.shape}")
        return K

    def lml_dense(self, K, mu):
        K, mu = self._dense(K), as_f64(mu)
        out, info = C.c_double(0.0), C.c_int(0)
        self.h.call("gpmi_linv_lml_dense", dptr(K), dptr(mu), C.byref(out), C.byref(info))
        return out.value, info.value

    def lml_grad_dense(self, K, mu):
        """(LML, G = A^T J^-1 A, w = A^T alpha, info): grad_j = 1/2 sum (w w^T - G) o dK_j."""
        K, mu = self._dense(K), as_f64(mu)
        lml, info = C.c_double(0.0), C.c_int(0)
        G, w = np.empty((self.n, self.n)), np.empty(self.n)
        self.h.call("gpmi_linv_lml_grad_dense", dptr(K), dptr(mu), C.byref(lml), dptr(G), dptr(w), C.byref(info))
        return lml.value, G, w, info.value

    def posterior_dense(self, K, mu, with_cov=True):
        K, mu = self._dense(K), as_f64(mu)
        info = C.c_int(0)
        mean = np.empty(self.n)
        cov = np.empty((self.n, self.n)) if with_cov else None
        self.h.call("gpmi_linv_posterior_dense", dptr(K), dptr(mu), dptr(mean), dptr(cov), C.byref(info))
        return mean, cov, info.value


SGP_SCHEDULE_FIELDS = ("panel", "m_pad", "data_run_tiles", "kmm_run_tiles", "weight_blocks", "panels")


def sgp_schedule(n, m, panel_rows=0):
    """gpmi_sgp_schedule (host only, needs no device): the size-dependent schedule of the sparse model's evaluations as a
    dict - rows of x per panel, m padded, the tiles per workgroup of the dF/dZ contraction over a data panel and over
    K_mm, the workgroups of the weights pass and the number of panels.  ValueError outside the library's ranges."""
    out = (C.c_int64 * 6)()
    if _lib.load().gpmi_sgp_schedule(int(n), int(m), int(panel_rows), out) != 0:
        raise ValueError(f"sgp_schedule: n = {n} (2 .. 2^30), m = {m} (1 .. {_lib.SGP_MAX_M}) or panel_rows = {panel_rows} "
                         "(0 .. 32768) out of range")
    return dict(zip(SGP_SCHEDULE_FIELDS, (int(v) for v in out)))


SGP_BATCH_SCHEDULE_FIELDS = ("chunk", "chunks", "bytes_per_problem", "panel", "panels", "m_pad")


def sgp_batch_schedule(n, m, d, T, panel_rows=0, want_grad=False, max_chunk=0, budget_bytes=0):
    """gpmi_sgp_batch_schedule (host only, needs no device): what `SparseEngine.bound_batch` does with T vectors as a dict -
    problems per chunk, chunks, workspace bytes per problem, rows of x per panel, panels, m padded.  budget_bytes = 0: the
    library's cap (GPMI_BATCH_GIB).  ValueError outside the library's ranges."""
    out = (C.c_int64 * 6)()
    if _lib.load().gpmi_sgp_batch_schedule(int(n), int(m), int(d), int(panel_rows), int(T), int(bool(want_grad)), int(max_chunk),
                                           int(budget_bytes), out) != 0:
        raise ValueError(f"sgp_batch_schedule: n = {n}, m = {m}, d = {d}, panel_rows = {panel_rows}, T = {T}, max_chunk = "
                         f"{max_chunk} or budget_bytes = {budget_bytes} out of range")
    return dict(zip(SGP_BATCH_SCHEDULE_FIELDS, (int(v) for v in out)))


def select_schedule(n):
    """gpmi_select_schedule (host only): the workgroups - block partials - of a selection step over n points."""
    out = (C.c_int64 * 1)()
    if _lib.load().gpmi_select_schedule(int(n), out) != 0:
        raise ValueError(f"select_schedule: n = {n} out of range (1 .. 2^30)")
    return int(out[0])


class SparseEngine:
    """One gpmi_sgp object (include/gpmi.h: the variational inducing-point model) on a handle of its own: x and the
    inducing inputs go up once, the residual and the data variances with `set_targets`; every evaluation then moves
    hyper-parameters up and a handful of numbers (and, on request, the N values of alpha) down."""

    def __init__(self, x, z, device=None):
        self.x, self.z = as_f64(x), as_f64(z)
        self.n, self.d = self.x.shape
        self.m = self.z.shape[0]
        self.h = _lib.Handle(device)
        self.ptr = C.c_void_p()
        self.h.call("gpmi_sgp_create", self.n, self.d, dptr(self.x), self.m, dptr(self.z), C.byref(self.ptr))

    def _call(self, name, *args):
        if not self.h.ctx:
            raise _lib.GpmiUnavailable("the device handle of this model has been closed")
        rc = getattr(self.h.lib, name)(self.ptr, *args)
        if rc != 0:
            raise _lib.GpmiError(f"{name} failed with status {rc}: {self.h.lib.gpmi_last_error(self.h.ctx).decode()}")

    def set_targets(self, r, noise_var=None):
        r = as_f64(r)
        nv = None if noise_var is None else as_f64(noise_var)
        self._call("gpmi_sgp_set_targets", dptr(r), dptr(nv))

    def set_inducing(self, z):
        """Replace the inducing inputs on the device (same shape, finite); a kept fit is dropped."""
        z = as_f64(z)
        if z.shape != (self.m, self.d):
            raise ValueError(f"the inducing inputs must keep their shape {(self.m, self.d)}, got {z.shape}")
        self._call("gpmi_sgp_set_inducing", dptr(z))
        self.z = z

    def bound(self, kernel, theta, white_var, jitter, panel_rows=0, want_grad=False, want_alpha=False, want_zgrad=False):
        """(F, gradient or None, alpha or None, info): info > 0 - not positive definite - leaves the rest undefined.
        want_zgrad: dF/dZ, (m, d), as a fifth element (gpmi_sgp_bound_zgrad; the other four keep their bits)."""
        theta = as_f64(theta)
        F, info = C.c_double(0.0), C.c_int(0)
        grad = np.zeros(theta.size + 1) if want_grad else None
        alpha = np.zeros(self.n) if want_alpha else None
        if want_zgrad:
            zgrad = np.zeros((self.m, self.d))
            self._call("gpmi_sgp_bound_zgrad", int(kernel), dptr(theta), theta.size, float(white_var), float(jitter),
                       int(panel_rows), C.byref(F), dptr(grad), dptr(zgrad), dptr(alpha), C.byref(info))
            return F.value, grad, alpha, info.value, zgrad
        self._call("gpmi_sgp_bound", int(kernel), dptr(theta), theta.size, float(white_var), float(jitter), int(panel_rows),
                   C.byref(F), dptr(grad), dptr(alpha), C.byref(info))
        return F.value, grad, alpha, info.value

    def set_observations(self, y, noise_var=None):
        """y itself and the data variances for `bound_batch`: they go up once and stay."""
        y = as_f64(y)
        nv = None if noise_var is None else as_f64(noise_var)
        if y.shape != (self.n,) or (nv is not None and nv.shape != (self.n,)):
            raise ValueError(f"y and noise_var must have shape ({self.n},)")
        self._call("gpmi_sgp_set_observations", dptr(y), dptr(nv))

    def bound_batch(self, kernel, thetas, white_vars, jitter, panel_rows=0, *, mu_const=None, mus=None, want_grad=False,
                    want_alpha=False, max_chunk=0):
        """gpmi_sgp_bound_batch for the T rows of `thetas`: (F (T,), gradient (T, n_theta + 1) | None, sum_alpha (T,) | None,
        alpha (T, N) | None, info (T,)).  Exactly one of mu_const (T,) and mus (T, N); sum_alpha comes with the gradient.
        A row with info > 0 did not factorise: its other entries are unspecified."""
        thetas = as_f64(np.atleast_2d(thetas))
        T, n_theta = thetas.shape
        white = as_f64(np.broadcast_to(np.asarray(white_vars, dtype=float), (T,)))
        mu_const = None if mu_const is None else as_f64(np.asarray(mu_const, dtype=float).reshape(T))
        mus = None if mus is None else as_f64(np.asarray(mus, dtype=float).reshape(T, self.n))
        F, info = np.zeros(T), np.zeros(T, dtype=np.int32)
        grad = np.zeros((T, n_theta + 1)) if want_grad else None
        sum_alpha = np.zeros(T) if want_grad else None
        alpha = np.zeros((T, self.n)) if want_alpha else None
        self._call("gpmi_sgp_bound_batch", int(kernel), T, dptr(thetas), n_theta, dptr(white), dptr(mu_const), dptr(mus),
                   float(jitter), int(panel_rows), int(max_chunk), dptr(F), dptr(grad), dptr(sum_alpha), dptr(alpha),
                   info.ctypes.data_as(C.POINTER(C.c_int)))
        return F, grad, sum_alpha, alpha, info

    def fit(self, kernel, theta, white_var, jitter, panel_rows=0):
        theta = as_f64(theta)
        F, info = C.c_double(0.0), C.c_int(0)
        self._call("gpmi_sgp_fit",int(kernel), dptr(theta), theta.size, float(white_var), float(jitter), int(panel_rows),
                   C.byref(F), C.byref(info))
        return F.value, info.value

    def predict(self, pts, want_var=True):
        pts = as_f64(pts)
        mean = np.zeros(pts.shape[0])
        var = np.zeros(pts.shape[0]) if want_var else None
        self._call("gpmi_sgp_predict", dptr(pts), pts.shape[0], dptr(mean), dptr(var))
        return mean, var

    def posterior(self, pts, mean_only=False):
        """gpmi_sgp_posterior: (mean (M,), covariance (M, M) | None) of the latent function at `pts`, without the mean
        function."""
        pts = as_f64(pts)
        m = pts.shape[0]
        mu = np.zeros(m)
        cov = None if mean_only else np.zeros((m, m))
        self._call("gpmi_sgp_posterior", dptr(pts), m, dptr(mu), dptr(cov))
        return mu, cov

    def posterior_draws(self, pts, n_draws=1, seed=0, z=None, jitter=1e-9, first_draw=0):
        """gpmi_sgp_posterior_draws: arguments and the result (draws | None, mu (M,), eps, info) as
        `GpEngine.posterior_draws`."""
        pts = as_f64(pts)
        m = pts.shape[0]
        z = None if z is None else as_f64(z).reshape(int(n_draws), m)
        mu, draws = np.zeros(m), np.zeros((int(n_draws), m))
        eps, info = C.c_double(0.0), C.c_int(0)
        self._call("gpmi_sgp_posterior_draws", dptr(pts), m, float(jitter), int(n_draws), dptr(z), _seed_i64(seed),
                   int(first_draw), dptr(mu), dptr(draws), C.byref(eps), C.byref(info))
        return (draws if info.value == 0 else None), mu, eps.value, info.value

    def spatial_derivatives(self, pts, want_var=True):
        """gpmi_sgp_spatial_derivatives: (d mean / d q (M, d), d var / d q (M, d) | None)."""
        pts = as_f64(pts)
        m = pts.shape[0]
        dmu = np.zeros((m, self.d))
        dvar = np.zeros((m, self.d)) if want_var else None
        self._call("gpmi_sgp_spatial_derivatives", dptr(pts), m, dptr(dmu), dptr(dvar))
        return dmu, dvar

    def profile_stages(self, on):
        """HIP-event timing of the four stages (GPMI_PROF_SGP_*) on or off; `stage_ms` reads and resets them."""
        mask = 0
        for k in (_lib.PROF_SGP_BUILD, _lib.PROF_SGP_GRAM, _lib.PROF_SGP_FACTOR, _lib.PROF_SGP_GRAD):
            mask |= 2 << k
        self.h.call("gpmi_profile_enable", mask if on else 0)
        self.h.call("gpmi_profile_reset")

    def stage_ms(self):
        out = {}
        for name, k in (("build", _lib.PROF_SGP_BUILD), ("gram", _lib.PROF_SGP_GRAM), ("factor", _lib.PROF_SGP_FACTOR),
                        ("grad", _lib.PROF_SGP_GRAD)):
            n = C.c_int64(0)
            ms, fl, by = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
            self.h.call("gpmi_profile_read", k, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
            out[name] = {"ms": ms.value, "flops": fl.value}
        self.h.call("gpmi_profile_reset")
        return out

    def close(self):
        if self.h.ctx and self.ptr:
            self.h.lib.gpmi_sgp_destroy(self.ptr)
        self.ptr = C.c_void_p()
        self.h.close()
