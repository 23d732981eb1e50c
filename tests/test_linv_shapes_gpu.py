"""
GPU tests of the linear-inversion pipeline (csrc/api_linv.hip) at the shapes the rest of the suite never gives it: more
data than parameters, more than one 512-wide outer block in either direction, ragged tile counts, rectangular products
on each of the three GEMM tile paths, per-datum errors.  tests/linv_host.py lists the shapes and what each is the smallest
case of; its float64 `mirror` - the same Cholesky / Woodbury formulation in SciPy - is the yardstick, and
tests/test_linv_cpu.py shows that the mirror is within 1e-11 of np.longdouble arithmetic and within 2e-11 of the LU
oracle on these very problems (cond(J) 4e4 .. 5e5).  Hence every output is held to the project's RTOL = 1e-10
(max |a - b| / max |b| per array), tighter than the 2e-9 / 2e-10 that test_linear_inverter_vs_reference has to grant the
LU side; gradient and w = A^T alpha also element by element (check_each).  n x n outputs are compared in full and a
failure names the 128 x 128 tiles that are off.  Every comparison is logged with tests/test_gpu_parity.py's `check`, so
the achieved errors appear in the end-of-run list.

Further: the dense entry points (K uploaded, G downloaded at a pitch), independence of the order of calls (bit for bit),
the failure path (info != 0 -> LinAlgError, the handle stays good) and the re-use of one handle for a smaller problem.
"""
import ctypes as C

import numpy as np
import pytest

import linv_host as lh
from test_gpu_parity import RTOL, _record, check, check_each, rel

pytestmark = pytest.mark.gpu

assert RTOL == lh.RTOL
CASE_D = ("D", "se", False, False)
CASE_F = ("F", "se", False, False)


def make_inverter(c):
    from inference_amd import gp

    cov = {"se": gp.SquaredExponential, "rq": gp.RationalQuadratic, "m52": gp.Matern52}[c.kind]()
    if c.white:
        cov = cov + gp.WhiteNoise()
    gli = gp.GpLinearInverter(y=c.y, y_err=c.y_err, model_matrix=c.A, parameter_spatial_positions=c.pos,
                              prior_covariance_function=cov,
                              prior_mean_function=gp.LinearMean() if c.linear else gp.ConstantMean())
    assert gli._dense is False and gli.n_hyperpars == c.theta.size
    return gli


def check_matrix(got, want, what=""):
    """`check` for an n x n output, compared in full; the failure message names the tiles."""
    r = rel(got, want)
    _record(what, r, RTOL)
    if not r <= RTOL:
        raise AssertionError("\n".join([f"{what}: relative error {r:.3e} > {RTOL:.1e}"]
                                       + lh.tile_report(got, want, RTOL, what)))
    return r


class Comparisons:
    """Runs every comparison of a case before failing, so that one failure message carries all outputs that are off -
    the tiles of the n x n ones included - and prints the case's achieved errors as one line."""

    def __init__(self, tag):
        self.tag, self.rows, self.failures = tag, [], []

    def add(self, label, fn, got, want, what):
        try:
            self.rows.append((label, fn(got, want, what=f"{self.tag} {what}")))
        except AssertionError as err:
            self.rows.append((label, float("nan")))
            self.failures.append(str(err))

    def finish(self):
        print(f"{self.tag:14s} " + "  ".join(f"{k} {v:.1e}" for k, v in self.rows))
        assert not self.failures, "\n".join([f"{self.tag}: {len(self.failures)} comparisons failed"] + self.failures)


# ------------------------------------------------------------------------------------------------- a) shape sweep
@pytest.mark.parametrize("case", lh.CASES, ids=lh.case_id)
def test_shape_against_the_mirror(case):
    c = lh.build_case(case)
    gli = make_inverter(c)
    ref = c.ref
    cmp = Comparisons(lh.case_id(case))
    cmp.add("lml", check, gli.marginal_likelihood(c.theta), ref["lml"], "lml")
    lml, grad = gli.marginal_likelihood_gradient(c.theta)
    cmp.add("lml2", check, lml, ref["lml"], "lml (gradient call)")
    assert grad.shape == c.grad.shape
    cmp.add("grad(each)", check_each, grad, c.grad, "lml gradient")
    mean, cov = gli.calculate_posterior(c.theta)
    cmp.add("mean", check, mean, ref["mean"], "posterior mean")
    cmp.add("cov", check_matrix, cov, ref["cov"], "posterior covariance")
    cmp.add("mean only", check, gli.calculate_posterior_mean(c.theta), ref["mean"], "posterior mean only")
    # engine level: w = A^T alpha and trace_q = sum_a (w_a^2 - G_aa) never reach the caller on their own
    theta_stat, extra = gli._device_args(c.theta)
    lml, g_stat, trace_q, w, info = gli.engine.lml_grad(gli._kernel_id, theta_stat, extra, c.mu)
    assert info == 0
    cmp.add("w(each)", check_each, w, ref["w"], "w = A^T alpha")
    cmp.add("trace_q", check, trace_q, ref["trace_q"], "trace_q")
    cmp.add("g_stat", check, g_stat, ref["grad"][:len(theta_stat)], "gradient of the stationary kernel")
    cmp.finish()


# ---------------------------------------------------------------------------------------- b) dense entry points
@pytest.mark.parametrize("case", [CASE_D, CASE_F], ids=lh.case_id)
def test_dense_entry_points_against_the_mirror(case):
    """K goes up and G = A^T J^-1 A and the covariance come down through 2-D copies at pitch ld against n (300 in 384
    columns, 700 in 768)."""
    c = lh.build_case(case)
    engine = make_inverter(c).engine
    ref = c.ref
    cmp = Comparisons(lh.case_id(case) + " dense")
    lml, info = engine.lml_dense(c.K, c.mu)
    assert info == 0
    cmp.add("lml", check, lml, ref["lml"], "lml")
    lml, G, w, info = engine.lml_grad_dense(c.K, c.mu)
    assert info == 0
    cmp.add("lml2", check, lml, ref["lml"], "lml (gradient call)")
    cmp.add("G", check_matrix, G, ref["G"], "G = A^T J^-1 A")
    cmp.add("w(each)", check_each, w, ref["w"], "w = A^T alpha")
    mean, cov, info = engine.posterior_dense(c.K, c.mu)
    assert info == 0
    cmp.add("mean", check, mean, ref["mean"], "posterior mean")
    cmp.add("cov", check_matrix, cov, ref["cov"], "posterior covariance")
    mean, none, info = engine.posterior_dense(c.K, c.mu, with_cov=False)
    assert info == 0 and none is None
    cmp.add("mean only", check, mean, ref["mean"], "posterior mean only")
    cmp.finish()


# ------------------------------------------------------------------------------------ c) order of calls, d) failure
METHODS = {
    "lml": lambda gli, th: np.array(gli.marginal_likelihood(th)),
    "grad": lambda gli, th: np.hstack(gli.marginal_likelihood_gradient(th)),
    "post": lambda gli, th: np.concatenate([a.ravel() for a in gli.calculate_posterior(th)]),
    "mean": lambda gli, th: gli.calculate_posterior_mean(th),
}


@pytest.fixture(scope="module")
def d_bits():
    """(case D, an inverter, the outputs of its four methods at the case's theta as first computed by a fresh inverter)"""
    c = lh.build_case(CASE_D)
    gli = make_inverter(c)
    return c, gli, {name: METHODS[name](gli, c.theta) for name in ("lml", "grad", "post", "mean")}


def same_bits(got, want, what):
    assert np.array_equal(got, want), f"{what}: bits differ, relative difference {rel(got, want):.3e}"


def test_outputs_do_not_depend_on_the_preceding_call(d_bits):
    """The entry points overwrite one another's operands (the gradient leaves J^-1 in J and A^T J^-1 A in K, the posterior
    its covariance in K, inv2 is shared): each output at theta must come out bit for bit whatever ran before it, and
    from a second inverter whose lazily allocated buffers (J2 / inv2 / Q / X) are created in another order."""
    c, gli, base = d_bits
    other = c.theta + np.array([0.05, -0.2, 0.15, -0.1])
    for name in ("mean", "post", "grad", "lml"):  # the reverse of the order of the fixture
        same_bits(METHODS[name](gli, c.theta), base[name], f"{name} in reverse order")
    for before, at, name in [("grad", c.theta, "lml"), ("post", other, "grad"), ("grad", other, "mean"),
                             ("grad", other, "post"), ("post", other, "lml"), ("lml", other, "post"),
                             ("mean", other, "grad"), ("post", c.theta, "mean")]:
        METHODS[before](gli, at)
        same_bits(METHODS[name](gli, c.theta), base[name], f"{name} after {before}")
    fresh = make_inverter(c)
    for name in ("post", "mean", "grad", "lml"):  # the posterior first: Q / X / inv2 before J2
        same_bits(METHODS[name](fresh, c.theta), base[name], f"{name} of a second inverter")


def test_non_finite_prior_raises_and_the_handle_stays_good(d_bits):
    """A NaN amplitude makes every entry of J NaN: no pivot is positive, info reports it (the library's designed path for
    an arithmetic failure, as in test_cholesky_failure_sentinel) and every method raises LinAlgError like the reference's
    Cholesky; the next good evaluation gives the recorded bits."""
    c, gli, base = d_bits
    bad = c.theta.copy()
    bad[1] = np.nan  # ln a
    for name in ("lml", "grad", "post", "mean"):
        with pytest.raises(np.linalg.LinAlgError):
            METHODS[name](gli, bad)
    theta_stat, extra = gli._device_args(bad)
    engine = gli.engine
    infos = [engine.lml(gli._kernel_id, theta_stat, extra, c.mu)[-1],
             engine.lml_grad(gli._kernel_id, theta_stat, extra, c.mu)[-1],
             engine.posterior(gli._kernel_id, theta_stat, extra, c.mu, with_cov=True)[-1],
             engine.posterior(gli._kernel_id, theta_stat, extra, c.mu, with_cov=False)[-1],
             engine.lml_dense(np.full((c.n, c.n), np.nan), c.mu)[-1]]
    print("info:", infos)
    for info in infos:
        assert 1 <= info <= c.m
    for name in ("lml", "grad", "post", "mean"):
        same_bits(METHODS[name](gli, c.theta), base[name], f"{name} after a failed evaluation")


# ------------------------------------------------------------------------------------- e) one handle, two problems
def test_handle_reuse_for_a_smaller_problem():
    """gpmi_linv_set on a handle that already holds a larger problem releases and re-creates every buffer (and forgets the
    size of the gradient workspace): the likelihood and gradient of the smaller problem equal those of a fresh handle bit
    for bit.  A new gpmi_set_data drops the inversion problem, and the next evaluation says so."""
    from inference_amd import _lib
    from inference_amd._lib import as_f64, dptr

    c = lh.build_case(CASE_D)
    rows = 140  # A' = the first 140 data of D on the same 300 positions: (mt, nt) = (2, 3) after (7, 3)
    A2, y2, e2 = as_f64(c.A[:rows]), as_f64(c.y[:rows]), as_f64(c.y_err[:rows])
    x, zeros, mu = as_f64(c.pos), np.zeros(c.n), as_f64(c.mu)
    theta = as_f64(c.theta[1:])

    def set_data(h):
        h.call("gpmi_set_data", dptr(x), dptr(zeros), None, None, c.n, c.d)

    def evaluate(h):
        lml, lml2, trq, info = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.c_int(-1)
        h.call("gpmi_linv_lml", _lib.KERNEL_SE, dptr(theta), theta.size, 0.0, dptr(mu), C.byref(lml), C.byref(info))
        assert info.value == 0
        grad, w = np.empty(theta.size), np.empty(c.n)
        h.call("gpmi_linv_lml_grad", _lib.KERNEL_SE, dptr(theta), theta.size, 0.0, dptr(mu), C.byref(lml2), dptr(grad),
               C.byref(trq), dptr(w), C.byref(info))
        assert info.value == 0
        return np.concatenate([[lml.value, lml2.value, trq.value], grad, w])

    used, fresh = _lib.Handle(), _lib.Handle()
    try:
        set_data(used)
        used.call("gpmi_linv_set", dptr(as_f64(c.A)), c.m, dptr(as_f64(c.y)), dptr(as_f64(c.y_err)))
        big = evaluate(used)
        check(big[0], c.ref["lml"], what="D lml through the C entry points")
        used.call("gpmi_linv_set", dptr(A2), rows, dptr(y2), dptr(e2))
        set_data(fresh)
        fresh.call("gpmi_linv_set", dptr(A2), rows, dptr(y2), dptr(e2))
        want = evaluate(fresh)
        same_bits(evaluate(used), want, "smaller problem on a used handle")
        small = lh.mirror(A2, c.K, c.dK, y2, e2, c.mu)
        check(want[0], small["lml"], what="A' lml")
        check_each(want[3:3 + theta.size], small["grad"], what="A' gradient of the kernel parameters")
        # a new data set: the inversion problem is gone
        set_data(used)
        lml, info = C.c_double(0.0), C.c_int(0)
        rc = used.lib.gpmi_linv_lml(used.ctx, _lib.KERNEL_SE, dptr(theta), theta.size, 0.0, dptr(mu), C.byref(lml),
                                    C.byref(info))
        assert rc == -1  # GPMI_ERR_ARG
        assert "gpmi_linv_set has not been called" in used.lib.gpmi_last_error(used.ctx).decode()
        # ... and the handle takes the problem again
        used.call("gpmi_linv_set", dptr(A2), rows, dptr(y2), dptr(e2))
        same_bits(evaluate(used), want, "smaller problem after a new data set")
    finally:
        used.close()
        fresh.close()
