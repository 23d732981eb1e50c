"""
The host mirror of the linear-inversion pipeline (tests/linv_host.py) earns, without a GPU, the tolerance that
tests/test_linv_shapes_gpu.py holds the device to (RTOL = 1e-10, max |a - b| / max |b| per array): the reference's own
error has to sit well inside it.

  * float64 mirror against the np.longdouble mirror (column Cholesky and substitutions written out in NumPy):
    <= RTOL / 10 at the shapes a longdouble pass can afford (A, B, C, F; 0.2 .. 1.5 s each).  Measured <= 1.6e-12 for
    lml, gradient, posterior mean and covariance, <= 4.7e-12 for the intermediates w, G and trace_q.
  * float64 mirror against OracleLinearInverter - the reference's LU formulation, another algorithm - at every shape:
    <= RTOL / 5.  Measured <= 8.3e-12; the worst is the posterior mean, and that distance is the LU side's: where the
    longdouble pass runs, the mirror's mean is within 3.3e-13 of it and 2e-12 .. 8e-12 from the oracle's.  That is why
    the GPU tests use the mirror and can be tighter than the 2e-9 / 2e-10 of test_linear_inverter_vs_reference.
  * cond(J) < 1e6 for every case, so that a later change of the generator cannot silently make the problems
    ill-conditioned.

The two caps are conditions on the inputs: if a new shape or kernel breaks one, change the problem, not the cap.
"""
import numpy as np
import pytest

import kernel_host as kh
import linv_host as lh
from oracle import gp_oracle as orc
from oracle.linv_oracle import OracleLinearInverter

ORACLE_CASES = [c for c in lh.CASES if c[1] in ("se", "rq") and not c[3]]  # the oracle has a constant mean, SE and RQ
LONGDOUBLE_CASES = [c for c in lh.CASES if c[0] in lh.LONGDOUBLE_SHAPES]


def report(case, what, r, cap):
    print(f"{lh.case_id(case):14s} {what:28s} {r:9.2e} (cap {cap:.0e})")
    assert r <= cap, f"{lh.case_id(case)} {what}: {r:.3e} > {cap:.1e}"


@pytest.mark.parametrize("case", lh.CASES, ids=lh.case_id)
def test_problems_are_well_conditioned(case):
    c = lh.build_case(case)
    assert c.A.shape == (c.m, c.n) and c.pos.shape == (c.n, c.d) and c.y.shape == c.y_err.shape == (c.m,)
    np.testing.assert_allclose(c.A.sum(axis=1), 1.0, rtol=1e-13)
    assert c.y_err.min() >= 0.02 and c.y_err.max() <= 0.1 and (c.m == 1 or np.ptp(c.y_err) > 0.0)
    cond = lh.cond_J(c.A, c.K, c.y_err)
    print(f"{lh.case_id(case):14s} cond(J) = {cond:.2e}")
    assert cond < lh.COND_CAP
    for value in c.ref.values():
        assert np.all(np.isfinite(value))


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lh.case_id)
def test_mirror_against_the_lu_oracle(case):
    c = lh.build_case(case)
    oracle = OracleLinearInverter(c.y, c.y_err, c.A, c.pos, orc.SE if c.kind == "se" else orc.RQ, white_noise=c.white)
    report(case, "lml", lh.rel(c.ref["lml"], oracle.marginal_likelihood(c.theta)), lh.CAP_ORACLE)
    lml, grad = oracle.marginal_likelihood_gradient(c.theta)
    report(case, "lml (gradient call)", lh.rel(c.ref["lml"], lml), lh.CAP_ORACLE)
    report(case, "gradient", lh.rel(c.grad, grad), lh.CAP_ORACLE)
    mean, cov = oracle.calculate_posterior(c.theta)
    report(case, "posterior mean", lh.rel(c.ref["mean"], mean), lh.CAP_ORACLE)
    report(case, "posterior covariance", lh.rel(c.ref["cov"], cov), lh.CAP_ORACLE)
    # calculate_posterior_mean solves the LU system for K u instead of multiplying the solved covariance by u and lands
    # two to five times further from the mirror (up to 2.3e-11): the oracle's second route, not an output of the mirror
    only = lh.rel(c.ref["mean"], oracle.calculate_posterior_mean(c.theta))
    print(f"{lh.case_id(case):14s} {'posterior mean only':28s} {only:9.2e} (not asserted)")


@pytest.mark.skipif(not kh.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 here")
@pytest.mark.parametrize("case", LONGDOUBLE_CASES, ids=lh.case_id)
def test_mirror_against_longdouble(case):
    c = lh.build_case(case)
    wide = lh.mirror(c.A, c.K, c.dK, c.y, c.y_err, c.mu, dtype=np.longdouble)
    for key in ("lml", "grad", "trace_q", "w", "G", "mean", "cov"):
        # trace_q and G feed the gradient; they get the cap of the outputs they are part of
        report(case, key, lh.rel(c.ref[key], wide[key]), lh.CAP_LONGDOUBLE)
    report(case, "gradient", lh.rel(c.grad, lh.full_gradient(wide, c.dmu)), lh.CAP_LONGDOUBLE)


def test_mirror_gradient_is_the_derivative_of_its_lml():
    """Central differences of the mirror's own lml along every hyper-parameter (shape A, RQ + white noise + linear mean
    so that every kind of entry is present): the assembly of the gradient, not its rounding, is what this pins."""
    sid, kind, white, linear = "A", "rq", True, True
    m, n, d = lh.SHAPES[sid]
    pos, A, y, y_err = lh.shape_problem(sid)
    theta = lh.theta_for(d, kind, white, linear)
    nm = lh.n_mean_params(d, linear)

    def lml(t):
        mu, _ = lh.prior_mean(pos, t[:nm], linear)
        K, dK = lh.prior(kind, pos, t[nm:], white)
        return lh.mirror(A, K, dK, y, y_err, mu)["lml"]

    mu, dmu = lh.prior_mean(pos, theta[:nm], linear)
    K, dK = lh.prior(kind, pos, theta[nm:], white)
    grad = lh.full_gradient(lh.mirror(A, K, dK, y, y_err, mu), dmu)
    h = 1e-5
    fd = np.array([(lml(theta + h * e) - lml(theta - h * e)) / (2 * h) for e in np.eye(theta.size)])
    assert lh.rel(grad, fd) < 1e-6, (grad, fd)
    ref = lh.mirror(A, K, dK, y, y_err, mu)
    assert ref["trace_q"] == pytest.approx(grad[-1] / np.exp(2 * theta[-1]), rel=1e-12)  # dK = 2 s^2 I


def test_tile_report_names_the_tiles():
    want = np.ones((300, 300))
    got = want.copy()
    assert lh.tile_report(got, want, what="cov") == []
    got[130, 5] += 1e-9
    got[299, 260] = np.nan
    lines = lh.tile_report(got, want, what="cov")
    assert "2 of 9 tiles" in lines[0] and "tile rows [1, 2]" in lines[0] and "tile columns [0, 2]" in lines[0]
    assert lines[1].startswith("tile (1, 0): 1 entries") and "[130, 5]" in lines[1]
    assert lines[2].startswith("tile (2, 2): 1 entries") and "[299, 260]" in lines[2]
