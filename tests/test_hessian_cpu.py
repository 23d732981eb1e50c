"""
CPU tests of the Hessian mirror (tests/hessian_host.py): its second-derivative profiles against fourth-order central
differences of an INDEPENDENT gradient - `oracle.gp_oracle.OracleGp` for SquaredExponential / RationalQuadratic, the
oracle of tests/matern_host.py for Matern32 / Matern52 - with WhiteNoise, ConstantMean and LinearMean; symmetry, the
zero noise row at sigma^2 = 0, finite values on duplicated points.  No GPU is needed.

The oracles have a constant mean; a LinearMean is given to them as data: y - (the linear part), and the gradient by the
slopes is Phi alpha with the oracle's own alpha.
"""
import numpy as np
import pytest

import hessian_host as hh
import matern_host as mh
from oracle import gp_oracle as orc

H_STEP = 1e-3
N, D = 48, 2

# kind -> (oracle, white noise, linear mean)
CASES = {"se_wn_const": ("se", True, False), "se_linear": ("se", False, True), "rq_wn_const": ("rq", True, False),
         "rq_linear": ("rq", False, True), "m32_wn_linear": ("m32", True, True), "m52_wn_const": ("m52", True, False),
         "m52_linear": ("m52", False, True)}


def dataset(n=N, d=D, seed=3, duplicate=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 2.0, (n, d))
    if duplicate:
        x[1::2] = x[0::2][: len(x[1::2])]
    y = np.sin(2.0 * x[:, 0]) + 0.4 * x.sum(axis=1) + 0.1 * rng.standard_normal(n)
    return x, y, np.full(n, 0.1)


def features(x, linear):
    cols = [np.ones(len(x))]
    if linear:
        cols.extend((x - x.mean(axis=0)).T)
    return np.array(cols)


def theta_for(kind, d, wn, linear):
    mean = [0.3] + ([0.2, -0.1][:d] if linear else [])
    kern = [0.1] + ([0.5] if kind == "rq" else []) + list(np.log(np.linspace(0.6, 0.9, d)))
    return np.array(mean + kern + ([np.log(0.15)] if wn else []))


class Independent:
    """LML and gradient at theta = [mean, kernel, (ln sigma)] from an oracle with a constant mean."""

    def __init__(self, kind, x, y, e, wn, phi):
        self.kind, self.x, self.y, self.e, self.wn, self.phi = kind, x, y, e, wn, phi
        self.n_mean = len(phi)
        if kind in ("m32", "m52"):
            self.model = mh.HostModel([(kind,)] + ([("wn",)] if wn else []), x)

    def _oracle(self, theta):
        m = theta[: self.n_mean]
        th = np.concatenate([m[:1], theta[self.n_mean:]])
        ys = self.y - m[1:] @ self.phi[1:]
        if self.kind in ("se", "rq"):
            o = orc.OracleGp(self.x, ys, self.e, kernel=orc.SE if self.kind == "se" else orc.RQ, white_noise=self.wn, hyperpars=th)
        else:
            o = mh.OracleGp(self.x, ys, self.e, self.model, th)
        return o, th

    def lml(self, theta):
        o, th = self._oracle(theta)
        return o.marginal_likelihood(th)

    def grad(self, theta):
        o, th = self._oracle(theta)
        g = o.marginal_likelihood_gradient(th)[1]
        return np.concatenate([g[:1], self.phi[1:] @ o.alpha, g[1:]])


def fd4(f, theta, j, h):
    e = np.zeros(theta.size)
    e[j] = h
    return (-f(theta + 2 * e) + 8 * f(theta + e) - 8 * f(theta - e) + f(theta - 2 * e)) / (12 * h)


def mirror(kind, x, y, e, theta, phi, wn, **kw):
    n_mean = len(phi)
    tk = theta[n_mean: len(theta) - (1 if wn else 0)]
    return hh.hessian(kind, x, y, e**2, theta[:n_mean], phi, tk, ln_sigma=theta[-1] if wn else None, **kw)


def assert_mirror_matches_differences(name, kind, x, y, e, theta, phi, wn):
    """The comparison of `test_mirror_against_differences_of_an_independent_gradient` on given inputs."""
    ind = Independent(kind, x, y, e, wn, phi)
    g0 = ind.grad(theta)
    ref_err = float(np.abs(np.array([fd4(ind.lml, theta, j, H_STEP) for j in range(theta.size)]) - g0).max() / np.abs(g0).max())
    m = mirror(kind, x, y, e, theta, phi, wn)
    assert np.abs(m["grad"] - g0).max() <= 1e-9 * np.abs(g0).max()
    H_fd = np.array([fd4(ind.grad, theta, j, H_STEP) for j in range(theta.size)]).T  # column j: d grad / d theta_j
    err = float(np.abs(H_fd - m["H"]).max() / m["scale"].max())
    per_entry = float((np.abs(H_fd - m["H"]) / m["scale"]).max())
    own = float((np.abs(H_fd - H_fd.T) / m["scale"]).max())
    print(f"{name}: mirror vs differenced gradient {err:.2e} of the largest sum |terms|; the scheme on the oracle's own LML / "
          f"gradient {ref_err:.2e}; allowance {10 * ref_err:.2e}.  Entry by entry: {per_entry:.2e}, the differenced gradient "
          f"against its own transpose {own:.2e}")
    assert err <= 10 * ref_err
    ml = mirror(kind, x, y, e, theta, phi, wn, dtype=np.longdouble)
    assert (np.abs(np.asarray(ml["H"], dtype=float) - m["H"]) / m["scale"]).max() < 1e-9


@pytest.mark.parametrize("name", sorted(CASES))
def test_mirror_against_differences_of_an_independent_gradient(name):
    """Allowance: ten times what the same difference scheme at the same step leaves between the oracle's LML and its own
    gradient.  Both sides in the same norm, the one of tests/test_multitarget_cpu.py: the largest deviation over the
    largest magnitude - for the gradient max |g_j|, for the Hessian the largest sum |T1| + |T2| + |T3| of an entry.
    Measured at h = 1e-3 (N = 48, d = 2): the scheme on the oracles 2e-12 .. 3e-11, the mirror 1e-12 .. 8e-12, 0.3 to 1.5
    times the oracle's figure (every case prints its own).  (Entry by entry, relative to that entry's own sum of terms, the differenced gradient
    disagrees with ITS OWN transpose by 1e-10 .. 3e-9 - the rounding of the oracle's explicit K^-1 divided by h - and
    with the mirror by as much; that figure is printed and not asserted.)"""
    kind, wn, linear = CASES[name]
    x, y, e = dataset()
    phi = features(x, linear)
    theta = theta_for(kind, D, wn, linear)
    assert_mirror_matches_differences(name, kind, x, y, e, theta, phi, wn)


@pytest.mark.parametrize("name", ["rq_wn_134x22", "rq_wn_70x64"])
def test_mirror_at_the_wide_pair_table_shapes(name):
    """The two RationalQuadratic + WhiteNoise shapes of tests/test_hessian_gpu.py with 22 and 64 length scales (253 sums in
    the length-scale block; 67 parameters in the pair table), on that file's own inputs: the same comparison, the same
    allowance."""
    import test_hessian_gpu as device_cases

    kind, x, y, e, theta, wn, linear = device_cases.case_inputs(name)
    assert kind == "rq" and wn and not linear and theta.size == x.shape[1] + 4
    assert_mirror_matches_differences(name, kind, x, y, e, theta, features(x, linear), wn)


@pytest.mark.parametrize("kind", ["se", "rq", "m32", "m52"])
def test_symmetry_and_terms(kind):
    x, y, e = dataset()
    phi = features(x, True)
    theta = theta_for(kind, D, True, True)
    m = mirror(kind, x, y, e, theta, phi, True)
    assert np.array_equal(m["H"], m["H"].T)
    assert np.allclose(m["T1"] + m["T2"] + m["T3"], m["H"], rtol=0, atol=0)


def test_noise_row_vanishes_without_noise():
    """sigma^2 -> 0: the ln sigma row and column of H are proportional to sigma^2 (and its square)."""
    x, y, e = dataset()
    phi = features(x, False)
    theta = theta_for("se", D, True, False)
    theta[-1] = -400.0  # sigma^2 = e^-800 = 0 in double precision
    m = mirror("se", x, y, e, theta, phi, True)
    assert np.all(m["H"][-1] == 0.0) and np.all(m["H"][:, -1] == 0.0) and m["grad"][-1] == 0.0
    without = mirror("se", x, y, e, theta[:-1], phi, False)
    assert np.array_equal(m["H"][:-1, :-1], without["H"])


def test_duplicated_points_are_finite_for_matern32():
    x, y, e = dataset(duplicate=True)
    assert np.array_equal(x[0], x[1])
    phi = features(x, False)
    theta = theta_for("m32", D, False, False)
    for dtype in (np.float64, np.longdouble):
        m = mirror("m32", x, y, e, theta, phi, False, dtype=dtype)
        assert np.isfinite(np.asarray(m["H"], dtype=float)).all() and np.isfinite(np.asarray(m["T1"], dtype=float)).all()


def test_header_and_ctypes_agree_on_the_entry_point():
    import os
    import re

    from inference_amd import _lib

    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    header = open(os.path.join(root, "include", "gpmi.h")).read()
    proto = re.search(r"int gpmi_lml_hessian\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["gpmi_lml_hessian"][1]) == 12
    assert "gpmi_lml_hessian_alpha" in _lib.SIGNATURES
