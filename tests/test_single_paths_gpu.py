"""
GPU tests of the single-evaluation entry points (one problem on one lane: csrc/api_single.hip) and of the fitted lane's
queries: the places where an entry point can read another work vector than the one it means (the lane's slots v / alpha
/ slot 2 / mu, the four leave-one-out vectors in front of the contraction's partial sums), the seam between two
2048-row chunks of a predict, and the `fitted` / `fit_params.kernel` / `mix_nk` flags the entry points leave behind.

The shape is the smallest that has two of everything: n = 130, d = 2, hence np = 256 - two diagonal blocks, two steps
per sweep and a ragged last tile.  y_err = 0.1, theta from tests/matern_host.py's `theta_for`, a constant prior mean of
0.1, fresh handles per case, the engine's own methods (one C call each).

One theta goes through every entry point of a build - kernels (gpmi_fit, gpmi_lml, gpmi_lml_grad, gpmi_loo_terms,
gpmi_loo_grad, gpmi_loo_diag), mixture (gpmi_fit_mix, gpmi_lml_mix, gpmi_lml_grad_mix, gpmi_loo_terms_mix), dense
(gpmi_fit_dense, gpmi_lml_dense, gpmi_loo_dense) - and what they have in common is compared: a wrong slot gives another
vector, not a rounding difference.

Which pairs are bit-identical was read off a run of this file against the library of the commit before the lane
pipeline (every `pair` prints whether its two sides have equal bits); those pairs assert np.array_equal (`bits=True`):
  * alpha of fit / lml_grad / loo_terms / loo_grad, of fit_mix / lml_grad_mix / loo_terms_mix, of fit_dense / lml_dense /
    loo_dense: the same build, factorisation and sweeps;
  * LML of lml against lml_grad, of lml_mix against lml_grad_mix, log-determinant of the fit against them;
  * diag K^-1 of loo_terms / loo_grad / loo_diag (and the dense and mixture counterparts): one row-norm kernel on one L^-T;
  * alpha, log-determinant, LML and diag K^-1 of the three builds of one matrix against each other (kernels, a mixture of
    one sub-kernel with unit weights, gpmi_covariance's matrix handed over dense; ChangePoint against its matrix assembled
    on the host): the builds give the same matrix to the last bit, and everything behind them is shared;
  * a predict's rows 0, 2047, 2048 of m = 2049 against calls of their own; posterior mean against predict mean;
    posterior_draws' mean against posterior's; the posterior covariance against its transpose.
The others carry the tolerance tests/test_gpu_parity.py uses for the quantity: single against single 1e-12 (LML, alpha and
the vectors formed like it), 1e-11 (gradients), 1e-10 against the NumPy mirror of tests/matern_host.py.  The diagonal of a
posterior covariance against a predict's variance: both are K_qq - sum_k q_k^2 over np = 256 terms, summed in another
order (GEMM tile against row reduction): at most 256 eps sum q^2 <= 6e-14 a^2, relative to the largest variance ~ a^2 -
the single-against-single 1e-12 covers it.  Every comparison prints its achieved error.
"""
import numpy as np
import pytest

import matern_host as mh

pytestmark = pytest.mark.gpu

N, D = 130, 2
MEAN = 0.1
WN = 0.15  # WhiteNoise sigma of the mixture
CP = (2.0, 0.5)  # location and width of the ChangePoint window (axis 0)


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def pair(a, b, tol, what, bits=False):
    """a against b: bit for bit where the commit before the lane pipeline gives equal bits (bits=True), else within tol."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    r = rel(a, b)
    equal = bool(np.array_equal(a, b))
    print(f"{what}: {r:.2e} (tol {tol:.0e}){' bit-identical' if equal else ''}{' [bits required]' if bits else ''}")
    if bits:
        assert equal, f"{what}: not bit-identical (relative difference {r:.3e}, {int((a != b).sum())} of {a.size} elements)"
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"


def _engine():
    from inference_amd._engine import GpEngine

    x, y, e = mh.dataset(N, D)
    g = GpEngine(x, y, noise_var=e**2)
    assert g.capacity() == 256
    return g


def _kernel_form(name):
    """(kernel id, covariance parameters, the components' ids of a sum or None, oracle parts)"""
    from inference_amd import _lib

    if name == "se":
        return _lib.KERNEL_SE, mh.theta_for("se", D, 0), None, [("se",)]
    rq = mh.theta_for("rq", D, 1)
    rq[0] -= 0.3
    return _lib.KERNEL_SUM, np.concatenate([mh.theta_for("se", D, 0), rq]), [_lib.KERNEL_SE, _lib.KERNEL_RQ], [("se",), ("rq",)]


def _kernel_engine(name):
    kern, theta, comps, parts = _kernel_form(name)
    g = _engine()
    if comps:
        g.set_sum(comps)
    return g, kern, theta, parts


def _window(xa):
    return 1.0 / (1.0 + np.exp(-(xa - CP[0]) / CP[1]))


def _mix_form(x):
    """ChangePoint[SE, SE] along axis 0 + WhiteNoise: (kernel ids, sub-kernel parameters, weights (2, n), extra diagonal)"""
    from inference_amd import _lib

    f = _window(x[:, 0])
    return [_lib.KERNEL_SE, _lib.KERNEL_SE], [mh.theta_for("se", D, 0), mh.theta_for("se", D, 10)], np.array([1.0 - f, f]), WN**2


MIX_PARTS = [("cp", ("se", "se"), 0), ("wn",)]


def _mix_theta():
    return np.concatenate([[MEAN], mh.theta_for("se", D, 0), mh.theta_for("se", D, 10), CP, [np.log(WN)]])


def _oracle(parts, theta_cov):
    x, y, e = mh.dataset(N, D)
    return mh.OracleGp(x, y, e, mh.HostModel(parts, x), np.concatenate([[MEAN], theta_cov]))


def _oracle_ikdiag(o):
    return np.diag(o._factor(o.theta, False)[1])


MU = np.full(N, MEAN)


# ------------------------------------------------------------------------------------------------------- vector slots
@pytest.mark.parametrize("form", ["se", "se+rq"])
def test_kernel_build_one_theta_through_every_single_entry_point(form):
    g, kern, theta, parts = _kernel_engine(form)
    o = _oracle(parts, theta)
    a_fit, logdet, info = g.fit(kern, theta, 0.0, MU)
    assert info == 0
    ik_diag = g.loo_diag()
    lml, info = g.lml(kern, theta, 0.0, MU)
    assert info == 0
    lml_g, grad, trq, a_grad, info = g.lml_grad(kern, theta, 0.0, MU)
    assert info == 0
    a_terms, ik_terms, info = g.loo_terms(kern, theta, 0.0, MU)
    assert info == 0
    a_loo, ik_loo, p, loo_grad, _, info = g.loo_grad(kern, theta, 0.0, MU)
    assert info == 0
    pair(a_grad, a_fit, 1e-12, f"{form} alpha: lml_grad against fit", bits=True)
    pair(a_terms, a_fit, 1e-12, f"{form} alpha: loo_terms against fit", bits=True)
    pair(a_loo, a_fit, 1e-12, f"{form} alpha: loo_grad against fit", bits=True)
    pair(ik_loo, ik_terms, 1e-12, f"{form} diag K^-1: loo_grad against loo_terms", bits=True)
    pair(ik_diag, ik_terms, 1e-12, f"{form} diag K^-1: loo_diag against loo_terms", bits=True)
    pair(lml_g, lml, 1e-12, f"{form} lml: lml_grad against lml", bits=True)
    pair(-0.5 * (g.y - MEAN) @ a_fit - logdet, lml, 1e-10, f"{form} lml: from the fit's alpha and log-determinant")
    pair(a_fit, o.alpha, 1e-10, f"{form} alpha against the oracle")
    pair(lml, o.marginal_likelihood(o.theta), 1e-10, f"{form} lml against the oracle")
    pair(ik_terms, _oracle_ikdiag(o), 1e-10, f"{form} diag K^-1 against the oracle")
    pair(grad, o.marginal_likelihood_gradient(o.theta)[1][1:], 1e-10, f"{form} lml gradient against the oracle")
    pair(loo_grad, o.loo_likelihood_gradient(o.theta)[1][1:], 1e-10, f"{form} loo gradient against the oracle")
    iK = o._factor(o.theta, False)[1]
    pair(p, iK @ (a_fit / np.diag(iK)), 1e-10, f"{form} p = K^-1 c1 against the oracle")


@pytest.mark.parametrize("own_weights", [True, False])
def test_mixture_build_one_theta_through_every_single_entry_point(own_weights):
    """own_weights: the row sums with the sub-kernels' own window weights (hw = NULL); else with the caller's two rows per
    sub-kernel (hw: here what the class passes - row 1 of sub-kernel 0 its weights 1 - f, row 0 of sub-kernel 1 its
    weights f, zeros elsewhere).  Either way 1/2 sum Q o dK / d(location, width) = sum_i df_i (h_1 - h_0)(i)."""
    g = _engine()
    ks, ths, w, extra = _mix_form(g.x)
    o = _oracle(MIX_PARTS, _mix_theta()[1:])
    f = w[1]
    z = (g.x[:, 0] - CP[0]) / CP[1]
    dloc, dwid = -f * (1 - f) / CP[1], -f * (1 - f) * z / CP[1]
    hw = None
    if not own_weights:
        hw = np.zeros((2, 2, N))
        hw[0, 1], hw[1, 0] = 1.0 - f, f
    a_fit, logdet, info = g.fit_mix(ks, ths, w, extra, MU)
    assert info == 0
    ik_diag = g.loo_diag()
    lml, info = g.lml_mix(ks, ths, w, extra, MU)
    assert info == 0
    lml_g, grad, hrows, a_grad, info = g.lml_grad_mix(ks, ths, w, extra, MU, row_weights=hw)
    assert info == 0
    a_terms, ik_terms, info = g.loo_terms_mix(ks, ths, w, extra, MU)
    assert info == 0
    tag = "mixture, own weights" if own_weights else "mixture, caller's weights"
    pair(a_grad, a_fit, 1e-12, f"{tag} alpha: lml_grad_mix against fit_mix", bits=True)
    pair(a_terms, a_fit, 1e-12, f"{tag} alpha: loo_terms_mix against fit_mix", bits=True)
    pair(ik_diag, ik_terms, 1e-12, f"{tag} diag K^-1: loo_diag against loo_terms_mix", bits=True)
    pair(lml_g, lml, 1e-12, f"{tag} lml: lml_grad_mix against lml_mix", bits=True)
    pair(-0.5 * (g.y - MEAN) @ a_fit - logdet, lml, 1e-10, f"{tag} lml: from the fit's alpha and log-determinant")
    pair(a_fit, o.alpha, 1e-10, f"{tag} alpha against the oracle")
    pair(lml, o.marginal_likelihood(o.theta), 1e-10, f"{tag} lml against the oracle")
    pair(ik_terms, _oracle_ikdiag(o), 1e-10, f"{tag} diag K^-1 against the oracle")
    ograd = o.marginal_likelihood_gradient(o.theta)[1][1:]
    pair(grad, ograd[:2 * (D + 1)], 1e-10, f"{tag} sub-kernel gradient against the oracle")
    assert hrows.shape == ((2, N) if own_weights else (2, 2, N))
    dh = hrows[1] - hrows[0] if own_weights else hrows[1, 0] - hrows[0, 1]
    win = [dloc @ dh, dwid @ dh]
    pair(win, ograd[2 * (D + 1):2 * (D + 1) + 2], 1e-10, f"{tag} window gradient against the oracle")


def test_dense_build_one_matrix_through_every_single_entry_point():
    g, kern, theta, parts = _kernel_engine("se")
    o = _oracle(parts, theta)
    K = g.covariance(kern, theta, 0.0, with_noise=True)
    a_fit, logdet, info = g.fit_dense(K, MU)
    assert info == 0
    ik_diag = g.loo_diag()
    lml0, none_a, none_k, info = g.lml_dense(K, MU)
    assert info == 0 and none_a is None and none_k is None
    lml1, a_lml, _, info = g.lml_dense(K, MU, want_alpha=True)
    assert info == 0
    lml2, a_inv, iK, info = g.lml_dense(K, MU, want_alpha=True, want_inverse=True)
    assert info == 0
    a_loo, ik_loo, none_p, none_w, info = g.loo_dense(K, MU)
    assert info == 0 and none_p is None and none_w is None
    a_loo2, ik_loo2, p, W, info = g.loo_dense(K, MU, want_gradient_pieces=True)
    assert info == 0
    for a, what in ((a_lml, "lml_dense"), (a_inv, "lml_dense with K^-1"), (a_loo, "loo_dense"), (a_loo2, "loo_dense with the pieces")):
        pair(a, a_fit, 1e-12, f"dense alpha: {what} against fit_dense", bits=True)
    pair(lml1, lml0, 1e-12, "dense lml: with alpha against without", bits=True)
    pair(lml2, lml0, 1e-12, "dense lml: with K^-1 against without", bits=True)
    pair(-0.5 * (g.y - MEAN) @ a_fit - logdet, lml0, 1e-10, "dense lml: from the fit's alpha and log-determinant")
    pair(ik_loo2, ik_loo, 1e-12, "dense diag K^-1: loo_dense with the pieces against without", bits=True)
    pair(ik_diag, ik_loo, 1e-12, "dense diag K^-1: loo_diag against loo_dense", bits=True)
    pair(np.diag(iK), ik_loo, 1e-12, "dense diag K^-1: the diagonal of lml_dense's inverse against loo_dense")
    pair(iK, iK.T, 1e-12, "dense K^-1 against its transpose", bits=True)
    pair(W, W.T, 1e-12, "dense W against its transpose", bits=True)
    oK = o._factor(o.theta, False)[1]
    pair(iK, oK, 1e-10, "dense K^-1 against the oracle")
    var = 1.0 / np.diag(oK)
    pair(p, oK @ (o.alpha * var), 1e-10, "dense p against the oracle")
    pair(W, oK @ np.diag(0.5 * var * (1.0 + var * o.alpha**2)) @ oK, 1e-10, "dense W against the oracle")


def test_the_three_builds_against_each_other():
    """The same matrix built by the kernels, as a mixture of one sub-kernel with unit weights, and handed over dense
    (gpmi_covariance with the noise): alpha, LML, diag K^-1 of the three.  Then ChangePoint[SE, SE] + WhiteNoise against
    its matrix assembled on the host from gpmi_covariance's sub-kernel matrices."""
    for form in ("se", "se+rq"):
        g, kern, theta, _ = _kernel_engine(form)
        K = g.covariance(kern, theta, 0.0, with_noise=True)
        a_k, ld_k, _ = g.fit(kern, theta, 0.0, MU)
        a_t, ik_k, _ = g.loo_terms(kern, theta, 0.0, MU)
        l_k, _ = g.lml(kern, theta, 0.0, MU)
        a_d, ld_d, info = g.fit_dense(K, MU)
        assert info == 0
        l_d, _, _, _ = g.lml_dense(K, MU)
        _, ik_d, _, _, _ = g.loo_dense(K, MU)
        pair(a_d, a_k, 1e-12, f"{form} alpha: dense against kernel build", bits=True)
        pair(ld_d, ld_k, 1e-12, f"{form} log-determinant: dense against kernel build", bits=True)
        pair(l_d, l_k, 1e-12, f"{form} lml: dense against kernel build", bits=True)
        pair(ik_d, ik_k, 1e-12, f"{form} diag K^-1: dense against kernel build", bits=True)
        if form == "se":
            one = np.ones((1, N))
            a_m, ld_m, info = g.fit_mix([kern], [theta], one, 0.0, MU)
            assert info == 0
            l_m, _ = g.lml_mix([kern], [theta], one, 0.0, MU)
            _, ik_m, _ = g.loo_terms_mix([kern], [theta], one, 0.0, MU)
            pair(a_m, a_k, 1e-12, "se alpha: mixture of one against kernel build", bits=True)
            pair(ld_m, ld_k, 1e-12, "se log-determinant: mixture of one against kernel build", bits=True)
            pair(l_m, l_k, 1e-12, "se lml: mixture of one against kernel build", bits=True)
            pair(ik_m, ik_k, 1e-12, "se diag K^-1: mixture of one against kernel build", bits=True)
    g = _engine()
    ks, ths, w, extra = _mix_form(g.x)
    K = sum(np.outer(w[m], w[m]) * g.covariance(ks[m], ths[m], 0.0, with_noise=False) for m in range(2))
    K = K + np.diag(np.full(N, 0.1**2 + extra))
    a_m, ld_m, info = g.fit_mix(ks, ths, w, extra, MU)
    assert info == 0
    l_m, _ = g.lml_mix(ks, ths, w, extra, MU)
    _, ik_m, _ = g.loo_terms_mix(ks, ths, w, extra, MU)
    a_d, ld_d, info = g.fit_dense(K, MU)
    assert info == 0
    l_d, _, _, _ = g.lml_dense(K, MU)
    _, ik_d, _, _, _ = g.loo_dense(K, MU)
    pair(a_d, a_m, 1e-12, "ChangePoint alpha: dense against mixture build", bits=True)
    pair(ld_d, ld_m, 1e-12, "ChangePoint log-determinant: dense against mixture build", bits=True)
    pair(l_d, l_m, 1e-12, "ChangePoint lml: dense against mixture build", bits=True)
    pair(ik_d, ik_m, 1e-12, "ChangePoint diag K^-1: dense against mixture build", bits=True)


# --------------------------------------------------------------------------------------------------- query chunk seams
def _points(m, seed):
    x = mh.dataset(N, D)[0]
    pts = np.random.default_rng(seed).uniform(0.0, 4.0, size=(m, D))
    pts[0] = x[2]  # a query point on a training point
    return pts


@pytest.mark.parametrize("form", ["kernel", "mixture", "dense"])
def test_predict_of_2049_rows_at_the_chunk_seam(form):
    """m = 2049: a chunk of 2048 rows and a chunk of one.  Rows 0, 2047, 2048 against the same points in calls of their
    own, mean and variance term; row 0 and 2048 against the oracle."""
    pts = _points(2049, 2049)
    g, kern, theta, parts = _kernel_engine("se")
    if form == "kernel":
        assert g.fit(kern, theta, 0.0, MU)[2] == 0
        call = lambda rows: g.predict(pts[rows])
        o = _oracle(parts, theta)
        variance = lambda v: v
    elif form == "dense":
        assert g.fit_dense(g.covariance(kern, theta, 0.0, with_noise=True), MU)[2] == 0
        Kq = g.cross_covariance(kern, theta, pts)
        call = lambda rows: g.predict_dense(Kq[rows])
        o = _oracle(parts, theta)
        variance = lambda ss: np.exp(2 * theta[0]) - ss
    else:
        ks, ths, w, extra = _mix_form(g.x)
        assert g.fit_mix(ks, ths, w, extra, MU)[2] == 0
        f = _window(pts[:, 0])
        gq = np.array([1.0 - f, f])
        call = lambda rows: g.predict_mix(pts[rows], gq[:, rows])
        o = _oracle(MIX_PARTS, _mix_theta()[1:])
        variance = lambda nss: gq[0] ** 2 * np.exp(2 * ths[0][0]) + gq[1] ** 2 * np.exp(2 * ths[1][0]) + nss
    whole = call(slice(0, 2049))
    assert whole[0].shape == whole[1].shape == (2049,)
    for r in (0, 2047, 2048):
        one = call(slice(r, r + 1))
        pair(whole[0][r:r + 1], one[0], 1e-12, f"{form} predict of 2049 [{r}] mean against a call of its own", bits=True)
        pair(whole[1][r:r + 1], one[1], 1e-12, f"{form} predict of 2049 [{r}] variance term against a call of its own", bits=True)
    rows = [0, 2047, 2048]
    mu, sd = o(pts[rows])
    pair(whole[0][rows], mu - MEAN, 1e-10, f"{form} predict of 2049 means against the oracle")
    pair(np.abs(variance(whole[1])[rows]), sd**2, 1e-10, f"{form} predict of 2049 variances against the oracle")


@pytest.mark.parametrize("form", ["kernel", "mixture"])
@pytest.mark.parametrize("m", [129, 1])
def test_posterior_against_predict(form, m):
    """m = 129: two tiles, the second ragged; m = 1."""
    pts = _points(m, 129)
    g, kern, theta, parts = _kernel_engine("se")
    if form == "kernel":
        assert g.fit(kern, theta, 0.0, MU)[2] == 0
        mean, var = g.predict(pts)
        mu, cov = g.posterior(pts)
        mu_only, none = g.posterior(pts, mean_only=True)
        draws, mu_d, _, info = g.posterior_draws(pts, n_draws=2, seed=7)
        assert info == 0 and draws.shape == (2, m)
        pair(mu_d, mu, 1e-12, f"kernel posterior_draws of {m}: mean against posterior", bits=True)
        o = _oracle(parts, theta)
    else:
        ks, ths, w, extra = _mix_form(g.x)
        assert g.fit_mix(ks, ths, w, extra, MU)[2] == 0
        f = _window(pts[:, 0])
        gq = np.array([1.0 - f, f])
        mean, nss = g.predict_mix(pts, gq)
        var = gq[0] ** 2 * np.exp(2 * ths[0][0]) + gq[1] ** 2 * np.exp(2 * ths[1][0]) + nss
        mu, cov = g.posterior_mix(pts, gq)
        mu_only, none = g.posterior_mix(pts, gq, mean_only=True)
        o = _oracle(MIX_PARTS, _mix_theta()[1:])
    assert none is None and cov.shape == (m, m)
    pair(mu, mean, 1e-12, f"{form} posterior of {m}: mean against predict", bits=True)
    pair(mu_only, mu, 1e-12, f"{form} posterior of {m}: mean alone against mean with covariance", bits=True)
    pair(np.diag(cov), var, 1e-12, f"{form} posterior of {m}: diagonal against predict's variance")
    pair(cov, cov.T, 1e-12, f"{form} posterior of {m}: covariance against its transpose", bits=True)
    omu, ocov = o.build_posterior(pts)
    pair(mu, omu - MEAN, 1e-10, f"{form} posterior of {m}: mean against the oracle")
    pair(cov, ocov, 1e-10, f"{form} posterior of {m}: covariance against the oracle")


def test_solve_rows_of_129():
    pts = _points(129, 130)
    g, kern, theta, _ = _kernel_engine("se")
    assert g.fit(kern, theta, 0.0, MU)[2] == 0
    Q = g.cross_covariance(kern, theta, pts)
    X, G = g.solve_rows(Q, want_rows=True, want_gram=True)
    G_only = g.solve_rows(Q, want_rows=False, want_gram=True)[1]
    _, ss = g.predict_dense(Q)
    pair((X**2).sum(axis=1), ss, 1e-10, "solve_rows of 129: squared row norms of X against predict_dense")
    pair(G, X @ X.T, 1e-10, "solve_rows of 129: gram against X X^T")
    pair(G_only, G, 1e-12, "solve_rows of 129: gram alone against gram with the rows", bits=True)
    L = g.get_L()
    pair(X @ L.T, Q, 1e-10, "solve_rows of 129: X L^T against Q")


# ---------------------------------------------------------------------------------------------------------- state flags
def test_state_flags_the_entry_points_leave_behind():
    from inference_amd._lib import GpmiError

    g, kern, theta, _ = _kernel_engine("se")
    pts = _points(3, 3)
    ks, ths, w, extra = _mix_form(g.x)
    gq = np.array([1.0 - _window(pts[:, 0]), _window(pts[:, 0])])
    assert g.fit_mix(ks, ths, w, extra, MU)[2] == 0
    g.predict_mix(pts, gq)
    # (gpmi_fit_mix leaves sub-kernel 0 in fit_params: gpmi_get_K answers with that kernel's matrix)
    pair(g.get_K(), g.covariance(ks[0], ths[0], 0.0, with_noise=True), 1e-12, "get_K after fit_mix against sub-kernel 0", bits=True)
    assert g.lml_mix(ks, ths, w, extra, MU)[1] == 0
    with pytest.raises(GpmiError, match="gpmi_predict_mix needs a successful gpmi_fit_mix"):
        g.predict_mix(pts, gq)
    assert g.fit_mix(ks, ths, w, extra, MU)[2] == 0
    assert g.loo_terms_mix(ks, ths, w, extra, MU)[2] == 0
    with pytest.raises(GpmiError, match="gpmi_predict_mix needs a successful gpmi_fit_mix"):
        g.predict_mix(pts, gq)
    assert g.fit_dense(g.covariance(kern, theta, 0.0, with_noise=True), MU)[2] == 0
    with pytest.raises(GpmiError, match="gpmi_predict: the model was fitted with a caller-built covariance"):
        g.predict(pts)
    with pytest.raises(GpmiError, match="gpmi_get_K: the covariance of this fit was built by the caller"):
        g.get_K()
    with pytest.raises(GpmiError, match="gpmi_predict_mix needs a successful gpmi_fit_mix"):
        g.predict_mix(pts, gq)
    g.predict_dense(g.cross_covariance(kern, theta, pts))
    assert g.fit(kern, theta, 0.0, MU)[2] == 0
    g.predict(pts)
    g.get_K()
