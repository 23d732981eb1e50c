"""
GPU tests of the seams of the lockstep batches (np <= 4096, the batch in blockIdx.z): the chunk loops, the offsets of the
second half-batch and of the asynchronous slots, and the per-sub-kernel strides of the mixture batches - the places a
chunk's rows can be filed under the wrong index.

The shape is the smallest that has two of everything: n = 130, d = 2, hence np = 256 - two diagonal blocks (one batched
panel step and update, two steps per sweep) and a ragged last tile.  y_err = 0.1; all theta distinct, a base vector plus
0.1 x normal: a row filed under another row's index is off by far more than any tolerance here.  Every case works on
fresh handles with `batch_independent_values(True)`.

Bit-for-bit comparisons (np.array_equal) are between calls that run the same chunks and launches (65 = 64 + 1), or rest
on the batch-independence of DESIGN.md section 4.4 (a value does not depend on the batch it is evaluated in).  The others
carry the tolerances tests/test_gpu_parity.py uses for the same comparison: batch member against single evaluation 1e-12
(LML) / 1e-11 (its gradient, element-wise too), 1e-11 / 1e-10 with etol 1e-6 (leave-one-out); 1e-10 against the NumPy
oracle of tests/matern_host.py.  Every comparison prints its achieved error.
"""
import numpy as np
import pytest

import matern_host as mh

pytestmark = pytest.mark.gpu

N, D = 130, 2
MODELS = {
    "se": [("se",)],
    "se+rq": [("se",), ("rq",)],
    "se+het": [("se",), ("het",)],
    "cp+wn": [("cp", ("se", "se"), 0), ("wn",)],
}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not np.isnan(a).any()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(a, b, tol, what):
    r = rel(a, b)
    print(f"{what}: {r:.2e} (tol {tol:.0e})")
    assert r <= tol, f"{what}: relative error {r:.3e} > {tol:.1e}"


def check_each(a, b, tol, what, floor=1e-6, etol=1e-7):
    """`check` plus the element-wise half of tests/test_gpu_parity.py's check_each."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    check(a, b, tol, what)
    big = np.abs(b) > floor * np.abs(b).max()
    r = float((np.abs(a - b)[big] / np.abs(b)[big]).max()) if big.any() else 0.0
    print(f"{what} (element-wise, {int(big.sum())} of {big.size}): {r:.2e} (tol {etol:.0e})")
    assert r <= etol, f"{what}: element-wise relative error {r:.3e} > {etol:.1e}"


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), f"{what}: not bit-identical (max difference {np.abs(a - b).max():.2e}, " \
                                 f"{int((a != b).sum())} of {a.size} elements)"
    print(f"{what}: bit-identical ({a.size} values)")


def _base_theta(parts):
    """[mean, the parts' parameters back to back] (the layout of tests/matern_host.py's HostModel)"""
    out = [0.1]
    for i, p in enumerate(parts):
        if p[0] == "wn":
            out.append(np.log(0.15))
        elif p[0] == "het":
            out.extend(np.log(np.linspace(0.05, 0.2, N)))
        elif p[0] == "cp":
            for j, k in enumerate(p[1]):
                out.extend(mh.theta_for(k, D, 10 * j))
            out.extend([2.0, 0.5])
        else:
            th = mh.theta_for(p[0], D, i)
            th[0] -= 0.3 * i
            out.extend(th)
    return np.array(out, dtype=float)


def _thetas(parts, T, seed):
    base = _base_theta(parts)
    th = base[None, :] + 0.1 * np.random.default_rng(seed).standard_normal((T, base.size))
    assert len({tuple(r) for r in th}) == T
    return th


def _fresh(parts, theta):
    """A regressor on a handle of its own, every batch on the lockstep path."""
    import inference_amd.gp as gp

    cls = {"se": gp.SquaredExponential, "rq": gp.RationalQuadratic, "wn": gp.WhiteNoise, "het": gp.HeteroscedasticNoise}
    objs = [gp.ChangePoint([cls[k]() for k in p[1]], axis=p[2]) if p[0] == "cp" else cls[p[0]]() for p in parts]
    cov = objs[0]
    for o in objs[1:]:
        cov = cov + o
    x, y, e = mh.dataset(N, D)
    g = gp.GpRegressor(x, y, y_err=e, kernel=cov, hyperpars=theta)
    g.batch_independent_values(True)
    assert g._generic is False and g.engine.capacity() == 256
    return g


def _batch_calls(g):
    """Log of the batch entry points the handle is called with from here on."""
    log, call = [], g.engine.h.call

    def spy(name, *args):
        if "_batch" in name:
            log.append(name)
        return call(name, *args)

    g.engine.h.call = spy
    return log


# ------------------------------------------------------------------------------- chunk boundary of the gradient batches
def _both_gradients(g, thetas):
    return (*g.marginal_likelihood_gradient_batch(thetas), *g.loo_likelihood_gradient_batch(thetas))


@pytest.mark.parametrize("model,entry", [("se", ("gpmi_lml_grad_batch", "gpmi_loo_grad_batch")),
                                         ("se+rq", ("gpmi_lml_grad_batch", "gpmi_loo_grad_batch")),
                                         ("se+het", ("gpmi_lml_grad_batch_noise", "gpmi_loo_grad_batch_noise")),
                                         ("cp+wn", ("gpmi_lml_grad_batch_mix", "gpmi_loo_grad_batch_mix"))])
def test_gradient_batch_of_65_is_a_chunk_of_64_and_a_chunk_of_one(model, entry):
    """T = 65 on a fresh handle: the workspace holds 64, so one C call runs a chunk of 64 and a chunk of one.  It must
    equal, bit for bit, a call with rows 0 .. 63 followed by a call with row 64 on another fresh handle (the same chunks,
    the same launches), and rows 0, 63, 64 must agree with one-at-a-time evaluations.  SE: the plain path; SE + RQ: a
    sum (bSum); SE + HeteroscedasticNoise: *_batch_noise with qdiag / mdiag; ChangePoint[SE, SE] + WhiteNoise: *_batch_mix
    with qdiag and the caller's row weights hw (what the class passes)."""
    parts = MODELS[model]
    thetas = _thetas(parts, 65, 65)
    g = _fresh(parts, thetas[0])
    log = _batch_calls(g)
    whole = _both_gradients(g, thetas)
    assert log == list(entry), log  # one C call each carries all 65
    assert whole[1].shape == whole[3].shape == thetas.shape
    h = _fresh(parts, thetas[0])
    head, tail = _both_gradients(h, thetas[:64]), _both_gradients(h, thetas[64:])
    for w, a, b, what in zip(whole, head, tail, ("lml", "lml gradient", "loo", "loo gradient")):
        same(w, np.concatenate([a, b]), f"{model} {what}: 65 against 64 + 1")
    s = _fresh(parts, thetas[0])
    for t in (0, 63, 64):
        v, gr = s.marginal_likelihood_gradient(thetas[t])
        check(whole[0][t], v, 1e-12, f"{model} [{t}] lml: batch against single")
        check_each(whole[1][t], gr, 1e-11, f"{model} [{t}] lml gradient: batch against single")
        v, gr = s.loo_likelihood_gradient(thetas[t])
        check(whole[2][t], v, 1e-11, f"{model} [{t}] loo: batch against single")
        check_each(whole[3][t], gr, 1e-10, f"{model} [{t}] loo gradient: batch against single", etol=1e-6)


def _mix_engine_batches(g, thetas):
    """Both mixture batches through the engine with the sub-kernels' OWN window weights (hw = NULL: the class always
    passes hw): every array the two calls return."""
    stat = [np.ascontiguousarray(t[g.cov_slice][g._stat_slice]) for t in thetas]
    ex = np.array([float(np.exp(2 * t[g.cov_slice][g._wn_index])) for t in thetas])
    args = [g._mix_args(s) for s in stat]
    sub, wts = [a[1] for a in args], np.array([a[2] for a in args])
    a = g.engine.lml_grad_batch_mix(args[0][0], sub, wts, ex, mu_const=thetas[:, 0], want_qdiag=True)
    b = g.engine.loo_grad_batch_mix(args[0][0], sub, wts, ex, mu_const=thetas[:, 0])
    names = ("lml", "gradient", "hrows", "alpha", "qdiag", "info", "loo alpha", "ikdiag", "p", "mdiag", "loo gradient",
             "loo hrows", "loo info")
    return dict(zip(names, (*a, *b))), (args, ex)


def _loo_value(alpha, ikdiag):
    """The leave-one-out log-likelihood as the class forms it (regression.py:468-487)."""
    var = 1.0 / np.asarray(ikdiag)
    return float(-0.5 * (var * np.asarray(alpha) ** 2 + np.log(var)).sum())


def test_mixture_batch_of_65_with_the_sub_kernels_own_window_weights():
    """The same 64 + 1 split for gpmi_lml_grad_batch_mix / gpmi_loo_grad_batch_mix with hw = NULL (one row sum per
    sub-kernel, the weights' stride instead of the row-sum weights'), every returned array.  The first 64 rows are the
    same launch on both sides of that comparison, so rows 0, 63, 64 are also held against evaluations of one theta each:
    the likelihood half (value, gradient, row sums) against gpmi_lml_grad_mix on the single-evaluation path; the
    leave-one-out value, formed from alpha and diag K^-1 as the class does, against gpmi_loo_terms_mix on that path; and
    every leave-one-out array against gpmi_loo_grad_batch_mix with that theta alone (a chunk of one has z = 0 only: no
    stride between problems enters).  Tolerances: those of the value for alpha and diag K^-1, which the value is formed
    from (1e-11); those of the gradient for p, diag M and the row sums, which the gradient is contracted from (1e-11
    likelihood, 1e-10 with etol 1e-6 leave-one-out)."""
    parts = MODELS["cp+wn"]
    thetas = _thetas(parts, 65, 66)
    g = _fresh(parts, thetas[0])
    log = _batch_calls(g)
    whole, (args, ex) = _mix_engine_batches(g, thetas)
    assert log == ["gpmi_lml_grad_batch_mix", "gpmi_loo_grad_batch_mix"], log
    assert whole["hrows"].shape == whole["loo hrows"].shape == (65, 2, N)
    assert not whole["info"].any() and not whole["loo info"].any()
    h = _fresh(parts, thetas[0])
    head, tail = _mix_engine_batches(h, thetas[:64])[0], _mix_engine_batches(h, thetas[64:])[0]
    for k in whole:
        same(whole[k], np.concatenate([head[k], tail[k]]), f"mixture, own weights, {k}: 65 against 64 + 1")
    s = _fresh(parts, thetas[0])
    for t in (0, 63, 64):
        lml, grad, hrows, alpha, info = s.engine.lml_grad_mix(*args[t], ex[t], np.full(N, thetas[t, 0]))
        assert info == 0
        check(whole["lml"][t], lml, 1e-12, f"mixture, own weights [{t}] lml: batch against single")
        check_each(whole["gradient"][t], grad, 1e-11, f"mixture, own weights [{t}] gradient: batch against single")
        check_each(whole["hrows"][t], hrows, 1e-11, f"mixture, own weights [{t}] row sums: batch against single")
        what = f"mixture, own weights [{t}] loo"
        alpha, ikdiag, info = s.engine.loo_terms_mix(*args[t], ex[t], np.full(N, thetas[t, 0]))
        assert info == 0
        check(_loo_value(whole["loo alpha"][t], whole["ikdiag"][t]), _loo_value(alpha, ikdiag), 1e-11,
              f"{what} value: batch against single")
        one = _mix_engine_batches(_fresh(parts, thetas[0]), thetas[t:t + 1])[0]
        assert not one["loo info"].any()
        check(_loo_value(whole["loo alpha"][t], whole["ikdiag"][t]), _loo_value(one["loo alpha"][0], one["ikdiag"][0]), 1e-11,
              f"{what} value: batch against batch of one")
        for k in ("loo alpha", "ikdiag"):
            check(whole[k][t], one[k][0], 1e-11, f"{what} {k}: batch against batch of one")
        for k in ("p", "mdiag", "loo gradient", "loo hrows"):
            check_each(whole[k][t], one[k][0], 1e-10, f"{what} {k}: batch against batch of one", etol=1e-6)


# ---------------------------------------------------------------------- split and chunk boundary of the likelihood batch
@pytest.fixture(scope="module")
def lml_case():
    """513 hyper-parameter vectors and their values in calls of four on one handle (computed once, not modified)."""
    parts = MODELS["se"]
    thetas = _thetas(parts, 513, 513)
    g = _fresh(parts, thetas[0])
    fours = np.concatenate([g.marginal_likelihood_batch(thetas[t:t + 4]) for t in range(0, 513, 4)])
    fours.setflags(write=False)
    x, y, e = mh.dataset(N, D)
    orc = mh.OracleGp(x, y, e, mh.HostModel(parts, x), thetas[0])
    oracle = {t: orc.marginal_likelihood(thetas[t]) for t in (0, 7, 8, 16, 512)}
    return parts, thetas, fours, oracle


@pytest.mark.parametrize("T", [15, 16, 17, 513])
def test_likelihood_batch_at_the_split_and_past_the_workspace(lml_case, T):
    """gpmi_lml_batch with T = 15 (one stream), 16 (two halves of 8), 17 (8 and 9) and 513 (the default 512-matrix
    workspace - two halves of 256 - and a chunk of one; about 300 MB at this size): bit for bit the values of the same
    theta in calls of four, and rows 0, 7, 8, 16, 512 against the oracle."""
    parts, thetas, fours, oracle = lml_case
    g = _fresh(parts, thetas[0])
    log = _batch_calls(g)
    vals = g.marginal_likelihood_batch(thetas[:T])
    assert log == ["gpmi_lml_batch"], log
    same(vals, fours[:T], f"lml batch of {T} against calls of four")
    for t, v in oracle.items():
        if t < T:
            check(vals[t], v, 1e-10, f"lml batch of {T} [{t}] against the oracle")


def test_asynchronous_slot_one_alone(lml_case):
    """submit(th[:3], 1) / wait(1) on a fresh handle - the offset bcap / 2 with nothing in slot 0 - equals the
    synchronous call bit for bit."""
    parts, thetas, fours, _ = lml_case
    g = _fresh(parts, thetas[0])
    assert g.async_batches()
    g.marginal_likelihood_batch_submit(thetas[:3], 1)
    same(g.marginal_likelihood_batch_wait(1), _fresh(parts, thetas[0]).marginal_likelihood_batch(thetas[:3]),
         "slot 1 alone against the synchronous call")
    same(g.marginal_likelihood_batch(thetas[:3]), fours[:3], "the synchronous call after the wait")


# ----------------------------------------------------------------------------------------------------- predict batch
def test_predict_batch_at_the_split_and_a_panel_boundary():
    """gpmi_predict_batch with T = 17 (halves of 8 and 9 on two streams) and m = 257 (one panel of 256 points and one
    point), mean and variance: every row bit-identical to the T = 1 call for that theta, and the mixture with all the
    weight on one theta returns that row."""
    parts = MODELS["se"]
    thetas = _thetas(parts, 17, 17)
    x, y, e = mh.dataset(N, D)
    pts = np.random.default_rng(257).uniform(0.0, 4.0, size=(257, D))
    pts[0] = x[2]  # a query point on a training point
    g = _fresh(parts, thetas[0])
    log = _batch_calls(g)
    means, sds = g.predict_samples(pts, thetas)
    assert log == ["gpmi_predict_batch"], log
    assert means.shape == sds.shape == (17, 257)
    one = _fresh(parts, thetas[0])
    for t in range(17):
        m1, s1 = one.predict_samples(pts, thetas[t:t + 1])
        same(means[t], m1[0], f"predict batch of 17 [{t}] mean against the batch of one")
        same(sds[t], s1[0], f"predict batch of 17 [{t}] standard deviation against the batch of one")
    for t in (0, 8, 16):
        w = np.zeros(17)
        w[t] = 1.0
        mean, sd = g.predict_marginalised(pts, thetas, weights=w)
        same(mean, means[t], f"mixture with all the weight on [{t}]: mean")
        same(sd, sds[t], f"mixture with all the weight on [{t}]: standard deviation")
    mu, _ = mh.OracleGp(x, y, e, mh.HostModel(parts, x), thetas[8])(pts)
    check(means[8], mu, 1e-10, "predict batch of 17 [8] mean against the oracle")
