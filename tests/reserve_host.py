"""
Cases and builders for the tests of regressors with reserved device capacity and of handles that `add_point` has grown
(tests/test_reserve_cpu.py, tests/test_reserve_gpu.py).  Host only: nothing here touches a device until a builder is
called.

A `GpRegressor(reserve=R)` pads its device matrices to np = round_up(n + R, 128) with identity; `add_point` then raises n
under the live handle (gpmi_append_point).  Per case three regressors on one data set at one theta:

    grown   built on the first n0 points with `reserve`, the other `appends` points added one by one;
    twin    built on all n0 + appends points with the reserve that gives the same capacity: same n, same np, never
            appended to;
    tight   the same data with reserve = 0.

The yardstick is tests/matern_host.py (`HostModel`, `OracleGp`), `parts` in its notation.  Every case's K + sig at the
final n has cond <= 2e4 (tests/test_reserve_cpu.py asserts it): the bound under which the comparisons behind a
factorisation meet the project's 1e-10.  Where `matern_host.dataset` / `theta_for` as generated exceed it, the error bars
or the length scales are changed (`inputs`), never a tolerance.
"""
from collections import namedtuple

import numpy as np

import matern_host as mh
import ycov_builders as yb

Case = namedtuple("Case", "parts d n0 appends reserve mean")

# name -> (parts, d, n0, appends, reserve, mean); np = round_up(n0 + reserve, 128)
CASES = {
    # crosses a 64 covariance tile; np = 384: two whole 128-tiles of padding; GpOptimiser's own reserve
    "se_62": Case([("se",)], 2, 62, 4, 256, "const"),
    # crosses a 128 tile (np = 256); Matern append; extra_diag; LinearMean: every prior mean moves with each point
    "m52wn_126": Case([("m52",), ("wn",)], 3, 126, 4, 8, "linear"),
    # GPMI_KERNEL_SUM; starts with exactly one whole padding tile and no ragged one (np = 256)
    "sum_128": Case([("se",), ("rq",), ("wn",)], 2, 128, 2, 128, "const"),
    # crosses a 512 outer block (np = 640): a new invD block and a new inv2 block
    "rq_510": Case([("rq",)], 1, 510, 5, 8, "const"),
    # np = 2048 = 4 outer blocks: the size from which a fit prebuilds the inverse blocks beside its sweeps where the lane has
    # its look-ahead streams (they come with N of ~7000, beyond this suite: here the blocks are cached by the predictions
    # between the appends, see `append`); four 512-blocks, the appended rows in the last one
    "m32_2040": Case([("m32",)], 2, 2040, 5, 8, "const"),
    # mixture builders over whole padding tiles (np = 512); add_point rebuilds and keeps reserve >= 128
    "cp_130": Case([("cp", ("se", "se"), 1), ("wn",)], 2, 130, 1, 256, "const"),
    # per-point-noise lockstep forms on padding (np = 384); add_point is refused
    "het_96": Case([("se",), ("het",)], 1, 96, 0, 200, "const"),
    # dense y_cov: the full-matrix add over n inside a larger np (384); add_point is refused
    "ycov_100": Case([("se",)], 2, 100, 0, 256, "const"),
}
GROWN = [name for name, c in CASES.items() if c.appends and c.parts[0][0] != "cp"]  # the O(N^2) appends
COND_MAX = 2e4
SIGMA_WN = 0.2


def round_up(n, m=128):
    return (n + m - 1) // m * m


def capacity(name):
    c = CASES[name]
    return round_up(c.n0 + c.reserve)


def theta_of(name):
    """[the mean's parameters | the parts' parameters back to back]: `matern_host.theta_for` per stationary kernel (the
    components of a sum and the regions of a ChangePoint get different seeds and amplitudes), sigma = 0.2 for WhiteNoise,
    per-point sigmas 0.15 .. 0.3 for HeteroscedasticNoise, the ChangePoint at 2.0 on its axis with width 0.5."""
    c = CASES[name]
    out = [0.1] + ([0.1, -0.2, 0.05][:c.d] if c.mean == "linear" else [])
    n = c.n0 + c.appends
    for i, p in enumerate(c.parts):
        if p[0] == "wn":
            out.append(np.log(SIGMA_WN))
        elif p[0] == "het":
            out.extend(np.log(np.linspace(0.15, 0.3, n)[np.random.default_rng(n).permutation(n)]))
        elif p[0] == "cp":
            for j, k in enumerate(p[1]):
                th = mh.theta_for(k, c.d, 10 * j)
                th[0] -= 0.3 * j
                out.extend(th)
            out.extend([2.0, 0.5])
        else:
            th = mh.theta_for(p[0], c.d, i)
            th[0] -= 0.3 * i
            out.extend(th)
    theta = np.array(out, dtype=float)
    if name == "m32_2040":  # as generated cond(K + sig) = 8.9e4: shorter length scales (and larger error bars, `inputs`)
        theta[-c.d:] += np.log(0.2)
    return theta


def inputs(name):
    """(x, y, data errors, theta) at the final n: `matern_host.dataset(n, d, far=False)`; the data errors are standard
    deviations (n,), or the dense covariance (n, n) of `ycov_100`."""
    c = CASES[name]
    n = c.n0 + c.appends
    x, y, e = mh.dataset(n, c.d, far=False)
    if name == "rq_510":  # as generated cond = 5.0e4
        e = np.full(n, 0.3)
    elif name == "m32_2040":
        e = np.full(n, 0.2)
    elif name == "ycov_100":
        rng = np.random.default_rng(100)
        t, s = yb.correlated_cov_inputs(rng, n)
        e = yb.correlated_cov(t, 4.0 * s)  # scales ~0.2: exponential correlation over random times plus a diagonal share
    return x, y, e, theta_of(name)


def thetas_around(name, count=3, seed=0):
    """`count` parameter vectors around the case's theta (normal steps of 0.05)."""
    theta = theta_of(name)
    rng = np.random.default_rng(1000 + seed + theta.size)
    return theta[None, :] + 0.05 * rng.standard_normal((count, theta.size))


def oracle(name, n=None):
    """The host oracle of a case on its first n points (default: all)."""
    c = CASES[name]
    x, y, e, theta = inputs(name)
    assert n is None or not any(p[0] == "het" for p in c.parts)
    n = len(y) if n is None else n
    e = e[:n, :n] if e.ndim == 2 else e[:n]
    mean = mh.LinearMeanHost(x[:n]) if c.mean == "linear" else None
    return mh.OracleGp(x[:n], y[:n], e, mh.HostModel(c.parts, x[:n]), theta, mean=mean)


def n_mean(name):
    c = CASES[name]
    return 1 + (c.d if c.mean == "linear" else 0)


def gradient_kind(name):
    """The kernel whose predictive-gradient kernels the device has for this case, or None (the documented refusal)."""
    stat = [p for p in CASES[name].parts if p[0] not in ("wn", "het")]
    return stat[0][0] if len(stat) == 1 and stat[0][0] in ("se", "m32", "m52") else None


def hessian_kind(name):
    """The kernel of a case that has the exact Hessian (one stationary kernel, + WhiteNoise, diagonal errors), or None."""
    c = CASES[name]
    stat = [p for p in c.parts if p[0] != "wn"]
    ok = len(stat) == 1 and stat[0][0] in ("se", "rq", "m32", "m52") and name != "ycov_100"
    return stat[0][0] if ok else None


# ---------------------------------------------------------------------------------------------------- the regressors
def device_cov(parts):
    import inference_amd.gp as gp

    cls = {"m32": gp.Matern32, "m52": gp.Matern52, "se": gp.SquaredExponential, "rq": gp.RationalQuadratic,
           "wn": gp.WhiteNoise, "het": gp.HeteroscedasticNoise}
    objs = [gp.ChangePoint([cls[k]() for k in p[1]], axis=p[2]) if p[0] == "cp" else cls[p[0]]() for p in parts]
    cov = objs[0]
    for o in objs[1:]:
        cov = cov + o
    return cov


def regressor(name, n, reserve):
    """The case's model on its first n points at the case's theta with `reserve`."""
    import inference_amd.gp as gp

    c = CASES[name]
    x, y, e, theta = inputs(name)
    err = dict(y_cov=e[:n, :n]) if e.ndim == 2 else dict(y_err=e[:n])
    return gp.GpRegressor(x[:n], y[:n], hyperpars=theta, kernel=device_cov(c.parts),
                          mean=gp.LinearMean if c.mean == "linear" else gp.ConstantMean, reserve=reserve, **err)


def append(gp, name, count=None):
    """`add_point` for the case's next `count` points (default: all that are left), with a prediction in front of every
    append, as GpOptimiser makes them (the acquisition is evaluated on the model before each evaluation is added): the
    prediction leaves the 512-wide inverse blocks of the factor cached at the old n, and the append has to drop them."""
    c = CASES[name]
    x, y, e, _ = inputs(name)
    stop = c.n0 + c.appends if count is None else gp.n_points + count
    for i in range(gp.n_points, stop):
        gp(x[i:i + 1] + 0.25)
        gp.add_point(x[i], y[i], e[i])
    return gp


def grown(name):
    c = CASES[name]
    gp = append(regressor(name, c.n0, c.reserve), name)
    assert gp.n_points == c.n0 + c.appends
    return gp


def twin(name, cap):
    """All points at once, with the reserve that pads to `cap`, the capacity of the grown handle."""
    c = CASES[name]
    n = c.n0 + c.appends
    gp = regressor(name, n, cap - n)
    assert gp.engine.capacity() == cap, (gp.engine.capacity(), cap)
    return gp


def tight(name):
    c = CASES[name]
    return regressor(name, c.n0 + c.appends, 0)
