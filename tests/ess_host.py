"""Shared pieces of the effective-sample-size tests (test infrastructure only: the product has no CPU path).

`case(name)` rebuilds the seeded inputs of golden/ess.npz (golden/make_golden_ess.py draws them from here too, and stores
the first and last 8 values of every drawn array, which `checked_case` compares); `mirror` is the device's definition in
NumPy: direct fp64 lag sums of the length-n circular autocorrelation up to the first negative lag."""
import numpy as np

SEED = 20261018
AR = {4096: 256, 20000: 8, 4097: 8, 65: 8}  # rows -> columns of the ar_<n> recipes
AR_EVEN = [4096, 20000]
RAMP_EVEN = [4096, 8190, 20000]
COS = [3, 255, 256, 257, 1023, 1024, 1025, 4096]
ODD = ["ar_4097", "ar_65", "ramp_8191"]
EVEN = [f"ar_{n}" for n in AR_EVEN] + [f"ramp_{n}" for n in RAMP_EVEN] + [f"cos_{c}" for c in COS]
LAYOUT_M = [1, 2, 15, 16, 17, 63, 65, 129]
TOL = 1e-10    # relative tolerance on f0 and sum: the project's parity class
MARGIN = 1e-7  # what the generator asserts of every even-n column: 500 x TOL, so cut and the integer cannot flip inside TOL


def _ar(n, p):
    e = np.random.default_rng(SEED).normal(size=(n, p))
    phi = 1.0 - np.logspace(-3, 0, p)
    x = np.empty((n, p))
    x[0] = e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    return x + 5.0


def cosine(c):
    """One column of n = 4 c - 2 rows whose first negative lag is exactly c: f[k] is proportional to cos(2 pi k / n), which
    changes sign between k = c - 1 (angle pi / 2 - pi / n) and k = c (pi / 2 + pi / n); the margin is sin(pi / n)."""
    n = 4 * c - 2
    return (3.0 + 2.0 * np.cos(2.0 * np.pi * np.arange(n) / n)).reshape(n, 1)


def case(name):
    """The input of a golden case, drawn again from its seed: always two-dimensional, (n, columns)."""
    kind, _, arg = name.partition("_")
    if kind == "ar":
        return _ar(int(arg), AR[int(arg)])
    if kind == "ramp":
        return (np.arange(int(arg)) * 0.25 - 7.0).reshape(-1, 1)
    if kind == "cos":
        return cosine(int(arg))
    if name == "layout":
        e = np.random.default_rng(SEED + 1).normal(size=(258, 129))
        phi = np.linspace(0.0, 0.9, 129)
        x = np.empty_like(e)
        x[0] = e[0]
        for i in range(1, 258):
            x[i] = phi * x[i - 1] + e[i]
        return x - 2.0
    if name == "const":
        a = np.column_stack([np.full(64, 3.0), np.arange(64.0), np.full(64, 3.0)])
        a[40, 2] = np.nan
        return a
    if name == "tiny_2":
        return np.array([[1.0], [2.0]])
    if name == "tiny_4":
        return np.array([[0.3], [-1.1], [0.9], [-0.4]])
    raise KeyError(name)


def ends(a):
    """First and last 8 values of a drawn array."""
    return np.concatenate([np.ravel(a)[:8], np.ravel(a)[-8:]])


def checked_case(g, name):
    """`case(name)`, checked against the ends that the golden file recorded when the reference ran on it."""
    a = case(name)
    np.testing.assert_array_equal(ends(a), g[f"{name}_ends"], err_msg=f"the seeded recipe of {name} drew other numbers")
    return a


def mirror_column(x):
    """(f0, sum, cut, ess, f[0 .. cut]) of one column by direct lag sums; cut = 0 and ess = -1 when no lag in
    [1, n // 2) is negative."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    y = x - x.mean()
    wrapped = np.concatenate([y, y[: n // 2]])
    f = [float(np.dot(y, y))]
    for k in range(1, n // 2):
        f.append(float(np.dot(y, wrapped[k:k + n])))
        if f[-1] < 0.0:
            f = np.array(f)
            total = f[:k].sum()
            return f[0], total, k, int(n / (total / f[0])), f
    return f[0], 0.0, 0, -1, np.array(f)


def mirror(sample2d):
    """`mirror_column` over the columns: f0, sum (float64), cut, ess (int64)."""
    cols = [mirror_column(c)[:4] for c in np.asarray(sample2d).T]
    f0, total, cut, ess = zip(*cols)
    return np.array(f0), np.array(total), np.array(cut, dtype=np.int64), np.array(ess, dtype=np.int64)


def rebuilt_chain(g):
    """A `GibbsChain` carrying the stored state of the reference's chain of the `chain` case."""
    from inference_amd.mcmc import GibbsChain

    samples = g["chain_samples"]
    chain = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=samples[0], display_progress=False)
    for k, p in enumerate(chain.params):
        p.samples = list(samples[:, k])
        p.sigma = float(g["chain_sigma"][k])
        p.sigma_values = list(g[f"chain_sigma_values_{k}"])
        p.sigma_checks = list(g[f"chain_sigma_checks_{k}"])
    chain.probs = list(g["chain_probs"])
    chain.chain_length = samples.shape[0]
    return chain


def rebuilt_ladder(g):
    """A `ParallelTempering` of four idle chains carrying the stored swap counters."""
    from inference_amd.mcmc import GibbsChain, ParallelTempering

    chains = [GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(2), temperature=T,
                         display_progress=False) for T in (1.0, 2.0, 4.0, 8.0)]
    ladder = ParallelTempering(chains)
    ladder.attempted_swaps = g["swap_attempted"].copy()
    ladder.successful_swaps = g["swap_successful"].copy()
    return ladder
