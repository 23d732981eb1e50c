"""Shared pieces of the EnsembleSampler tests (test infrastructure only): the posteriors and seeded recipes of
golden/ensemble.npz (golden/make_golden_ensemble.py builds the reference's samplers from here too), a recorder of every
accept test of a run, and a NumPy mirror of split mode written walker by walker.

The posteriors are sums and products of the parameters only, so their bits do not depend on a maths library."""
import numpy as np
from numpy.random import default_rng

SEED = 11
STATE_KEYS = ("sample", "sample_probs", "walker_positions", "walker_probs", "total_proposals", "failed_updates")


def post_a(t):
    """Two parameters with correlation 0.8."""
    return float(-(t[0] * t[0] - 1.6 * t[0] * t[1] + t[1] * t[1]) * 1.375)


def post_b(t):
    """Three parameters, the first two coupled, around (0.5, -0.25, 1)."""
    a, b, c = t[0] - 0.5, t[1] + 0.25, t[2] - 1.0
    return float(-0.5 * (a * a + 4.0 * b * b + 0.25 * c * c + a * b))


def post_c(t):
    """A quartic double well in one parameter."""
    s = t[0] * t[0] - 1.0
    return float(-2.0 * s * s)


def post_d(t):
    """A narrow target: most stretches of a wide ensemble are rejected."""
    a, b = t[0] - 0.3, t[1] + 0.2
    return float(-2000.0 * (a * a + b * b))


LOWER_B = np.array([-0.5, -1.0, -1.0])
UPPER_B = np.array([1.5, 0.75, 3.0])

# name -> posterior, parameters, walkers, iterations, centre and half-width of the box the walkers start in, the
# constructor's keywords and max_attempts
CASES = {
    "a": dict(post=post_a, P=2, walkers=12, iterations=40, centre=[0.0, 0.0], spread=[1.5, 1.5], kw={}, max_attempts=100),
    "b": dict(post=post_b, P=3, walkers=8, iterations=40, centre=[0.5, -0.125, 1.0], spread=[0.9, 0.8, 1.9],
              kw=dict(alpha=3, bounds=(LOWER_B, UPPER_B)), max_attempts=100),
    "c": dict(post=post_c, P=1, walkers=4, iterations=60, centre=[0.0], spread=[1.5], kw={}, max_attempts=100),
    "d": dict(post=post_d, P=2, walkers=6, iterations=30, centre=[0.3, -0.2], spread=[0.5, 0.5], kw={}, max_attempts=3),
}
MORE = 10  # iterations that golden case b goes on for after save / load, on a generator seeded SEED + 1


def batch_of(post):
    """The batched form of a posterior, row by row: the same bits."""
    def batch(rows):
        return np.array([post(t) for t in rows])

    return batch


def starts(name, walkers=None):
    """Seeded starting positions of a case, uniform in its box (uniform draws and arithmetic only)."""
    case = CASES[name]
    walkers = walkers or case["walkers"]
    u = default_rng(1000 + walkers).random((walkers, case["P"]))
    return np.array(case["centre"]) + np.array(case["spread"]) * (2.0 * u - 1.0)


def build(cls, name, seed=SEED, walkers=None, max_attempts=None, **kwargs):
    """A sampler of class `cls` (this package's or the reference's) for the case `name`; further keywords go to the
    constructor.  This package's class gets its seed there, the reference's a generator after construction."""
    case = CASES[name]
    kw = dict(case["kw"])
    kw.update(kwargs)
    ours = cls.__module__.startswith("inference_amd")
    if ours:
        kw["seed"] = seed
    sampler = cls(posterior=case["post"], starting_positions=starts(name, walkers), display_progress=False, **kw)
    if not ours:
        sampler.rng = default_rng(seed)
    sampler.max_attempts = max_attempts or case["max_attempts"]
    return sampler


def state(sampler):
    """Everything the identity claims are about."""
    return {"sample": np.array(sampler.sample), "sample_probs": np.array(sampler.sample_probs),
            "walker_positions": np.array(sampler.walker_positions), "walker_probs": np.array(sampler.walker_probs),
            "total_proposals": np.array(sampler.total_proposals), "failed_updates": np.array(sampler.failed_updates)}


class _Draws:
    """Stands in for a sampler's generator and tells the recorder what is drawn."""

    def __init__(self, rng, recorder):
        self._rng, self._rec = rng, recorder

    def integers(self, *args, **kwargs):
        return self._rng.integers(*args, **kwargs)

    def random(self, *args, **kwargs):
        u = self._rng.random(*args, **kwargs)
        self._rec.uniform(u)
        return u


class Recorder:
    """Watches a sampler that is advanced by `advance` (of either package in serial mode, of this package in split mode)
    through its public seams - `rng`, `posterior`, `batch_posterior` - and lists every accept test as (u, q, p): the
    uniform drawn, the acceptance ratio exp((P - 1) log z + p - walker_probs[i]) and the log-probability p of the
    proposal.  The walkers a draw belongs to are those that have no attempt count for the running iteration yet: the
    first of them in serial mode, those of the running half in split mode."""

    def __init__(self, sampler):
        self.s = sampler
        self.tests = []
        self.split = getattr(sampler, "update", "serial") == "split"
        self._z = self._p = None
        sampler.rng = _Draws(sampler.rng, self)
        if getattr(sampler, "batch_posterior", None) is not None:
            inner_batch = sampler.batch_posterior

            def batch(rows):
                self._p = np.array(inner_batch(rows), dtype=float)
                return self._p

            sampler.batch_posterior = batch
        else:
            inner = sampler.posterior

            def posterior(t):
                p = inner(t)
                self._p = p if self._p is None else np.append(self._p, p)
                return p

            sampler.posterior = posterior

    def _active(self):
        s = self.s
        waiting = np.array([len(c) == s.n_iterations for c in s.total_proposals])
        if not self.split:
            return np.flatnonzero(waiting)[:1]
        half = s.n_walkers // 2
        first = np.flatnonzero(waiting[:half])
        return first if first.size else half + np.flatnonzero(waiting[half:])

    def uniform(self, u):
        s = self.s
        u = np.atleast_1d(u)
        if self._z is None:  # the stretch; the proposals' values follow
            self._z = 0.5 * (s.x_lwr + s.x_width * u) ** 2
            self._p = None
            return
        p = np.atleast_1d(self._p)
        active = self._active()
        assert active.size == u.size == p.size == self._z.size
        q = np.exp((s.n_parameters - 1) * np.log(self._z) + p - s.walker_probs[active])
        self.tests += list(zip(u, q, p))
        self._z = self._p = None

    def margins(self):
        """(margin, largest |p|): the smallest |u - q| over the accept tests with q < 1 + 1e-6 (a test with a larger q
        is decided whatever u is), and the largest |p| of a proposal."""
        t = np.array(self.tests)
        close = t[:, 1] < 1.0 + 1e-6
        return np.abs(t[close, 0] - t[close, 1]).min() if close.any() else np.inf, np.abs(t[:, 2]).max()


def split_mirror(post, start, iterations, alpha=2.0, bounds=None, max_attempts=100, seed=SEED):
    """Split mode walker by walker, with scalar arithmetic: the state that `EnsembleSampler(update="split")` must reach."""
    from inference_amd.mcmc import Bounds

    rng = default_rng(seed)
    X = np.array(start, dtype=float)
    W, P = X.shape
    box = None if bounds is None else Bounds(lower=bounds[0], upper=bounds[1])
    probs = np.array([post(t) for t in X])
    x_lwr = np.sqrt(2.0 / alpha)
    x_width = np.sqrt(2.0 * alpha) - x_lwr
    total, failed, sample, sample_probs = [[] for _ in range(W)], [], [], []
    A, B = list(range(W // 2)), list(range(W // 2, W))
    for _ in range(iterations):
        failed.append(0)
        for S, C in ((A, B), (B, A)):
            active = list(S)
            for attempt in range(1, max_attempts + 1):
                k = len(active)
                partner = rng.integers(0, len(C), size=k)
                u = rng.random(k)
                z = 0.5 * (x_lwr + x_width * u) ** 2
                proposals = []
                for r, i in enumerate(active):
                    y = X[i] + z[r] * (X[C[partner[r]]] - X[i])
                    proposals.append(y if box is None else box.reflect(y))
                p = [post(y) for y in proposals]
                a = rng.random(k)
                left = []
                for r, i in enumerate(active):
                    if a[r] <= np.exp((P - 1) * np.log(z[r]) + p[r] - probs[i]):
                        X[i], probs[i] = proposals[r], p[r]
                        total[i].append(attempt)
                    else:
                        left.append(i)
                active = left
                if not active:
                    break
            for i in active:
                total[i].append(max_attempts)
                failed[-1] += 1
        sample.append(X.copy())
        sample_probs.append(probs.copy())
    return {"sample": np.concatenate(sample), "sample_probs": np.concatenate(sample_probs), "walker_positions": X,
            "walker_probs": probs, "total_proposals": np.array(total), "failed_updates": np.array(failed)}
