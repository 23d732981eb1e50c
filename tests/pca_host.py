"""Shared pieces of the PcaChain tests (test infrastructure only): the analytic posteriors and the seeded recipes of
golden/pca.npz (golden/make_golden_pca.py builds the reference's chains from here too), a recorder of the margins by which
a run's random decisions were taken, and the integer data of the exact covariance tests.

The posteriors are correlated Gaussians written out in scalar Python arithmetic (no BLAS, no LAPACK): the same doubles
wherever they run."""
import numpy as np
from numpy.random import default_rng

STEPS = 300          # two direction updates, at chain lengths 100 and 250
UPDATES = [100, 250]
UPDATE_ROWS = [99, 149]  # get_parameter(i)[last_update:] keeps burn = 1: samples 1 .. 99 and 101 .. 249
RIPPLE = 2.0 ** -44  # relative ripple put on the reference's covariance for the device tolerance


def _precision(sds, pairs):
    """Upper-triangle terms (i, j, a) of the quadratic form of independent normals with the given standard deviations,
    except the listed (i, j, rho) pairs, which are correlated."""
    terms = {(i, i): 1.0 / (s * s) for i, s in enumerate(sds)}
    for i, j, rho in pairs:
        f = 1.0 / (1.0 - rho * rho)
        terms[(i, i)] = f / (sds[i] * sds[i])
        terms[(j, j)] = f / (sds[j] * sds[j])
        terms[(i, j)] = -2.0 * f * rho / (sds[i] * sds[j])
    return [(i, j, a) for (i, j), a in sorted(terms.items())]


def make_posterior(mean, sds, pairs):
    terms = _precision(sds, pairs)
    mean = [float(v) for v in mean]

    def posterior(t):
        d = [float(t[i]) - mean[i] for i in range(len(mean))]
        q = 0.0
        for i, j, a in terms:
            q += a * d[i] * d[j]
        return -0.5 * q

    return posterior


POSTERIOR3 = make_posterior([1.0, -0.5, 2.0], [1.0, 0.5, 2.0], [(0, 1, 0.95)])
# (scales a factor of ten apart: the five eigenvalues of the covariance stay well separated)
POSTERIOR5 = make_posterior([1.0, -0.5, 2.0, 0.0, 3.0], [1.0, 0.5, 10.0, 5.0, 0.25], [(0, 1, 0.95), (2, 3, -0.9)])
POSTERIOR1 = make_posterior([1.0], [0.5], [])

# name -> (posterior, start, widths, constructor keywords, seed).  The seeds are ones whose traces survive the ripples of
# the maker's robustness check (`rippled`, golden/make_golden_pca.py) and keep the logged sines within the sample's
# allowance under them: about one seed in a thousand does.
CASES = {
    "plain": (POSTERIOR3, [1.5, 0.0, 3.0], [0.5, 0.3, 1.0], dict(), 7171),
    "bounded": (POSTERIOR3, [1.5, 0.0, 3.0], [0.5, 0.3, 1.0],
                dict(temperature=2.0, bounds=(np.array([-2.0, -2.0, -4.0]), np.array([4.0, 1.5, 8.0]))), 289),
    "p5": (POSTERIOR5, [1.5, 0.0, 3.0, 0.5, 2.5], [0.5, 0.3, 3.0, 2.0, 0.2], dict(), 2833),
}


def batch_of(posterior):
    """The batched form that the lockstep drivers take, row by row from the scalar posterior."""
    return lambda thetas: np.array([posterior(t) for t in thetas])


def numpy_covariance(rows):
    return np.cov(rows.T)


ROBUST_RIPPLES = 48


def rippled(k):
    """Ripple k of the maker's robustness check: `cov -> cov * (1 + a r)` with a = 2^-44, 2^-46, ... 2^-52 in turn and a
    fresh symmetric matrix r of uniform numbers in [-1, 1] at every call, from a generator seeded with 1000 + k."""
    amplitude = 2.0 ** -(44 + 2 * (k % 5))
    rng = default_rng(1000 + k)

    def ripple(cov):
        r = rng.uniform(-1.0, 1.0, cov.shape)
        r = np.triu(r) + np.triu(r, 1).T
        return cov * (1.0 + amplitude * r)

    return ripple


def build(cls, name, seed=None, **kwargs):
    """A chain of class `cls` (this package's or the reference's) for the case `name`; the generator is set after
    construction."""
    posterior, start, widths, kw, case_seed = CASES[name]
    kw = dict(kw)
    kw.update(kwargs)
    chain = cls(posterior=posterior, start=np.array(start), widths=list(widths), display_progress=False, **kw)
    chain.rng = default_rng(case_seed if seed is None else seed)
    return chain


def state(chain):
    """Everything the identity claims are about."""
    out = {"sample": np.array([p.samples for p in chain.params]).T, "probs": np.array(chain.probs),
           "update_history": np.array(chain.update_history, dtype=np.int64), "angles_history": np.array(chain.angles_history),
           "directions": np.array(chain.directions), "covar": np.array(chain.covar)}
    for i, p in enumerate(chain.params):
        out[f"sigma_values_{i}"] = np.array(p.sigma_values, dtype=np.float64)
        out[f"sigma_checks_{i}"] = np.array(p.sigma_checks, dtype=np.float64)
    return out


class _Draws:
    """Stands in for a chain's generator and logs what is drawn."""

    def __init__(self, rng, events):
        self._rng, self._events = rng, events

    def normal(self, *args, **kwargs):
        self._events.append(("normal", None))
        return self._rng.normal(*args, **kwargs)

    def random(self):
        u = self._rng.random()
        self._events.append(("uniform", u))
        return u


class Recorder:
    """Watches a chain (of either package) through its public seams - `rng`, every parameter's `submit_accept_prob` and
    `update_epsilon`, `update_directions` - and reports how far every decision of the run was from going the other way."""

    def __init__(self, chain):
        self.chain = chain
        self.events = []
        self.reviews = []
        self.components = []
        self.proposals = []  # cumulative number of proposals after every step
        chain.rng = _Draws(chain.rng, self.events)
        for par in chain.params:
            self._watch(par)
        update = chain.update_directions

        def update_directions():
            update()
            self.components.append(float(np.abs(np.array(chain.directions)).min()))

        chain.update_directions = update_directions

    def _watch(self, par):
        submit, review = par.submit_accept_prob, par.update_epsilon

        def submit_accept_prob(p):
            self.events.append(("accept_prob", float(p)))
            submit(p)

        def update_epsilon():
            rate, spread = par.avg / par.num, np.sqrt(par.var) / par.num
            self.reviews.append(min(abs(par.target_rate - (rate - 2 * spread)), abs(par.target_rate - (rate + 2 * spread)))
                                / par.target_rate)
            review()

        par.submit_accept_prob, par.update_epsilon = submit_accept_prob, update_epsilon

    def run(self, steps):
        for _ in range(steps):
            self.chain.take_step()
            self.proposals.append(sum(1 for kind, _ in self.events if kind == "normal"))

    def margins(self):
        """(accept, review, component): the smallest |u - accept_prob| over the accept tests that drew a uniform, the
        smallest relative distance of the target rate from the 2-sigma edges of a width review, and the smallest
        magnitude of a component of a direction."""
        accept = np.inf
        for k, (kind, value) in enumerate(self.events):
            if kind == "uniform":
                before = self.events[k - 1]
                assert before[0] == "accept_prob"
                accept = min(accept, abs(value - before[1]))
        return accept, min(self.reviews, default=np.inf), min(self.components, default=np.inf)


def exact_integers(rng, n, m):
    """Integers in [-1000, 1000] whose column sums are multiples of n - the first row is adjusted by the remainder, by at
    most n / 2, and may leave the range: the mean is exact, and so is every centred product and sum (|y| < 1000 + n,
    |S| <= n (1000 + n)^2 < 2^53 for the sizes of the tests)."""
    x = rng.integers(-1000, 1001, size=(n, m)).astype(np.float64)
    r = x.sum(axis=0) % n
    x[0] -= np.where(r <= n // 2, r, r - n)
    assert (x.sum(axis=0) % n == 0).all() and np.abs(x[1:]).max(initial=0) <= 1000 and np.abs(x[0]).max() <= 1000 + n // 2 + 1
    assert n * (2000.0 + n) ** 2 < 2.0 ** 53
    return x
