"""Shared pieces of the HamiltonianChain tests (test infrastructure only): the analytic posterior and the seeded recipes of
golden/hmc.npz (golden/make_golden_hmc.py builds the reference's chains from here too), a recorder of the margins by
which a run's random decisions were taken, and the chain restored from the fixture for the read-out tests."""
import numpy as np
from numpy.random import default_rng

M = np.array([0.0, 1.0, 2.0])
S = np.array([1.0, 0.4, 2.5])
START = np.array([1.5, 0.5, 3.0])
LOWER = np.array([-2.0, -0.5, -3.0])
UPPER = np.array([2.5, 2.0, 6.0])
FULL = np.array([[1.0, 0.2, 0.1], [0.2, 0.16, 0.05], [0.1, 0.05, 6.25]])  # a full inverse mass (a covariance)
SEED = 5
STEPS = 12
LONG = 2000  # steps of the chain behind the read-out tests (length 2001)

# name -> (constructor keywords, steps to take); `grad` is added by `build` unless the case asks for finite differences
CASES = {
    "scalar": (dict(epsilon=0.2), 300),
    "vector": (dict(inverse_mass=S ** 2, temperature=2.5, bounds=(LOWER, UPPER)), 300),
    "matrix": (dict(inverse_mass=FULL), 300),
    "fdiff": (dict(grad=None, temperature=2.0), 150),
}


def posterior(t):
    """A bounded coupling of the first two parameters on top of independent normals (a polynomial coupling makes the
    reference overflow once epsilon has grown)."""
    return float(-0.5 * np.sum(((t - M) / S) ** 2) - 0.5 * np.log1p((t[0] * t[1]) ** 2))


def gradient(t):
    g = -(t - M) / S ** 2
    c = t[0] * t[1]
    g[0] -= c * t[1] / (1.0 + c * c)
    g[1] -= c * t[0] / (1.0 + c * c)
    return g


def batch(thetas):
    """The batched form that `advance_lockstep_hmc` takes, row by row from the two functions above."""
    return np.array([posterior(t) for t in thetas]), np.array([gradient(t) for t in thetas])


def build(cls, name=None, seed=SEED, **kwargs):
    """A chain of class `cls` (this package's or the reference's) for the case `name`, or for the given keywords."""
    kw = dict(posterior=posterior, grad=gradient)
    kw.update(CASES[name][0] if name else {})
    kw.update(kwargs)
    chain = cls(start=START.copy(), display_progress=False, **kw)
    chain.rng = default_rng(seed)
    chain.steps = STEPS
    return chain


def state(chain):
    """Everything the identity claims are about."""
    return {"theta": np.array(chain.theta), "probs": np.array(chain.probs), "leapfrog_steps": np.array(chain.leapfrog_steps),
            "epsilon_values": np.array(chain.ES.epsilon_values), "epsilon_checks": np.array(chain.ES.epsilon_checks)}


class _Draws:
    """Stands in for a chain's generator and logs what is drawn."""

    def __init__(self, rng, events):
        self._rng, self._events = rng, events

    def normal(self, **kwargs):
        self._events.append(("momentum", None))
        return self._rng.normal(**kwargs)

    def random(self):
        u = self._rng.random()
        self._events.append(("uniform", u))
        return u


class Recorder:
    """Watches a chain (of either package) through its public seams - `rng`, `ES.add_probability`, `ES.update_epsilon` -
    and reports how far every random decision of the run was from going the other way."""

    def __init__(self, chain):
        self.chain = chain
        self.events = []
        self.reviews = []
        chain.rng = _Draws(chain.rng, self.events)
        es = chain.ES
        add, review = es.add_probability, es.update_epsilon

        def add_probability(p):
            self.events.append(("accept_prob", p))
            add(p)

        def update_epsilon():
            rate, spread = es.avg / es.num, np.sqrt(es.var) / es.num
            self.reviews.append(min(abs(es.accept_rate - (rate - 2 * spread)), abs(es.accept_rate - (rate + 2 * spread)))
                                / es.accept_rate)
            review()

        es.add_probability, es.update_epsilon = add_probability, update_epsilon

    def margins(self):
        """(accept, steps, review, retries): the smallest |u - accept_prob| over the accept tests that drew a uniform, the
        smallest distance of steps * (1 + (u - 0.5) * 0.2) from an integer, the smallest relative distance of the target
        rate from the 2-sigma edges of an epsilon review, and the number of rejected attempts."""
        accept, steps, retries = np.inf, np.inf, 0
        for k, (kind, value) in enumerate(self.events):
            if kind != "uniform":
                continue
            before = self.events[k - 1]
            if before[0] == "momentum":
                x = self.chain.steps * (1 + (value - 0.5) * 0.2)
                steps = min(steps, abs(x - round(x)))
            else:
                assert before[0] == "accept_prob"
                accept = min(accept, abs(value - before[1]))
                retries += not value <= before[1]
        return accept, steps, min(self.reviews, default=np.inf), retries


def rebuilt_chain(g):
    """A `HamiltonianChain` carrying the stored state of the reference's long chain: no sampling."""
    from inference_amd.mcmc import HamiltonianChain

    chain = build(HamiltonianChain, "scalar")
    chain.theta = list(g["long_theta"])
    chain.probs = list(g["long_probs"])
    chain.leapfrog_steps = list(g["long_leapfrog_steps"])
    chain.chain_length = len(chain.theta)
    chain.ES.epsilon_values = list(g["long_epsilon_values"])
    chain.ES.epsilon_checks = list(g["long_epsilon_checks"])
    chain.ES.epsilon = float(g["long_epsilon_values"][-1])
    return chain
