"""
Affine-invariant ensemble sampler - counterpart of the reference's `EnsembleSampler` (mcmc/ensemble.py): the stretch
move of Goodman & Weare.  An ensemble of `n_walkers` points moves through parameter space; a walker at X_i proposes
X_i + z (X_j - X_i) with another walker X_j and a stretch z drawn from g(z) ~ 1 / sqrt(z) on [1 / alpha, alpha], and the
proposal is accepted with probability min(1, z^(P - 1) p(Y) / p(X_i)).

`update="serial"` (the default) is the reference's sweep, draw for draw: walker i moves against the CURRENT position of a
random other walker, which may have moved in this iteration already, so an ensemble asks for one posterior value at a
time.  Per attempt of walker i the generator `rng` gives `integers(low=1, high=n_walkers)` (the other walker is that many
places further on, modulo n_walkers), `random()` for the stretch z = (x_lwr + x_width u)^2 / 2, and, after the posterior
value p of the reflected proposal, `random()` for the accept test u <= exp((P - 1) log z + p - walker_probs[i]).

MI355X-specific additions: `update="split"` moves each half of the walkers against the frozen other half, so that one
ensemble fills batches of n_walkers / 2 rows (`batch_posterior`), and `advance_lockstep_ensembles` advances MANY ensembles,
serial or split, with one batched evaluation per round (`GpRegressor.marginal_likelihood_batch`).

Draw order of split mode (part of the interface).  The walkers [0, n_walkers // 2) are the set A, the others B; an
iteration is the half-sweep of A against B and then the half-sweep of B against A.  A half-sweep of S against its frozen
complement C keeps the walkers of S that have not accepted yet as its active list, in ascending order, and makes up to
`max_attempts` rounds.  One round of an active list of length k draws, in this order,
    j = C[rng.integers(0, len(C), size=k)]      the partner of every active walker
    u = rng.random(k)                           z = (x_lwr + x_width u)^2 / 2
    (the k reflected proposals are evaluated in ONE posterior call)
    a = rng.random(k)                           row r is accepted where a[r] <= exp((P - 1) log z[r] + p[r] - walker_probs[i_r])
and the accepted walkers commit, recording the number of the round as their attempt count; walkers still active after the
last round are recorded as failed, as in serial mode.  `max_attempts = 1` is the textbook parallel stretch move.
"""
import sys
from time import time

import numpy as np
from numpy import array, concatenate, cov, diag, exp, isfinite, linspace, log, median, ndarray, sqrt, triu, var
from numpy.random import default_rng

from inference_amd.mcmc.base import MarkovChain
from inference_amd.mcmc.utilities import Bounds
from inference_amd.pdf import _messages as msg

__all__ = ["EnsembleSampler", "advance_lockstep_ensembles"]


class EnsembleSampler(MarkovChain):
    """
    :param posterior: callable `theta (ndarray) -> float` log-probability.
    :param starting_positions: the walkers' starting positions, an ndarray of shape (n_walkers, n_parameters) with
        n_walkers >= n_parameters + 1.  The sampler keeps this array and moves the walkers in it (as the reference does).
    :param alpha: width of the distribution of the stretch z, which lies in [1 / alpha, alpha]; above 1.
    :param bounds: a `Bounds`, or a pair `(lower, upper)` of arrays; proposals are reflected into them.
    :param display_progress: print the progress of `advance`.
    :param update: "serial" (the reference's sweep) or "split" (half against half, see the module's docstring), which
        needs n_walkers >= 2 (n_parameters + 1).
    :param batch_posterior: callable `thetas (B, P) -> (B,)`.  When given it serves every evaluation of both modes (serial
        mode calls it with one row) and the starting probabilities come from one call of it; `posterior` may then be None.
    :param seed: seed of the sampler's generator `rng` (`numpy.random.default_rng`).  Constructing draws nothing.
    """

    def __init__(self, posterior, starting_positions, alpha: float = 2.0, bounds=None, display_progress=True, *,
                 update: str = "serial", batch_posterior=None, seed=None):
        self.posterior = posterior
        self.batch_posterior = batch_posterior
        self.rng = default_rng(seed)
        if update not in ("serial", "split"):
            raise ValueError(msg.ensemble_update(update))
        self.update = update

        if starting_positions is not None:
            if posterior is None and batch_posterior is None:
                raise ValueError(msg.ensemble_no_posterior())
            self.walker_positions = self._validate_starting_positions(starting_positions)
            # (a 1D array passed the checks as one column and stops here, as in the reference: ensemble.py:62)
            self.n_walkers, self.n_parameters = starting_positions.shape
            if update == "split" and self.n_walkers < 2 * (self.n_parameters + 1):
                raise ValueError(msg.ensemble_split_walkers(self.n_walkers, self.n_parameters))
            self.walker_probs = self._evaluate(self.walker_positions)
            self.n_iterations = 0
            self.chain_length = 0
            self.total_proposals = [[] for _ in range(self.n_walkers)]
            self.failed_updates = []

        if bounds is None:
            self.bounds = None
        else:
            if isinstance(bounds, Bounds):
                self.bounds = bounds
            else:
                try:
                    lower, upper = bounds
                except (TypeError, ValueError):
                    raise ValueError(msg.ensemble_bounds_type(type(bounds))) from None
                self.bounds = Bounds(lower=lower, upper=upper, error_source="EnsembleSampler")
            if hasattr(self, "walker_positions"):
                for v in self.walker_positions:
                    self.bounds.validate_start_point(v, error_source="EnsembleSampler")

        if not alpha > 1.0:
            raise ValueError(msg.ensemble_alpha())
        self.alpha = alpha
        # uniform in x with z = x^2 / 2 gives the density of z
        self.x_lwr = sqrt(2.0 / self.alpha)
        self.x_width = sqrt(2.0 * self.alpha) - self.x_lwr

        self.max_attempts = 100
        self.sample = None
        self.sample_probs = None
        self.display_progress = display_progress

    @staticmethod
    def _validate_starting_positions(positions):
        """ensemble.py:113-180."""
        if not isinstance(positions, ndarray):
            raise ValueError(msg.ensemble_positions_type(type(positions)))
        theta = positions.reshape([positions.size, 1]) if positions.ndim == 1 else positions
        if theta.ndim != 2 or theta.shape[0] < (theta.shape[1] + 1):
            raise ValueError(msg.ensemble_positions_shape(positions.shape))
        if not isfinite(theta).all():
            raise ValueError(msg.ensemble_positions_not_finite())
        if theta.shape[1] == 1:
            if var(theta) == 0:
                raise ValueError(msg.ensemble_zero_variance())
        else:
            covar = cov(theta.T)
            std_dev = sqrt(diag(covar))
            if (std_dev == 0).any():
                raise ValueError(msg.ensemble_zero_variance_columns())
            correlation = covar / (std_dev[:, None] * std_dev[None, :])
            if (abs(triu(correlation, k=1)) > 0.999).any():
                raise ValueError(msg.ensemble_colinear())
        return theta

    # -- evaluation and the two sweeps ----------------------------------------------------------
    def _evaluate(self, rows):
        """The log-probabilities of the rows: one `batch_posterior` call, or `posterior` row by row."""
        if self.batch_posterior is not None:
            return array(self.batch_posterior(rows), dtype=float).reshape(len(rows))
        return array([self.posterior(t) for t in rows])

    def process_proposal(self, prop):
        """The proposal (or the rows of proposals) reflected into the bounds; itself without bounds."""
        return prop if self.bounds is None else self.bounds.reflect(prop)

    def _serial_sweep(self):
        """One iteration of the reference (ensemble.py:182-210); yields one proposal row per attempt."""
        X, probs, n = self.walker_positions, self.walker_probs, self.n_walkers
        for i in range(n):
            for attempts in range(1, self.max_attempts + 1):
                j = (self.rng.integers(low=1, high=n) + i) % n
                z = 0.5 * (self.x_lwr + self.x_width * self.rng.random()) ** 2
                Y = self.process_proposal(X[i, :] + z * (X[j, :] - X[i, :]))
                p = (yield Y[None, :])[0]
                with np.errstate(over="ignore"):  # (a ratio beyond the doubles is +inf: accepted)
                    q = exp((self.n_parameters - 1) * log(z) + p - probs[i])
                if self.rng.random() <= q:
                    X[i, :] = Y
                    probs[i] = p
                    self.total_proposals[i].append(attempts)
                    break
            else:
                self.total_proposals[i].append(self.max_attempts)
                self.failed_updates[-1] += 1

    def _half_sweep(self, S, C):
        """The walkers `S` against the frozen walkers `C`; yields the proposals of the active list, one round at a time."""
        X, probs = self.walker_positions, self.walker_probs
        active = S
        for attempts in range(1, self.max_attempts + 1):
            k = active.size
            j = C[self.rng.integers(0, C.size, size=k)]
            z = 0.5 * (self.x_lwr + self.x_width * self.rng.random(k)) ** 2
            Xi = X[active]
            Y = self.process_proposal(Xi + z[:, None] * (X[j] - Xi))
            p = yield Y
            a = self.rng.random(k)
            with np.errstate(over="ignore"):
                accepted = a <= exp((self.n_parameters - 1) * log(z) + p - probs[active])
            moved = active[accepted]
            X[moved] = Y[accepted]
            probs[moved] = p[accepted]
            for i in moved:
                self.total_proposals[i].append(attempts)
            active = active[~accepted]
            if not active.size:
                return
        for i in active:
            self.total_proposals[i].append(self.max_attempts)
            self.failed_updates[-1] += 1

    def _rounds(self, iterations: int, progress=None):
        """The sampler's work for `iterations` iterations as a generator: it yields (rows, P) arrays of proposals and is
        sent their log-probabilities, (rows,).  `advance` drives one of these and `advance_lockstep_ensembles` many.  The
        iterations completed when it ends, or is abandoned, are joined to `sample` and `sample_probs`."""
        sample_arrays = [] if self.sample is None else [self.sample]
        prob_arrays = [] if self.sample_probs is None else [self.sample_probs]
        half = self.n_walkers // 2
        A, B = np.arange(half), np.arange(half, self.n_walkers)
        try:
            for k in range(iterations):
                self.failed_updates.append(0)
                if self.update == "serial":
                    yield from self._serial_sweep()
                else:
                    yield from self._half_sweep(A, B)
                    yield from self._half_sweep(B, A)
                self.n_iterations += 1
                sample_arrays.append(self.walker_positions.copy())
                prob_arrays.append(self.walker_probs.copy())
                if progress is not None:
                    progress(k)
        finally:
            del self.failed_updates[self.n_iterations:]  # (an iteration that was abandoned half-way leaves no counts)
            for counts in self.total_proposals:
                del counts[self.n_iterations:]
            if sample_arrays:
                self.sample = concatenate(sample_arrays)
                self.sample_probs = concatenate(prob_arrays)
                self.chain_length = self.sample_probs.size

    def advance(self, iterations: int):
        """Advance the ensemble by `iterations` iterations.  Every iteration stores the positions of all walkers: the
        sample grows by `iterations * n_walkers` rows."""
        t_start = time()
        group = max(iterations // 100, 1)

        def progress(k):
            if self.display_progress and (k + 1) % group == 0:
                eta = int((time() - t_start) * (iterations / (k + 1) - 1))
                self._print(f"[ {int(100 * (k + 1) / iterations)}% complete  |  ETA: {eta} sec ]    ")

        rounds = self._rounds(iterations, progress)
        try:
            rows = next(rounds)
            while True:
                rows = rounds.send(self._evaluate(rows))
        except StopIteration:
            pass
        if self.display_progress:
            self._print(f"[ complete - {iterations} iterations taken in {int(time() - t_start)} sec ]      \n")

    @staticmethod
    def _print(text):
        sys.stdout.write(f"\r  EnsembleSampler:   {text}")
        sys.stdout.flush()

    # -- results (ensemble.py:290-353; `burn` defaults to 0 here, to 1 in the chains) ------------
    def mode(self) -> ndarray:
        """The sample with the highest log-probability so far."""
        return self.sample[self.sample_probs.argmax(), :]

    def get_parameter(self, index: int, burn=0, thin=1) -> ndarray:
        return self.sample[burn::thin, index]

    def get_probabilities(self, burn=0, thin=1) -> ndarray:
        return self.sample_probs[burn::thin]

    def get_sample(self, burn=0, thin=1) -> ndarray:
        return self.sample[burn::thin, :]

    # -- diagnostics (ensemble.py:244-288) -------------------------------------------------------
    def diagnostics_data(self, burn: int = 0, *, ess=False, device=None) -> dict:
        """The arrays that `plot_diagnostics` draws: the iteration axis, the cumulative acceptance rate of every walker
        (iterations over proposals so far, shape (n_walkers, n_iterations)) and their mean over the walkers, the
        log-probabilities as (n_iterations, n_walkers) with their median over the walkers and the limits of that panel,
        and the number of walkers per iteration that used up `max_attempts`.  With `ess=True` also `ess`, the effective
        sample size of every walker's series of every parameter from iteration `burn` on, as an (n_walkers, P) integer
        array from ONE device call (`effective_sample_size_batch` on (iterations - burn) rows and n_walkers * P columns),
        which raises what that function raises.  `burn` counts iterations and applies to `ess` only."""
        n, w = self.n_iterations, self.n_walkers
        x = linspace(1, n, n)
        rates = x / array(self.total_proposals).cumsum(axis=1)
        itr_probs = self.sample_probs.reshape([n, w])
        floor = itr_probs[n // 2:, :].min()
        data = {
            "iterations": x,
            "acceptance_rates": rates,
            "mean_acceptance_rate": rates.mean(axis=0),
            "probs": itr_probs,
            "median_probs": median(itr_probs, axis=1),
            "prob_ylims": [floor, self.sample_probs.max() * 1.1 - 0.1 * floor],
            "failed_updates": array(self.failed_updates),
        }
        if ess:
            from inference_amd.mcmc.utilities import effective_sample_size_batch

            series = self.sample.reshape(n, w * self.n_parameters)[burn:]
            data["burn"] = burn
            data["ess"] = effective_sample_size_batch(series, device=device).reshape(w, self.n_parameters)
        return data

    def plot_diagnostics(self, show=True, filename=None):
        """Plot the acceptance rate and the log-probability of every walker against the number of iterations.  Returns
        the figure (the reference returns None)."""
        data = self.diagnostics_data()

        import matplotlib.pyplot as plt

        x = data["iterations"]
        fig = plt.figure(figsize=(10, 4))
        ax1 = fig.add_subplot(121)
        opacity = max(0.01, min(1, 20.0 / float(self.n_walkers)))
        for rates in data["acceptance_rates"]:
            ax1.plot(x, rates, lw=0.5, c="C0", alpha=opacity)
        ax1.plot(x, data["mean_acceptance_rate"], lw=2, c="red", label="mean rate of all walkers")
        ax1.set_ylim([0, 1])
        ax1.grid()
        ax1.legend()
        ax1.set_title("walker acceptance rates")
        ax1.set_xlabel("iteration")
        ax1.set_ylabel("average acceptance rate per walker")

        ax2 = fig.add_subplot(122)
        ax2.plot(x, data["probs"], marker=".", ls="none", c="C0", alpha=0.05)
        ax2.plot(x, data["median_probs"], c="red", lw=2, label="median walker log-probability")
        ax2.set_ylim(data["prob_ylims"])
        ax2.grid()
        ax2.legend()
        ax2.set_title("walker log-probabilities")
        ax2.set_xlabel("iteration")
        ax2.set_ylabel("walker log-probability")

        fig.tight_layout()
        if filename is not None:
            fig.savefig(filename)
        if show:
            plt.show()
        return fig

    # -- save / load (ensemble.py:355-411) -------------------------------------------------------
    def save(self, filename):
        """Write the sampler's state as an .npz file of plain arrays: the reference's keys (a file written here loads in
        the reference and the other way round) and, beside them, `failed_updates`, `update` and the state of the
        generator when it is a PCG64 (what `default_rng` makes; another bit generator's state is not written)."""
        D = {
            "walker_positions": self.walker_positions,
            "n_parameters": self.n_parameters,
            "n_walkers": self.n_walkers,
            "walker_probs": self.walker_probs,
            "n_iterations": self.n_iterations,
            "total_proposals": array(self.total_proposals),
            "alpha": self.alpha,
            "max_attempts": self.max_attempts,
            "display_progress": self.display_progress,
            "failed_updates": array(self.failed_updates, dtype=np.int64),
            "update": array(self.update),
        }
        if self.bounds is not None:
            D["lower_bounds"] = self.bounds.lower
            D["upper_bounds"] = self.bounds.upper
        if self.sample is not None:
            D["sample"] = self.sample
            D["sample_probs"] = self.sample_probs
        state = self.rng.bit_generator.state
        if state["bit_generator"] == "PCG64":
            words = [state["state"]["state"], state["state"]["inc"]]
            D["rng_pcg64"] = array([[v >> 64, v & (2 ** 64 - 1)] for v in words], dtype=np.uint64)
            D["rng_uint32"] = array([state["has_uint32"], state["uinteger"]], dtype=np.uint64)
        np.savez(filename, **D)

    @classmethod
    def load(cls, filename, posterior=None, batch_posterior=None):
        """The sampler that `save` (here or in the reference) wrote to `filename`.  Unlike the reference's, it can be
        advanced: `chain_length` is restored, and `failed_updates` too (zeros when the file, written by the reference,
        does not hold them).  A file without the generator's state gives a sampler with a fresh `default_rng()`."""
        D = np.load(filename, allow_pickle=False)
        bounds = None
        if all(k in D for k in ["lower_bounds", "upper_bounds"]):
            bounds = Bounds(lower=D["lower_bounds"], upper=D["upper_bounds"], error_source="EnsembleSampler")
        sampler = cls(posterior=posterior, starting_positions=None, bounds=bounds, alpha=float(D["alpha"]),
                      display_progress=bool(D["display_progress"]), batch_posterior=batch_posterior,
                      update=str(D["update"]) if "update" in D else "serial")
        sampler.walker_positions = D["walker_positions"]
        sampler.n_parameters = int(D["n_parameters"])
        sampler.n_walkers = int(D["n_walkers"])
        sampler.walker_probs = D["walker_probs"]
        sampler.n_iterations = int(D["n_iterations"])
        sampler.total_proposals = [[int(c) for c in v] for v in D["total_proposals"]]
        sampler.max_attempts = int(D["max_attempts"])
        if "failed_updates" in D:
            sampler.failed_updates = [int(c) for c in D["failed_updates"]]
        else:
            sampler.failed_updates = [0] * sampler.n_iterations
        sampler.chain_length = 0
        if "sample" in D:
            sampler.sample = D["sample"]
            sampler.sample_probs = D["sample_probs"]
            sampler.chain_length = sampler.sample_probs.size
        if "rng_pcg64" in D:
            words = [(int(hi) << 64) | int(lo) for hi, lo in D["rng_pcg64"]]
            state = sampler.rng.bit_generator.state
            state["state"] = {"state": words[0], "inc": words[1]}
            state["has_uint32"], state["uinteger"] = (int(v) for v in D["rng_uint32"])
            sampler.rng.bit_generator.state = state
        return sampler


def advance_lockstep_ensembles(samplers, iterations: int, batch_posterior, max_batch: int = None) -> int:
    """Advance every `EnsembleSampler` of `samplers` by `iterations` iterations with batched evaluations.

    `batch_posterior(thetas (B, P)) -> (B,)` is the log-probability of all of them (`GpRegressor.marginal_likelihood_batch`
    has this signature; for a bound method of an object with `batch_independent_values`, batch-independent values are
    switched on).  Every round, each sampler that still has work contributes the rows it waits for - a serial sampler ONE,
    the proposal of its current attempt, a split sampler the active list of its current half-sweep - and the round is one
    call of `batch_posterior`, or calls of at most `max_batch` rows.  Samplers retry on their own, so they drift apart
    inside a call and meet again at its end; serial and split samplers, with any settings, can be mixed.

    A sampler draws from its own generator only and does here what `advance` does: both drive the same generator of
    rounds.  Identity: if a sampler's own evaluations agree row for row, bit for bit, with `batch_posterior` (on the
    device: they go through this function too, with `batch_independent_values(True)`), its trajectory - `sample`,
    `sample_probs`, `walker_positions`, `walker_probs`, `total_proposals`, `failed_updates` - is the one `advance` gives it
    alone.

    Returns the number of rows evaluated, which is the growth of the sum of all `total_proposals`."""
    samplers = list(samplers)
    if not samplers or iterations <= 0:
        return 0
    sizes = sorted({s.n_parameters for s in samplers})
    if len(sizes) > 1:
        raise ValueError(msg.lockstep_ensembles_mixed(sizes))
    owner = getattr(batch_posterior, "__self__", None)
    if hasattr(owner, "batch_independent_values"):
        owner.batch_independent_values(True)  # ragged rounds: a row must not depend on its batch

    waiting = []  # (a sampler's generator of rounds, the rows it waits for)
    for s in samplers:
        rounds = s._rounds(iterations)
        waiting.append((rounds, next(rounds)))
    evals = 0
    while waiting:
        rows = concatenate([r for _, r in waiting])
        values = np.empty(len(rows))
        size = max_batch or len(rows)
        for lo in range(0, len(rows), size):
            values[lo:lo + size] = batch_posterior(rows[lo:lo + size])
        evals += len(rows)
        still, at = [], 0
        for rounds, r in waiting:
            try:
                still.append((rounds, rounds.send(values[at:at + len(r)])))
            except StopIteration:
                pass
            at += len(r)
        waiting = still
    return evals
