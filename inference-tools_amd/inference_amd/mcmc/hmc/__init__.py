"""
Hamiltonian Monte-Carlo chain - counterpart of the reference's `HamiltonianChain` (mcmc/hmc/__init__.py): proposals are
made by integrating Hamilton's equations with the negative log-posterior as the potential (leapfrog steps of size
epsilon, optionally reflected at parameter bounds), the step size is tuned towards a 65 % acceptance rate
(`EpsilonSelector`) and momenta are drawn for a scalar, vector or matrix mass.  One attempt draws from the chain's single
generator `rng` in the reference's order: the momentum, one uniform for the number of leapfrog steps, and one uniform
for the accept test when the acceptance probability is below one (or NaN).  `save` / `load` are out of scope.

MI355X-specific addition: `advance_lockstep_hmc` advances MANY chains together, with ONE batched value-and-gradient
evaluation (`GpRegressor.marginal_likelihood_gradient_batch`) per leapfrog round.
"""
import sys
from time import time

import numpy as np
from numpy import argmax, array, cov, exp, float64, isfinite, ndarray, var, zeros
from numpy.random import default_rng

from inference_amd.mcmc.base import MarkovChain
from inference_amd.mcmc.hmc.epsilon import EpsilonSelector
from inference_amd.mcmc.hmc.mass import MatrixMass, ScalarMass, VectorMass, get_particle_mass
from inference_amd.mcmc.utilities import Bounds
from inference_amd.pdf import _messages as msg

__all__ = ["HamiltonianChain", "advance_lockstep_hmc", "EpsilonSelector", "ScalarMass", "VectorMass", "MatrixMass",
           "get_particle_mass"]


class HamiltonianChain(MarkovChain):
    """
    :param posterior: callable `theta (ndarray) -> float` log-probability.
    :param start: starting parameter vector.
    :param grad: callable `theta -> ndarray`, the gradient of the log-probability; estimated by finite differences
        (`finite_diff`) when not given.
    :param epsilon: initial guess of the leapfrog step size.
    :param temperature: chain temperature T; the chain samples posterior ** (1 / T).
    :param bounds: a `Bounds`, or a pair `(lower, upper)` of arrays.
    :param inverse_mass: a scalar, a vector (approximately the variances of the marginals) or a matrix (approximately
        the covariance of the posterior).
    :param display_progress: print the progress of `advance` and `run_for`.
    """

    def __init__(self, posterior, start, grad=None, epsilon: float = 0.1, temperature: float = 1.0, bounds=None,
                 inverse_mass=None, display_progress: bool = True):
        self.posterior = posterior
        self.rng = default_rng()
        self.grad = self.finite_diff if grad is None else grad
        self.temperature = temperature
        self.inv_temp = 1.0 / temperature

        start = array(start, dtype=float64)  # (a copy: the chain's first sample is its own array)
        assert start.ndim == 1
        self._validate_posterior(posterior, start)
        self.theta = [start]
        self.probs = [self.posterior(start) * self.inv_temp]
        self.leapfrog_steps = [0]
        self.n_parameters = start.size
        self.mass = get_particle_mass(inverse_mass=inverse_mass if inverse_mass is not None else 1.0,
                                      n_parameters=self.n_parameters)
        self.chain_length = 1

        if bounds is None:
            self.run_leapfrog = self.standard_leapfrog
            self.bounds = None
        else:
            self.run_leapfrog = self.bounded_leapfrog
            self.bounds = bounds if isinstance(bounds, Bounds) else Bounds(lower=bounds[0], upper=bounds[1],
                                                                           error_source="HamiltonianChain")
            self.bounds.validate_start_point(start, error_source="HamiltonianChain")

        self.max_attempts = 200
        self.ES = EpsilonSelector(epsilon)
        self.steps = 50
        self.display_progress = display_progress
        # what `advance_lockstep_hmc` holds for theta[-1]: (that array, a copy of it, the un-tempered value and gradient there)
        self._held = None

    # -- stepping (hmc/__init__.py:127-194) ---------------------------------------------------
    def take_step(self):
        """One HMC step: trajectories from the last sample, each with a fresh momentum, until one is accepted."""
        steps_taken = 0
        for _ in range(self.max_attempts):
            r0, n_steps, H0 = self._draw_attempt()
            t, r = self.run_leapfrog(self.theta[-1].copy(), r0.copy(), n_steps)
            steps_taken += n_steps
            p = self.posterior(t) * self.inv_temp
            if self._accept(H0, r, p):
                break
        else:
            raise ValueError(msg.hmc_attempts(self.max_attempts))
        self._commit(t, p, steps_taken)

    def _draw_attempt(self):
        """The random part of one attempt: the momentum, then the number of leapfrog steps (within 10 % of `steps`);
        with them the Hamiltonian at the start."""
        r0 = self.mass.sample_momentum(self.rng)
        H0 = self.kinetic_energy(r0) - self.probs[-1]
        n_steps = int(self.steps * (1 + (self.rng.random() - 0.5) * 0.2))
        return r0, n_steps, H0

    def _accept(self, H0, r, p) -> bool:
        """The accept test of a trajectory that ended with momentum `r` at tempered log-probability `p`; its acceptance
        probability goes to the step-size selector (a non-finite one as zero)."""
        H = self.kinetic_energy(r) - p
        accept_prob = exp(H0 - H)
        self.ES.add_probability(min(accept_prob, 1) if isfinite(accept_prob) else 0.0)
        return (accept_prob >= 1) or (self.rng.random() <= accept_prob)

    def _commit(self, t, p, steps_taken):
        self.theta.append(t)
        self.probs.append(p)
        self.leapfrog_steps.append(steps_taken)
        self.chain_length += 1

    def standard_leapfrog(self, t: ndarray, r: ndarray, n_steps: int):
        r_step = self.inv_temp * self.ES.epsilon
        r += (0.5 * r_step) * self.grad(t)
        for _ in range(n_steps - 1):
            t += self.ES.epsilon * self.mass.get_velocity(r)
            r += r_step * self.grad(t)
        t += self.ES.epsilon * self.mass.get_velocity(r)
        r += (0.5 * r_step) * self.grad(t)
        return t, r

    def bounded_leapfrog(self, t: ndarray, r: ndarray, n_steps: int):
        """`standard_leapfrog` with every new position folded back into the bounds, the momentum reversed along the
        axes on which it was reflected an odd number of times."""
        r_step = self.inv_temp * self.ES.epsilon
        r += (0.5 * r_step) * self.grad(t)
        for _ in range(n_steps - 1):
            t += self.ES.epsilon * self.mass.get_velocity(r)
            t, reflections = self.bounds.reflect_momenta(t)
            r *= reflections
            r += r_step * self.grad(t)
        t += self.ES.epsilon * self.mass.get_velocity(r)
        t, reflections = self.bounds.reflect_momenta(t)
        r *= reflections
        r += (0.5 * r_step) * self.grad(t)
        return t, r

    def hamiltonian(self, t: ndarray, r: ndarray) -> float:
        return 0.5 * (r @ self.mass.get_velocity(r)) - self.posterior(t) * self.inv_temp

    def kinetic_energy(self, r: ndarray) -> float:
        return 0.5 * (r @ self.mass.get_velocity(r))

    def estimate_mass(self, burn=1, thin=1, diagonal=True):
        """Replace the mass by one estimated from the sample: its variances, or (`diagonal=False`) its covariance."""
        sample = array(self.theta[burn::thin])
        inverse_mass = var(sample, axis=0) if diagonal else cov(sample.T)
        self.mass = get_particle_mass(inverse_mass=inverse_mass, n_parameters=self.n_parameters)

    def finite_diff(self, t: ndarray) -> ndarray:
        """Forward differences of the TEMPERED log-probability with relative steps of 1e-5.  (As in the reference, the
        leapfrog multiplies what `grad` returns by 1 / T again: a chain without an analytic gradient at T != 1 moves in a
        potential tempered twice.)"""
        p = self.posterior(t) * self.inv_temp
        G = zeros(self.n_parameters)
        for i in range(self.n_parameters):
            delta = zeros(self.n_parameters) + 1
            delta[i] += 1e-5
            G[i] = (self.posterior(t * delta) * self.inv_temp - p) / (t[i] * 1e-5)
        return G

    def advance(self, m: int):
        """Advance the chain by `m` steps."""
        t_start = time()
        group = max(m // 100, 1)
        for j in range(m):
            self.take_step()
            if self.display_progress and (j + 1) % group == 0:
                eta = int((time() - t_start) * (m / (j + 1) - 1))
                self._print(f"[ {int(100 * (j + 1) / m)}% complete  |  ETA: {eta} sec ]    ")
        if self.display_progress:
            self._print(f"[ complete - {m} steps taken in {_clock(time() - t_start)} ]      \n")

    def run_for(self, minutes=0, hours=0, days=0):
        """Advance the chain for a chosen amount of computation time."""
        update_interval = 20
        start_length = self.chain_length
        run_time = ((days * 24.0 + hours) * 60.0 + minutes) * 60.0
        start_time = time()
        end_time = start_time + run_time
        steps_taken = 0
        while time() < end_time:
            for _ in range(update_interval):
                self.take_step()
            steps_taken = self.chain_length - start_length
            update_interval = max(int(steps_taken / (time() - start_time)), 1)  # about one report per second
            if self.display_progress:
                self._print(f"[ {steps_taken} steps taken, time remaining: {_clock(max(end_time - time(), 0))} ]    ")
        if self.display_progress:
            self._print(f"[ complete - {steps_taken} steps taken in {_clock(run_time)} ]      \n")

    @staticmethod
    def _print(text):
        sys.stdout.write(f"\r  advancing chain:   {text}")
        sys.stdout.flush()

    # -- state access -----------------------------------------------------------------------
    def get_last(self) -> ndarray:
        return self.theta[-1]

    def replace_last(self, theta: ndarray):
        self.theta[-1] = theta

    def get_parameter(self, index: int, burn: int = 1, thin: int = 1) -> ndarray:
        return array([v[index] for v in self.theta[burn::thin]]).squeeze()

    def get_probabilities(self, burn: int = 1, thin: int = 1) -> ndarray:
        return array(self.probs[burn::thin])

    def get_sample(self, burn: int = 1, thin: int = 1) -> ndarray:
        return array(self.theta[burn::thin])

    def mode(self) -> ndarray:
        """The sample with the highest log-probability so far."""
        return array(self.theta[argmax(self.probs)]).squeeze()

    # -- diagnostics (hmc/__init__.py:245-359, :399-408) ----------------------------------------
    def estimate_burn_in(self) -> int:
        """An estimate of the burn-in: the later of the step at which the chain first enters the top 1 % of its
        log-probabilities and the last review that found the step size more than 15 % away from its final value - which
        the log counts in ATTEMPTS, converted to steps by the target acceptance rate - and at most 0.9 of the chain.
        (As in the reference, a step size that never was that far away contributes its LAST review, the 0 that argmax
        gives for no match on the reversed log.)"""
        probs = array(self.probs)
        prob_estimate = argmax(probs > np.percentile(probs, 99))
        far = abs(array(self.ES.epsilon_values)[::-1] / self.ES.epsilon - 1.0) > 0.15
        checks = array(self.ES.epsilon_checks)[::-1]
        epsilon_estimate = checks[argmax(far)] * self.ES.accept_rate
        return int(min(max(prob_estimate, epsilon_estimate), 0.9 * self.chain_length))

    def diagnostics_data(self, burn=None, *, device=None) -> dict:
        """The arrays that `plot_diagnostics` draws.  `burn` defaults to `estimate_burn_in()`; `ess` holds the effective
        sample size of every parameter over `get_sample(burn=burn)`, from ONE device call for all of them
        (`effective_sample_size_batch`), and `ess_mean` / `ess_min` the integers of the text panel."""
        from inference_amd.mcmc.utilities import effective_sample_size_batch

        if burn is None:
            burn = self.estimate_burn_in()
        ess = effective_sample_size_batch(self.get_sample(burn=burn), device=device)
        probs = array(self.probs)
        floor = probs[self.chain_length // 2:].min()
        return {
            "burn": burn,
            "ess": ess,
            "ess_mean": int(np.mean(ess)),
            "ess_min": int(ess.min()),
            "step_axis": np.arange(probs.size) * 1e-3,
            "probs": probs,
            "prob_ylims": [floor, probs.max() * 1.1 - 0.1 * floor],
            "epsilon_steps": array(self.ES.epsilon_checks) * 1e-3,
            "epsilon_values": array(self.ES.epsilon_values),
        }

    def plot_diagnostics(self, show=True, filename=None, burn=None, *, device=None):
        """Plot diagnostic traces that show how the chain is progressing: the log-probability against the step number
        with the burn-in marked, the history of the leapfrog step size against the number of attempted trajectories,
        the effective sample size of every parameter after the burn-in (a histogram of them from 50 parameters on), and
        a summary of the three.  Returns the figure (the reference returns None)."""
        data = self.diagnostics_data(burn=burn, device=device)

        import matplotlib.pyplot as plt

        fig = plt.figure(figsize=(12, 9))
        burn_mark = data["burn"] * 1e-3

        ax1 = fig.add_subplot(221)
        ax1.plot(data["step_axis"], data["probs"], marker=".", ls="none", markersize=3)
        ax1.plot([burn_mark, burn_mark], data["prob_ylims"], c="red", ls="dashed", lw=2)
        ax1.set_xlabel("chain step number ($10^3$)", fontsize=12)
        ax1.set_ylabel("posterior log-probability", fontsize=12)
        ax1.set_title("Chain log-probability history")
        ax1.set_ylim(data["prob_ylims"])
        ax1.grid()

        ax2 = fig.add_subplot(222)
        ax2.plot(data["epsilon_steps"], data["epsilon_values"], ".-")
        ax2.set_xlabel("chain step number ($10^3$)", fontsize=12)
        ax2.set_ylabel("Leapfrog step-size", fontsize=12)
        ax2.set_title("Simulation time-step adjustment summary")
        ax2.set_yscale("log")
        ax2.grid()

        ax3 = fig.add_subplot(223)
        if self.n_parameters < 50:
            ax3.bar(range(self.n_parameters), data["ess"], color=["C0", "C1", "C2", "C3", "C4"])
            ax3.set_xlabel("parameter", fontsize=12)
            ax3.set_ylabel("effective sample size", fontsize=12)
            ax3.set_title("Parameter effective sample size estimate")
            ax3.set_xticks(range(self.n_parameters))
        else:
            ax3.hist(data["ess"], bins=20)
            ax3.set_xlabel("effective sample size", fontsize=12)
            ax3.set_ylabel("frequency", fontsize=12)
            ax3.set_title("Parameter effective sample size estimates")

        ax4 = fig.add_subplot(224)
        rows = (("Estimated burn-in:", data["burn"]), ("Average ESS:", data["ess_mean"]), ("Lowest ESS:", data["ess_min"]))
        for k, (name, value) in enumerate(rows):
            height = 0.85 - 0.1 * k
            ax4.text(0.5, height, name, horizontalalignment="right", fontsize=14)
            ax4.text(0.55, height, "{:.5G}".format(value), horizontalalignment="left", fontsize=14)
        ax4.axis("off")

        fig.tight_layout()
        if filename is not None:
            fig.savefig(filename)
        if show:
            plt.show()
        return fig


def _clock(seconds) -> str:
    mins, secs = divmod(int(seconds), 60)
    hrs, mins = divmod(mins, 60)
    return f"{hrs}:{mins:02d}:{secs:02d}"


def advance_lockstep_hmc(chains, n: int, batch_value_and_grad, max_batch: int = None) -> int:
    """Advance every `HamiltonianChain` of `chains` by `n` steps with batched evaluations.

    `batch_value_and_grad(thetas (B, P)) -> (values (B,), grads (B, P))` is the UN-tempered log-probability and its
    gradient (`GpRegressor.marginal_likelihood_gradient_batch` has this signature; for it, batch-independent values are
    switched on).  Every round, each chain that still has work contributes ONE row: the position of its current leapfrog
    stage.  Chains have their own step size, their own number of leapfrog steps and their own retries, so they drift
    apart inside a call and only meet again at its end.  `max_batch` splits a round into calls of at most that many
    rows.

    Per chain the arithmetic and the generator draws are those of `take_step`, operation for operation; the positions and
    momenta of all chains are kept in (chains, P) arrays and the element-wise updates of scalar and vector masses and of
    the reflections are done for all rows at once (element-wise IEEE operations give the same bits row by row; a
    `MatrixMass` keeps its own `inv_mass @ r`).  Two facts make a round cheaper than `take_step`'s sequence of calls:
    the last position of a trajectory needs the gradient (final half kick) AND the value (accept test), and one row
    delivers both; and the gradient at the start of an attempt is the one the chain received at the end of its last
    accepted trajectory, or used in its previous, rejected, attempt.  The chain keeps the (position, value, gradient) it
    holds for `theta[-1]` and a row for the start is asked for only when there is none for exactly that array: on the
    first call after construction and after `replace_last`.

    Identity: if `batch_value_and_grad` agrees row for row, bit for bit, with each chain's own `posterior` and `grad`,
    every chain's trajectory - `theta`, `probs`, `leapfrog_steps`, `ES.epsilon_values`, `ES.epsilon_checks` - is the one
    `take_step` gives it alone.  (On the device that asks for one-by-one functions that go through a batch of one with
    `batch_independent_values(True)`: `marginal_likelihood_gradient` alone takes the single-evaluation kernels.)

    Returns the number of rows evaluated: the sum of the `leapfrog_steps` added by the call, plus one for every chain
    that held nothing for its `theta[-1]`.  Chains without an analytic gradient are refused (TypeError)."""
    chains = list(chains)
    if not chains or n <= 0:
        return 0
    for ch in chains:
        if getattr(ch.grad, "__func__", None) is HamiltonianChain.finite_diff:
            raise TypeError(msg.lockstep_needs_gradient())
    owner = getattr(batch_value_and_grad, "__self__", None)
    if (getattr(batch_value_and_grad, "__name__", "") == "marginal_likelihood_gradient_batch"
            and hasattr(owner, "batch_independent_values")):
        owner.batch_independent_values(True)  # ragged rounds: a row must not depend on its batch

    C, P = len(chains), chains[0].n_parameters
    T, R, G = np.empty((C, P)), np.empty((C, P)), np.zeros((C, P))  # position, momentum, gradient in hand
    V = np.zeros(C)                       # value that came with G
    have = np.zeros(C, dtype=bool)        # G[c] is the gradient at T[c]
    stage = np.zeros(C, dtype=np.int64)   # gradients applied in this attempt
    last = np.ones(C, dtype=np.int64)     # the stage whose gradient is the final half kick
    eps, kick = np.empty(C), np.empty(C)  # epsilon and inv_temp * epsilon of the attempt
    inv_mass = np.ones((C, P))
    dense = [c for c, ch in enumerate(chains) if isinstance(ch.mass, MatrixMass)]
    is_dense = np.zeros(C, dtype=bool)
    is_dense[dense] = True
    for c, ch in enumerate(chains):
        if not is_dense[c]:
            inv_mass[c] = ch.mass.inv_mass
    bounded = np.array([ch.bounds is not None for ch in chains])
    lower, width = np.zeros((C, P)), np.ones((C, P))
    for c, ch in enumerate(chains):
        if bounded[c]:
            lower[c], width[c] = ch.bounds.lower, ch.bounds.width
    done, attempts, taken = [0] * C, [0] * C, [0] * C
    n_steps, H0 = [0] * C, [0.0] * C

    def begin(c):
        """Chain c starts an attempt; it has the gradient at its start in hand unless `theta[-1]` was replaced."""
        ch = chains[c]
        if attempts[c] >= ch.max_attempts:
            raise ValueError(msg.hmc_attempts(ch.max_attempts))
        attempts[c] += 1
        r0, n_steps[c], H0[c] = ch._draw_attempt()
        t0 = ch.theta[-1]
        T[c], R[c] = t0, r0
        stage[c], last[c] = 0, max(n_steps[c], 1)  # (a trajectory of no steps still makes one: hmc/__init__.py:168-175)
        eps[c], kick[c] = ch.ES.epsilon, ch.inv_temp * ch.ES.epsilon
        held = ch._held
        have[c] = held is not None and held[0] is t0 and np.array_equal(held[1], t0)
        if have[c]:
            G[c] = held[3]

    active = np.arange(C)
    for c in active:
        begin(c)
    evals = 0
    while active.size:
        ask = active[~have[active]]
        if ask.size:
            size = max_batch or ask.size
            for lo in range(0, ask.size, size):
                rows = ask[lo:lo + size]
                V[rows], G[rows] = batch_value_and_grad(T[rows])
            evals += ask.size
            have[ask] = True
            for c in ask[stage[ask] == 0]:
                chains[c]._held = (chains[c].theta[-1], T[c].copy(), V[c], G[c].copy())

        # trajectories at their last position: final half kick, accept test, and the next attempt or step
        ending = active[stage[active] == last[active]]
        if ending.size:
            R[ending] += (0.5 * kick[ending])[:, None] * G[ending]
            finished = []
            for c in ending:
                ch = chains[c]
                t, r = T[c].copy(), R[c].copy()
                p = V[c] * ch.inv_temp
                taken[c] += n_steps[c]
                if ch._accept(H0[c], r, p):
                    ch._commit(t, p, taken[c])
                    ch._held = (t, t.copy(), V[c], G[c].copy())
                    done[c] += 1
                    attempts[c] = taken[c] = 0
                if done[c] < n:
                    begin(c)
                else:
                    finished.append(c)
            if finished:
                active = active[~np.isin(active, finished)]

        # every chain with a gradient in hand: kick (half at the start), move, reflect
        go = active[have[active]]
        if go.size:
            R[go] += np.where(stage[go] == 0, 0.5 * kick[go], kick[go])[:, None] * G[go]
            velocity = R[go] * inv_mass[go]
            for k in np.flatnonzero(is_dense[go]):
                velocity[k] = chains[go[k]].mass.get_velocity(R[go[k]].copy())
            T[go] += eps[go][:, None] * velocity
            hit = go[bounded[go]]
            if hit.size:
                bounces, inside = np.divmod(T[hit] - lower[hit], width[hit])
                odd = bounces % 2
                sign = 1 - 2 * odd
                T[hit] = lower[hit] + sign * inside + odd * width[hit]
                R[hit] *= sign
            stage[go] += 1
            have[go] = False
    return evals
