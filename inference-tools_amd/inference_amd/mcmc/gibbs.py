"""
Gibbs-sampling Markov chain — the caller of the GP log-marginal-likelihood in
BASELINE config 5.  Mirrors the step semantics of the reference's `GibbsChain`
(inference/mcmc/gibbs.py:593-656) and of its per-parameter proposal / width
adaptation (`Parameter`, gibbs.py:16-160): every step is a sequence of 1-D
Metropolis-Hastings updates, one per parameter, each retried until accepted,
with proposal widths tuned towards a 50 % acceptance rate.

Provided: what `ParallelTempering` needs (`inv_temp`, `take_step`, `get_last`,
`replace_last`, `probs`, sample access, boundaries) and the reference's read-out
of results (base.py:75-160, gibbs.py:370-377; shared with `HamiltonianChain` through `MarkovChain`): `get_marginal` (a device
`GaussianKDE` of one parameter), `get_interval`, `mode`, `matrix_plot` and
`trace_plot` (base.py:162-216, over `inference_amd.plotting`), and the check that
comes before them (gibbs.py:405-519, :577-592): `estimate_burn_in`, `diagnostics_data`
(with the effective sample size of every parameter from one device call) and
`plot_diagnostics`.  `UnimodalPdf` marginals and save / load of the reference are out of scope.

MI355X-specific addition: `advance_lockstep` advances MANY chains together so
that each round of proposals is ONE batched posterior evaluation on the device
(`GpRegressor.marginal_likelihood_batch`).  Chains keep their own random
generators (one per chain, one per parameter, as in the reference), so lockstep
and one-by-one execution produce identical trajectories.
"""
from copy import copy

import numpy as np
from numpy import argmax, array, exp, float64, log, sqrt
from numpy.random import default_rng

from inference_amd.mcmc.base import MarkovChain


class Parameter:
    """Proposal state of one model parameter (reference: gibbs.py:16-160)."""

    def __init__(self, value: float, sigma: float):
        self.samples = [value]
        self.sigma = sigma
        self.rng = default_rng()
        # acceptance statistics since the last width assessment
        self.avg = 0
        self.var = 0
        self.num = 0
        self.sigma_values = [copy(self.sigma)]
        self.sigma_checks = [0.0]
        self.try_count = 0
        # adaptation settings (gibbs.py:41-46)
        self.target_rate = 0.25
        self.max_tries = 50
        self.chk_int = 100
        self.growth_factor = 1.75
        self.adjust_rate = 0.25
        self.non_negative = False
        self.bounded = False
        self.lower = 0.0
        self.upper = 0.0
        self.width = 0.0

    def set_boundaries(self, lower, upper):
        if not lower < upper:
            raise ValueError("Upper limit must be greater than lower limit")
        self.lower, self.upper, self.width = lower, upper, upper - lower
        self.bounded = True

    def remove_boundaries(self):
        self.bounded = False
        self.lower = self.upper = self.width = 0.0

    def _fold_into_bounds(self, value):
        """Reflect `value` back into [lower, upper] as many times as needed (a triangle wave of period 2 width)."""
        offset = value - self.lower
        inside = offset % self.width
        bounces = offset // self.width
        return self.lower + inside if bounces % 2 == 0 else self.upper - inside

    def proposal(self):
        """Draw the next 1-D proposal (behaviour of gibbs.py:88-122): a normal step from the last sample; a
        parameter that has already failed `max_tries` times in this update has its width quartered first;
        bounded parameters are reflected inside, non-negative ones mirrored at zero."""
        self.try_count += 1
        if self.try_count > self.max_tries:
            self.adjust_sigma(0.25)
        step = self.rng.normal(loc=self.samples[-1], scale=self.sigma)
        if self.bounded:
            return self._fold_into_bounds(step)
        return abs(step) if self.non_negative else step

    def submit_accept_prob(self, p: float):
        """Record the acceptance probability of one proposal; every `chk_int` records the width is reviewed."""
        self.num += 1
        self.avg += p
        self.var += p * (1 - p)
        if self.num >= self.chk_int:
            self.update_epsilon()

    def update_epsilon(self):
        """Width review (behaviour of gibbs.py:132-148).  The number of acceptances is approximately normal
        (Poisson-binomial); the width changes only when the target rate lies outside two standard deviations
        of the observed mean rate, otherwise the review interval grows."""
        rate = self.avg / self.num
        spread = sqrt(self.var) / self.num
        if rate - 2 * spread < self.target_rate < rate + 2 * spread:
            self.chk_int = int((self.growth_factor * self.chk_int) * 0.1) * 10
            return
        factor = (log(self.target_rate) / log(rate)) ** self.adjust_rate
        self.adjust_sigma(min(max(factor, 0.1), 3.0))

    def adjust_sigma(self, ratio: float):
        """Scale the proposal width, log it and restart the acceptance statistics."""
        self.sigma *= ratio
        self.sigma_values.append(copy(self.sigma))
        self.sigma_checks.append(len(self.samples))
        self.avg = self.var = self.num = 0

    def add_sample(self, s):
        self.samples.append(s)
        self.try_count = 0


class GibbsChain(MarkovChain):
    """
    :param posterior: callable `theta (ndarray) -> float` log-probability
        (e.g. `GpRegressor.marginal_likelihood`).
    :param start: starting parameter vector.
    :param widths: initial proposal widths (default 5 % of `start`, 1.0 where it is zero).
    :param temperature: chain temperature T; the chain samples posterior ** (1 / T).
    """

    def __init__(self, posterior, start, widths=None, temperature: float = 1.0, display_progress: bool = True):
        self.inv_temp = 1.0 / temperature
        self.rng = default_rng()
        self.posterior = posterior
        self._validate_posterior(posterior, start)
        if widths is None:
            widths = [v * 0.05 if v != 0 else 1.0 for v in start]
        self.params = [Parameter(value=v, sigma=s) for v, s in zip(start, widths)]
        for p in self.params:
            p.target_rate = 0.5  # optimal for 1-D updates (gibbs.py:621-625)
        self.chain_length = 1
        self.n_parameters = len(start)
        self.probs = [self.posterior(self.get_last()) * self.inv_temp]
        self.display_progress = display_progress

    # -- stepping ----------------------------------------------------------------------
    def take_step(self):
        """One Gibbs step: a retried-until-accepted 1-D MH update per parameter (gibbs.py:627-656)."""
        p_old = self.probs[-1]
        prop = self.get_last()
        p_new = p_old
        for i, par in enumerate(self.params):
            while True:
                prop = self._propose(prop, i)
                p_new = self.posterior(prop) * self.inv_temp
                if self._mh_test(par, p_new, p_old):
                    break
            p_old = p_new
        self._commit(prop, p_new)

    def _propose(self, prop, par: int):
        """The next proposal of the step in progress, for the update of parameter `par`: `prop`, the point the step has
        reached, with a new value of that parameter.  The seam through which the lockstep drivers ask a chain for its
        proposals (`PcaChain` proposes a whole vector along a direction instead)."""
        prop[par] = self.params[par].proposal()
        return prop

    def _mh_test(self, par, p_new, p_old) -> bool:
        if p_new > p_old:
            par.submit_accept_prob(1.0)
            return True
        acceptance_prob = exp(p_new - p_old)
        par.submit_accept_prob(acceptance_prob)
        return bool(self.rng.random() < acceptance_prob)

    def _commit(self, prop, p_new):
        for v, par in zip(prop, self.params):
            par.add_sample(v)
        self.probs.append(p_new)
        self.chain_length += 1

    def advance(self, m: int):
        for _ in range(m):
            self.take_step()

    # -- state access -------------------------------------------------------------------
    def get_last(self):
        return array([p.samples[-1] for p in self.params], dtype=float64)

    def replace_last(self, theta):
        for p, t in zip(self.params, theta):
            p.samples[-1] = t

    def get_parameter(self, index: int, burn: int = 1, thin: int = 1):
        return array(self.params[index].samples[burn::thin])

    def get_probabilities(self, burn: int = 1, thin: int = 1):
        return array(self.probs[burn::thin])

    def get_sample(self, burn: int = 1, thin: int = 1):
        return array([self.get_parameter(i, burn=burn, thin=thin) for i in range(self.n_parameters)]).T

    # -- results: `get_marginal`, `get_interval`, `matrix_plot` and `trace_plot` come from `MarkovChain` ------------------
    def mode(self):
        """The sample with the highest log-probability so far."""
        ind = argmax(self.probs)
        return array([p.samples[ind] for p in self.params])

    # -- diagnostics (reference: gibbs.py:405-519, :577-592) -----------------------------------
    def estimate_burn_in(self) -> int:
        """An estimate of the burn-in: the later of the step at which the chain first enters the top 1 % of its
        log-probabilities and the mean, over the parameters, of the last step at which the proposal width was reviewed
        and found more than 15 % away from its final value.  (As in the reference, a parameter whose width never was
        that far away contributes its LAST review, the 0 that argmax gives for no match on the reversed log.)"""
        probs = array(self.probs)
        prob_estimate = argmax(probs > np.percentile(probs, 99))
        width_estimates = []
        for p in self.params:
            latest_first = array(p.sigma_values)[::-1]
            checks = array(p.sigma_checks)[::-1]
            far = abs(latest_first / p.sigma - 1.0) > 0.15
            width_estimates.append(checks[argmax(far)])
        return int(max(prob_estimate, np.mean(width_estimates)))

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
        widths = [array(p.sigma_values) for p in self.params]
        return {
            "burn": burn,
            "ess": ess,
            "ess_mean": int(np.mean(ess)),
            "ess_min": int(ess.min()),
            "step_axis": np.arange(probs.size) * 1e-3,
            "probs": probs,
            "prob_ylims": [floor, probs.max() * 1.1 - 0.1 * floor],
            "width_steps": [array(p.sigma_checks[1:]) * 1e-3 for p in self.params],
            "width_percent_change": [1e2 * np.diff(w) / w[:-1] for w in widths],
        }

    def plot_diagnostics(self, show=True, filename=None, *, device=None):
        """Plot diagnostic traces that show how the chain is progressing: the log-probability against the step number
        with the estimated burn-in marked, the history of the changes to every parameter's proposal width (which
        should die away), the effective sample size of every parameter after the burn-in, and a summary of the
        three.  Returns the figure (the reference returns None)."""
        data = self.diagnostics_data(device=device)

        import matplotlib.pyplot as plt

        fig = plt.figure(figsize=(12, 9))
        burn_mark = data["burn"] * 1e-3
        length_mark = self.chain_length * 1e-3

        ax1 = fig.add_subplot(221)
        ax1.plot(data["step_axis"], data["probs"], marker=".", ls="none", markersize=3)
        ax1.plot([burn_mark, burn_mark], data["prob_ylims"], c="red", ls="dashed", lw=2)
        ax1.set_xlabel("chain step number ($10^3$)", fontsize=12)
        ax1.set_ylabel("posterior log-probability", fontsize=12)
        ax1.set_title("Chain log-probability history")
        ax1.set_ylim(data["prob_ylims"])
        ax1.grid()

        ax2 = fig.add_subplot(222)
        for steps, change in zip(data["width_steps"], data["width_percent_change"]):
            ax2.plot(steps, change, marker="D", markersize=3)
        for level in (5, -5):
            ax2.plot([0, length_mark], [level, level], ls="dashed", lw=2, color="black")
        ax2.set_xlabel("chain step number ($10^3$)", fontsize=12)
        ax2.set_ylabel("% change in proposal widths", fontsize=12)
        ax2.set_title("Parameter proposal widths adjustment summary")
        ax2.set_ylim([-50, 50])
        ax2.grid()

        ax3 = fig.add_subplot(223)
        ax3.bar(range(self.n_parameters), data["ess"], color=["C0", "C1", "C2", "C3", "C4"])
        ax3.set_xlabel("parameter", fontsize=12)
        ax3.set_ylabel("effective sample size", fontsize=12)
        ax3.set_title("Parameter effective sample size estimate")
        ax3.set_xticks(range(self.n_parameters))

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

    def set_non_negative(self, parameter: int, flag=True):
        self.params[parameter].non_negative = flag

    def set_boundaries(self, parameter: int, boundaries, remove=False):
        if remove:
            self.params[parameter].remove_boundaries()
        else:
            self.params[parameter].set_boundaries(*boundaries)


def advance_lockstep(chains, n: int, batch_posterior):
    """Advance every chain by `n` Gibbs steps with batched posterior evaluations.

    `batch_posterior(thetas (B, P)) -> (B,)` must agree element-wise with each chain's own
    `posterior`.  Every round, every chain that still has work proposes a value for ITS current
    parameter (`chain._propose`: `GibbsChain`s and `PcaChain`s may be mixed) and all proposals are evaluated in one call; a chain whose proposal is accepted moves
    on to its next parameter (and its next step) at once, one whose proposal is rejected retries
    (the retry-until-accept loop of gibbs.py:635-648).  Chains therefore drift apart inside a call
    and only meet again at its end - a chain draws from its own generators only and never sees the
    others, so its trajectory is the one it would follow alone - and the batches stay full until the
    first chains finish, instead of shrinking 64 -> 1 for every parameter.
    Returns the number of posterior evaluations made."""
    if not chains or n <= 0:
        return 0
    P = chains[0].n_parameters
    evals = 0
    step = [0] * len(chains)  # completed steps
    par = [0] * len(chains)   # parameter being updated
    p_old = [c.probs[-1] for c in chains]
    p_acc = list(p_old)
    prop = [c.get_last() for c in chains]
    active = list(range(len(chains)))
    while active:
        for c in active:
            prop[c] = chains[c]._propose(prop[c], par[c])
        vals = batch_posterior(array([prop[c] for c in active]))
        evals += len(active)
        still = []
        for c, v in zip(active, vals):
            chain = chains[c]
            p_new = float(v) * chain.inv_temp
            if chain._mh_test(chain.params[par[c]], p_new, p_old[c]):
                p_old[c] = p_new
                p_acc[c] = p_new
                par[c] += 1
                if par[c] == P:
                    chain._commit(prop[c], p_acc[c])
                    step[c] += 1
                    par[c] = 0
                    if step[c] < n:
                        p_old[c] = chain.probs[-1]
                        p_acc[c] = p_old[c]
                        prop[c] = chain.get_last()
            if step[c] < n:
                still.append(c)
        active = still
    return evals
