"""Selection of the leapfrog step size of a `HamiltonianChain` (reference: mcmc/hmc/epsilon.py:5-54)."""
from copy import copy

from numpy import log, sqrt


class EpsilonSelector:
    """Tunes `epsilon` towards an acceptance rate of 65 %.  Every `chk_int` submitted acceptance probabilities the rate is
    reviewed: the number of acceptances is approximately normal (Poisson-binomial), and epsilon changes only when the
    target lies outside two standard deviations of the observed mean rate; otherwise the review interval grows."""

    def __init__(self, epsilon: float):
        self.epsilon = epsilon
        self.epsilon_values = [copy(epsilon)]  # the value after each change
        self.epsilon_checks = [0.0]            # the number of submitted probabilities at each change
        # acceptance statistics since the last change
        self.avg = 0
        self.var = 0
        self.num = 0
        self.accept_rate = 0.65
        self.chk_int = 15
        self.growth_factor = 1.4

    def add_probability(self, p: float):
        self.num += 1
        self.avg += p
        self.var += max(p * (1 - p), 0.03)  # (the floor keeps a run of certain outcomes from looking exact)
        if self.num >= self.chk_int:
            self.update_epsilon()

    def update_epsilon(self):
        rate = self.avg / self.num
        spread = sqrt(self.var) / self.num
        if rate - 2 * spread < self.accept_rate < rate + 2 * spread:
            self.chk_int = int((self.growth_factor * self.chk_int) * 0.1) * 10
            return
        factor = (log(self.accept_rate) / log(rate)) ** 0.15
        self.adjust_epsilon(max(min(factor, 2.0), 0.5))

    def adjust_epsilon(self, ratio: float):
        """Scale the step size, log it and restart the acceptance statistics."""
        self.epsilon *= ratio
        self.epsilon_values.append(copy(self.epsilon))
        self.epsilon_checks.append(self.epsilon_checks[-1] + self.num)
        self.avg = self.var = self.num = 0
