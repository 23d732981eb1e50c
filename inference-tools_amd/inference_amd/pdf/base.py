"""Base class of the 1D density estimators (reference: pdf/base.py:8-72).  The reference's `plot_summary` is not
provided, and nothing here imports matplotlib."""
from abc import ABC, abstractmethod

from numpy import array, ndarray
from scipy.optimize import minimize

from inference_amd.pdf import _messages as msg
from inference_amd.pdf.hdi import sample_hdi


class DensityEstimator(ABC):
    """
    Abstract base class for 1D density estimators.
    """

    sample: ndarray
    mode: float

    @abstractmethod
    def __call__(self, x: ndarray) -> ndarray:
        pass

    @abstractmethod
    def cdf(self, x: ndarray) -> ndarray:
        pass

    @abstractmethod
    def moments(self) -> tuple:
        pass

    def _pdf_and_cdf(self, x: ndarray):
        """pdf and cdf at the same points; an estimator that can produce both at once overrides this."""
        return self(x), self.cdf(x)

    def interval(self, fraction: float) -> tuple[float, float]:
        """
        Calculates the 'highest-density interval', the shortest single interval which contains a chosen fraction of the
        total probability.

        :param fraction: Fraction of the total probability contained by the interval, between 0 and 1.
        :return: A tuple of the lower and upper limits of the interval, ``(lower_limit, upper_limit)``.
        """
        if not 0.0 < fraction < 1.0:
            raise ValueError(msg.interval_bad_fraction(self.__class__.__name__, fraction))
        # use the sample to estimate the HDI, then switch to the centre and width of the interval
        lwr, upr = sample_hdi(self.sample, fraction=fraction)
        c = 0.5 * (lwr + upr)
        w = upr - lwr

        simplex = array([[c, w], [c, 0.95 * w], [c - 0.05 * w, w]])
        weight = 0.2 / self(self.mode)
        result = minimize(
            fun=self._hdi_cost,
            x0=simplex[0, :],
            method="Nelder-Mead",
            options={"initial_simplex": simplex},
            args=(fraction, weight),
        )
        c, w = result.x
        return c - 0.5 * w, c + 0.5 * w

    def _hdi_cost(self, theta, fraction, prob_weight):
        c, w = theta
        v = array([c - 0.5 * w, c + 0.5 * w])
        (Pa, Pb), (Fa, Fb) = self._pdf_and_cdf(v)
        return (prob_weight * (Pa - Pb)) ** 2 + (Fb - Fa - fraction) ** 2
