"""Base class of the 1D density estimators (reference: pdf/base.py:8-169): the search for the highest-density interval
and `plot_summary`, which `GaussianKDE` and `UnimodalPdf` share.  matplotlib is imported inside `plot_summary` only, so
the package imports without it."""
from abc import ABC, abstractmethod

from numpy import array, linspace, ndarray, sqrt
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

    def plot_summary(self, filename=None, show=True, label=None):
        """
        Plot the estimated PDF beside a table of summary statistics: the mode, the mean and the standard deviation, the
        1-sigma and 2-sigma highest-density intervals, and the variance, skewness and excess kurtosis.

        :keyword str filename: File to which the plot is saved. If unspecified, the plot is not saved.
        :keyword bool show: Whether the plot is displayed in a window (default True).
        :keyword str label: Label of the x-axis.
        :return: The figure and its two axes, ``(fig, ax)``.
        """
        import matplotlib.pyplot as plt

        intervals = [("1-sigma:", self.interval(fraction=0.68268)), ("2-sigma:", self.interval(fraction=0.95449))]
        mu, var, skw, kur = self.moments()
        peak = self(self.mode)

        # the axis: the 2-sigma interval plus a tenth of its width either side, extended until the pdf is below 0.5 % of its peak
        lwr, upr = intervals[1][1]
        step = 0.1 * (upr - lwr)
        lwr, upr = lwr - step, upr + step
        while self(lwr) / peak > 5e-3:
            lwr -= step
        while self(upr) / peak > 5e-3:
            upr += step
        axis = linspace(lwr, upr, 500)
        pdf = self(axis)

        fig, ax = plt.subplots(nrows=1, ncols=2, figsize=(10, 6), gridspec_kw={"width_ratios": [2, 1]})
        curve, table = ax
        curve.plot(axis, pdf, lw=1, c="C0")
        curve.fill_between(axis, pdf, color="C0", alpha=0.1)
        curve.plot([self.mode, self.mode], [0.0, peak], c="red", ls="dashed")
        curve.set_xlabel(label or "argument", fontsize=13)
        curve.set_ylabel("probability density", fontsize=13)
        curve.set_ylim([0.0, None])
        curve.grid()

        # the table: (name, text) rows, a bold title for a row without text, None for an empty line
        rows = [("Basics", None), ("Mode:", f"{self.mode:.5G}"), ("Mean:", f"{mu:.5G}"),
                ("Standard dev:", f"{sqrt(var):.5G}"), None, ("Highest-density intervals", None)]
        rows += [(name, rf"{iv[0]:.5G} $\rightarrow$ {iv[1]:.5G}") for name, iv in intervals]
        rows += [None, ("Higher moments", None), ("Variance:", f"{var:.5G}"), ("Skewness:", f"{skw:.5G}"),
                 ("Kurtosis:", f"{kur:.5G}")]
        for line, entry in enumerate(rows):
            height = 0.95 - 0.05 * line
            if entry is None:
                continue
            name, text = entry
            if text is None:
                table.text(0.0, height, name, horizontalalignment="left", fontweight="bold")
            else:
                table.text(0.35, height, name, horizontalalignment="right")
                table.text(0.40, height, text, horizontalalignment="left")
        table.axis("off")

        plt.tight_layout()
        if filename is not None:
            plt.savefig(filename)
        if show:
            plt.show()
        return fig, ax
