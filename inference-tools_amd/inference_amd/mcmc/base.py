"""What the chains share (reference: mcmc/base.py): the check of the posterior at construction and the read-out of
results over `get_parameter`, `get_probabilities` and `get_sample`, which every chain class provides itself."""
from numpy import isfinite
from numpy.random import permutation


class MarkovChain:
    chain_length: int
    n_parameters: int

    def _validate_posterior(self, posterior, start):
        """base.py:266-296."""
        name = self.__class__.__name__
        if not callable(posterior):
            raise ValueError(f"\n[ {name} error ]\n>> The given 'posterior' is not a callable object.")
        prob = posterior(start)
        if not isinstance(prob, float):
            raise ValueError(
                f"\n[ {name} error ]\n>> The given 'posterior' must return a float or a type which derives "
                f"from float, however the returned value has type:\n>> {type(prob)}"
            )
        if not isfinite(prob):
            raise ValueError(
                f"\n[ {name} error ]\n>> The given 'posterior' must return a finite value for the given "
                f"'start' parameter values, but instead returns a value of:\n>> {prob}"
            )

    # -- results (reference: base.py:75-216) ---------------------------------------------
    def get_marginal(self, index: int, burn: int = 1, thin: int = 1, unimodal=False):
        """Estimate of the 1D marginal distribution of parameter `index`: a `GaussianKDE` of
        `get_parameter(index, burn, thin)`.  `unimodal=True` (a `UnimodalPdf` in the reference) is not provided."""
        from inference_amd.pdf import GaussianKDE
        from inference_amd.pdf._messages import marginal_unimodal

        if unimodal:
            raise NotImplementedError(marginal_unimodal(self.__class__.__name__))
        return GaussianKDE(self.get_parameter(index, burn=burn, thin=thin))

    def get_interval(self, interval: float = 0.95, burn: int = 1, thin: int = 1, samples: int = None):
        """The samples in the highest-probability fraction `interval` of the chain, ordered by increasing
        log-probability, and their log-probabilities.  `samples` overrides `thin`.  As in the reference, the trim to
        `samples` draws `numpy.random.permutation` and then indexes with the None that `ndarray.sort()` returns: no
        sample is removed and both arrays gain a leading axis of length 1."""
        probs = self.get_probabilities(burn=burn)
        if samples is not None:
            thin = max(probs.size // samples, 1)

        sample = self.get_sample(burn=burn, thin=thin)
        probs = probs[::thin]

        sorter = probs.argsort()
        sample = sample[sorter, :]
        probs = probs[sorter]
        # trim the lowest-probability samples
        cutoff = int(probs.size * (1 - interval))
        sample = sample[cutoff:, :]
        probs = probs[cutoff:]

        if samples is not None:
            n_trim = probs.size - samples
            if n_trim > 0:
                subsample = permutation(probs.size)[n_trim:].sort()
                sample = sample[subsample, :]
                probs = probs[subsample]

        return sample, probs

    def matrix_plot(self, params=None, burn: int = 0, thin: int = 1, **kwargs):
        """The matrix plot of the parameters (or of those whose indices `params` lists): all 1D and 2D marginal
        distributions of the samples left after `burn` and `thin`.  The other keyword arguments are those of
        `inference_amd.plotting.matrix_plot`, whose figure is returned (the reference returns None)."""
        from inference_amd.plotting import matrix_plot

        self._plot_checks(burn, thin, "matrix")
        params = params if params is not None else range(self.n_parameters)
        samples = [self.get_parameter(i, burn=burn, thin=thin) for i in params]
        return matrix_plot(samples, **kwargs)

    def trace_plot(self, params=None, burn: int = 0, thin: int = 1, **kwargs):
        """The trace plot of the parameters (or of those whose indices `params` lists): the value of each as a function
        of the step number, for the samples left after `burn` and `thin` (base.py:191-216).  The other keyword arguments
        are those of `inference_amd.plotting.trace_plot`, whose figure is returned (the reference returns None)."""
        from inference_amd.plotting import trace_plot

        self._plot_checks(burn, thin, "trace")
        params = params if params is not None else range(self.n_parameters)
        samples = [self.get_parameter(i, burn=burn, thin=thin) for i in params]
        return trace_plot(samples, **kwargs)

    def _plot_checks(self, burn: int, thin: int, plot_type: str):
        """base.py:218-237."""
        from inference_amd.pdf._messages import plot_burn_thin, plot_no_samples

        name = self.__class__.__name__
        if self.chain_length < 2:
            raise ValueError(plot_no_samples(name, plot_type, self.chain_length))
        reduced_length = max(self.chain_length - burn - 1, 0) // thin + 1
        if reduced_length < 2:
            raise ValueError(plot_burn_thin(name, plot_type, reduced_length))
