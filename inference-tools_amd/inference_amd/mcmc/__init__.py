from inference_amd.mcmc.gibbs import GibbsChain, advance_lockstep
from inference_amd.mcmc.parallel import ParallelTempering, advance_ladders
from inference_amd.mcmc.utilities import effective_sample_size, effective_sample_size_batch

__all__ = ["GibbsChain", "ParallelTempering", "advance_lockstep", "advance_ladders", "effective_sample_size",
           "effective_sample_size_batch"]
