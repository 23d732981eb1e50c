from inference_amd.mcmc.ensemble import EnsembleSampler, advance_lockstep_ensembles
from inference_amd.mcmc.gibbs import GibbsChain, advance_lockstep
from inference_amd.mcmc.hmc import HamiltonianChain, advance_lockstep_hmc
from inference_amd.mcmc.parallel import ParallelTempering, advance_ladders
from inference_amd.mcmc.pca import PcaChain
from inference_amd.mcmc.utilities import Bounds, effective_sample_size, effective_sample_size_batch, sample_covariance

__all__ = ["GibbsChain", "HamiltonianChain", "PcaChain", "EnsembleSampler", "ParallelTempering", "Bounds", "advance_lockstep",
           "advance_lockstep_hmc", "advance_lockstep_ensembles", "advance_ladders", "effective_sample_size",
           "effective_sample_size_batch", "sample_covariance"]
