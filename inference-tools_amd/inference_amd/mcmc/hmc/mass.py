"""Particle masses of a `HamiltonianChain` (reference: mcmc/hmc/mass.py): the inverse mass turns a momentum into a
velocity, and momenta are drawn from the normal distribution whose covariance is the mass."""
from numpy import eye, isscalar, ndarray, sqrt
from numpy.linalg import cholesky
from scipy.linalg import issymmetric, solve_triangular

from inference_amd.pdf import _messages as msg


class ScalarMass:
    """One inverse mass for every parameter."""

    def __init__(self, inv_mass, n_parameters: int):
        self.inv_mass = inv_mass
        self.sqrt_mass = 1 / sqrt(self.inv_mass)
        self.n_parameters = n_parameters

    def get_velocity(self, r: ndarray) -> ndarray:
        return r * self.inv_mass

    def sample_momentum(self, rng) -> ndarray:
        return rng.normal(size=self.n_parameters, scale=self.sqrt_mass)


class VectorMass(ScalarMass):
    """An inverse mass per parameter: approximately the variance of its marginal distribution.  (As in the reference, a
    vector of the wrong shape fails the assertions; the ValueError is left for entries that are not positive.)"""

    def __init__(self, inv_mass: ndarray, n_parameters: int):
        super().__init__(inv_mass, n_parameters)
        assert inv_mass.ndim == 1
        assert inv_mass.size == n_parameters
        if not (inv_mass > 0.0).all():
            raise ValueError(msg.vector_mass(n_parameters))


class MatrixMass:
    """A full inverse-mass matrix: approximately the covariance of the posterior."""

    def __init__(self, inv_mass: ndarray, n_parameters: int):
        if inv_mass.ndim != 2 or inv_mass.shape[0] != inv_mass.shape[1] or not issymmetric(inv_mass):
            raise ValueError(msg.matrix_mass_covariance())
        if inv_mass.shape[0] != n_parameters:
            raise ValueError(msg.matrix_mass_size(inv_mass.shape, n_parameters))
        self.inv_mass = inv_mass
        self.n_parameters = n_parameters
        # with inv_mass = C C^T the mass is C^-T C^-1: momenta are C^-T z for standard normal z
        self.L = solve_triangular(cholesky(inv_mass), eye(n_parameters), lower=True).T

    def get_velocity(self, r: ndarray) -> ndarray:
        return self.inv_mass @ r

    def sample_momentum(self, rng) -> ndarray:
        return self.L @ rng.normal(size=self.n_parameters)


def get_particle_mass(inverse_mass, n_parameters: int):
    """The mass class for a scalar, a vector or a matrix `inverse_mass`."""
    if isscalar(inverse_mass):
        return ScalarMass(inverse_mass, n_parameters)
    if not isinstance(inverse_mass, ndarray):
        raise TypeError(msg.inverse_mass_type(type(inverse_mass)))
    if inverse_mass.ndim == 1:
        return VectorMass(inverse_mass, n_parameters)
    return MatrixMass(inverse_mass, n_parameters)
