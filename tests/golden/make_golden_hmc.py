"""
Golden vectors of the reference's HamiltonianChain (mcmc/hmc/__init__.py), its masses (mcmc/hmc/mass.py) and Bounds
(mcmc/utilities.py:98-162), written to hmc.npz beside this file by IMPORTING the reference the way make_golden.py does.
Data only (allow_pickle=False).

Run in the build container only:   python tests/golden/make_golden_hmc.py

The chains are the seeded recipes of tests/hmc_host.py (`build`), run with warnings turned into errors.

Cases
  scalar, vector, matrix, fdiff   the four traces of hmc_host.CASES: `<case>_theta`, `_probs`, `_leapfrog_steps`,
              `_epsilon_values`, `_epsilon_checks`, `_burn` (estimate_burn_in) and `_mode`
  long        the scalar recipe run for 2000 steps: the same arrays, estimate_mass (diagonal and full), the three getters
              and get_interval at a burn and thin, and the ESS of plot_diagnostics at an odd burn (so that the length
              left is even, where the device batch is the reference's number)
  bounds_*    reflect and reflect_momenta at seeded points up to five widths outside the bounds
  momentum_*  seeded sample_momentum draws of the three masses

Every trace is ASSERTED to keep its distance from the places where a rounding error could change a decision: every accept
test that drew a uniform has |u - accept_prob| >= 1e-6, every steps * (1 + (u - 0.5) * 0.2) is at least 1e-9 from an
integer, and at every epsilon review the target rate is at least 1e-6 (relative) from the 2-sigma edges.  The ESS columns
keep the margins of make_golden_ess.py (ess_host.MARGIN).
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.mcmc import HamiltonianChain  # noqa: E402
from inference.mcmc.hmc.mass import get_particle_mass  # noqa: E402
from inference.mcmc.utilities import Bounds, effective_sample_size  # noqa: E402

import ess_host as eh  # noqa: E402
import hmc_host as hh  # noqa: E402
from make_golden_ess import reference_numbers  # noqa: E402

OUT = {}


def trace(name, recipe, steps):
    chain = hh.build(HamiltonianChain, recipe)
    rec = hh.Recorder(chain)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(steps):
            chain.take_step()
    for key, value in hh.state(chain).items():
        OUT[f"{name}_{key}"] = value
    assert np.isfinite(OUT[f"{name}_theta"]).all() and np.isfinite(OUT[f"{name}_probs"]).all(), name
    OUT[f"{name}_burn"] = np.array(chain.estimate_burn_in())
    OUT[f"{name}_mode"] = chain.mode()
    accept, n_steps, review, retries = rec.margins()
    assert accept >= 1e-6 and n_steps >= 1e-9 and review >= 1e-6, (name, accept, n_steps, review)
    print(f"{name:7s} length {chain.chain_length}, {retries} retried attempts, {len(rec.reviews)} epsilon reviews "
          f"({len(chain.ES.epsilon_values) - 1} changes), margins {accept:.1e} {n_steps:.1e} {review:.1e}, "
          f"burn {int(OUT[f'{name}_burn'])}")
    return chain


def long_case():
    chain = trace("long", "scalar", hh.LONG)
    burn = int(chain.estimate_burn_in()) | 1  # odd: the length left is even
    assert (chain.chain_length - burn) % 2 == 0
    OUT["long_diag_burn"] = np.array(burn)
    OUT["long_diag_ess"] = np.array([effective_sample_size(np.array(chain.get_parameter(i, burn=burn, thin=1)))
                                     for i in range(3)], dtype=np.int64)
    lag_margin, int_margin = np.inf, np.inf
    for column in chain.get_sample(burn=burn).T:
        f0, total, cut, f = reference_numbers(column)
        assert cut >= 1
        lag_margin = min(lag_margin, np.abs(f[: cut + 1]).min() / f0)
        if cut > 1:
            q = column.size / (total / f0)
            int_margin = min(int_margin, abs(q - round(q)) / q)
    assert lag_margin >= eh.MARGIN and int_margin >= eh.MARGIN, (lag_margin, int_margin)
    print(f"long: diagnostics burn {burn}, ess {OUT['long_diag_ess'].tolist()}, margins {lag_margin:.1e} {int_margin:.1e}")

    OUT["long_parameter"] = chain.get_parameter(1, burn=10, thin=3)
    OUT["long_probabilities"] = chain.get_probabilities(burn=10, thin=3)
    OUT["long_sample"] = chain.get_sample(burn=10, thin=3)
    OUT["long_interval_sample"], OUT["long_interval_probs"] = chain.get_interval(interval=0.9, burn=200, thin=2)
    chain.estimate_mass(burn=200, thin=2, diagonal=True)
    OUT["long_mass_diagonal"] = np.array(chain.mass.inv_mass)
    chain.estimate_mass(burn=200, thin=2, diagonal=False)
    OUT["long_mass_full"] = np.array(chain.mass.inv_mass)


def bounds_and_masses():
    rng = np.random.default_rng(hh.SEED + 1)
    bounds = Bounds(lower=hh.LOWER, upper=hh.UPPER)
    points = hh.LOWER + (hh.UPPER - hh.LOWER) * rng.uniform(-5.0, 6.0, size=(64, 3))
    OUT["bounds_points"] = points
    OUT["bounds_reflect"] = np.array([bounds.reflect(p) for p in points])
    both = [bounds.reflect_momenta(p) for p in points]
    OUT["bounds_reflect_momenta"] = np.array([b[0] for b in both])
    OUT["bounds_reflections"] = np.array([b[1] for b in both])
    assert OUT["bounds_reflections"].min() == -1 and OUT["bounds_reflections"].max() == 1
    for name, inverse_mass in (("scalar", 0.25), ("vector", hh.S ** 2), ("matrix", hh.FULL)):
        mass = get_particle_mass(inverse_mass, 3)
        draws = np.random.default_rng(hh.SEED + 2)
        OUT[f"momentum_{name}"] = np.array([mass.sample_momentum(draws) for _ in range(4)])
        OUT[f"velocity_{name}"] = np.array([mass.get_velocity(r) for r in OUT[f"momentum_{name}"]])


def main():
    for name, (_, steps) in hh.CASES.items():
        trace(name, name, steps)
    long_case()
    bounds_and_masses()
    path = os.path.join(HERE, "hmc.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
