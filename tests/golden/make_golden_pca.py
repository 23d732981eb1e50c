"""
Golden traces of the reference's PcaChain (mcmc/pca.py), written to pca.npz beside this file by IMPORTING the reference
the way make_golden.py does.  Data only (allow_pickle=False).

Run in the build container only:   python tests/golden/make_golden_pca.py

The chains are the seeded recipes of tests/pca_host.py (`build`), run for 300 steps with warnings turned into errors:
two direction updates, at chain lengths 100 and 250, the second through the blend with the first covariance.

Per case (`plain`, `bounded`, `p5`): `<case>_sample`, `_probs`, `_sigma_values_<i>`, `_sigma_checks_<i>`, `_update_history`,
`_angles_history`, `_directions`, `_covar`, `_burn` (estimate_burn_in), `_mode`, `_update_rows` (the rows of the sample that
went into each covariance), `_ripple_dev` and `_ripple_angles`.

Every trace is ASSERTED to keep its distance from the places where a rounding error could change a decision: every accept
test that drew a uniform has |u - accept_prob| >= 1e-6, at every width review the target rate is at least 1e-6 (relative)
from the 2-sigma edges, and no component of a direction (all of them enter a proposal with their sign) is below 1e-6.
The SIGN of an eigenvector is a decision too, and the touchiest one: LAPACK's dsyevr (the default driver of
scipy.linalg.eigh) normalises no sign, and a change in the last bit of the covariance can turn a direction round, which
mirrors every later proposal along it.  So every recipe is run again under the 48 ripples of pca_host.rippled (relative
amplitudes 2^-44 ... 2^-52) and ASSERTED to make the same number of proposals in every step and to stay within 1e-9 of
the trace.  The logged sines sqrt(1 - d^2) of a small angle carry the rounding of the dot product d divided by the sine
squared, which the deviation of the sample knows nothing of; the device tests hold them to the sample's allowance all the
same, so the largest relative deviation of the sines over all 49 rippled runs (`_ripple_angles`) is ASSERTED to be within
10 `_ripple_dev`: a trace whose own ripples miss the allowance cannot serve as its measure.  The seeds of pca_host.CASES
are seeds for which all of this holds (about one in a thousand does).

`_ripple_dev` is the measure of the device tests' tolerance: the recipe is run again with the reference's `cov` multiplied,
element by element, by 1 + 2^-44 r with a symmetric matrix r of uniform numbers in [-1, 1] - 2^-44 is the smallest power
of two above the device kernel's error bound (2 n + 16) 2^-53 at the largest update of the trace -, the number of
proposals of every step is asserted to be the same, and the largest deviation of the sample is stored.
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
import inference.mcmc.pca as ref_pca  # noqa: E402
from inference.mcmc import PcaChain  # noqa: E402

import pca_host as ph  # noqa: E402

OUT = {}


def trace(name, cov=None):
    chain = ph.build(PcaChain, name)
    rec = ph.Recorder(chain)
    rows = []
    plain_cov = ref_pca.cov

    def watched(data):
        rows.append(data.shape[1])
        return plain_cov(data) if cov is None else cov(plain_cov(data))

    ref_pca.cov = watched
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            rec.run(ph.STEPS)
    finally:
        ref_pca.cov = plain_cov
    return chain, rec, rows


def case(name):
    chain, rec, rows = trace(name)
    for key, value in ph.state(chain).items():
        OUT[f"{name}_{key}"] = value
    assert np.isfinite(OUT[f"{name}_sample"]).all() and np.isfinite(OUT[f"{name}_probs"]).all(), name
    assert chain.chain_length == ph.STEPS + 1 and list(chain.update_history) == ph.UPDATES, chain.update_history
    assert rows == ph.UPDATE_ROWS, rows
    OUT[f"{name}_update_rows"] = np.array(rows, dtype=np.int64)
    OUT[f"{name}_burn"] = np.array(chain.estimate_burn_in())
    OUT[f"{name}_mode"] = chain.mode()
    accept, review, component = rec.margins()
    assert accept >= 1e-6 and review >= 1e-6 and component >= 1e-6, (name, accept, review, component)
    assert (ph.RIPPLE > (2 * max(rows) + 16) * 2.0 ** -53 >= ph.RIPPLE / 2)

    size = chain.n_parameters
    r = np.random.default_rng(ph.CASES[name][4] + 100).uniform(-1.0, 1.0, size=(size, size))
    r = np.triu(r) + np.triu(r, 1).T
    rippled, rec2, _ = trace(name, cov=lambda c: c * (1.0 + ph.RIPPLE * r))
    assert rec2.proposals == rec.proposals, name
    dev = float(np.abs(ph.state(rippled)["sample"] - OUT[f"{name}_sample"]).max())
    first = float(np.abs(ph.state(rippled)["sample"][:100] - OUT[f"{name}_sample"][:100]).max())
    assert first == 0.0 and dev > 0.0, (name, first, dev)
    OUT[f"{name}_ripple_dev"] = np.array(dev)
    angles = float(np.abs(ph.state(rippled)["angles_history"] / OUT[f"{name}_angles_history"] - 1.0).max())
    worst = 0.0
    for k in range(ph.ROBUST_RIPPLES):
        other, rec3, _ = trace(name, cov=ph.rippled(k))
        assert rec3.proposals == rec.proposals, (name, k)
        worst = max(worst, float(np.abs(ph.state(other)["sample"] - OUT[f"{name}_sample"]).max()))
        angles = max(angles, float(np.abs(ph.state(other)["angles_history"] / OUT[f"{name}_angles_history"] - 1.0).max()))
    assert worst < 1e-9, (name, worst)
    # the logged sines are held to the allowance of the sample: the reference's own rippled runs must meet it
    assert angles <= 10.0 * dev, (name, angles, dev)
    OUT[f"{name}_ripple_angles"] = np.array(angles)
    print(f"{name:8s} length {chain.chain_length}, {rec.proposals[-1]} proposals, {len(rec.reviews)} width reviews, "
          f"margins {accept:.1e} {review:.1e} {component:.1e}, burn {int(OUT[f'{name}_burn'])}, ripple dev {dev:.2e} "
          f"(angles {angles:.1e} relative), {ph.ROBUST_RIPPLES} more ripples within {worst:.1e}")


def main():
    for name in ph.CASES:
        case(name)
    path = os.path.join(HERE, "pca.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
