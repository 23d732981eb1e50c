"""
Golden vectors of the reference's EnsembleSampler (mcmc/ensemble.py), written to ensemble.npz beside this file by
IMPORTING the reference the way make_golden.py does.  Data only (allow_pickle=False).

Run in the build container only:   python tests/golden/make_golden_ensemble.py

The samplers are the seeded recipes of tests/ensemble_host.py (`build`), run with warnings turned into errors.

Cases
  a, b, c, d   the four traces of ensemble_host.CASES: `<case>_sample`, `_sample_probs`, `_walker_positions`,
               `_walker_probs`, `_total_proposals`, `_failed_updates`, and `_mode`
  b_readouts   get_parameter, get_probabilities, get_sample at a burn and thin, with the default burn, and get_interval
  save_b_*     every array of the file that the reference's `save` writes for case b after its run, and `save_keys`, their
               names; `more_*` is the state after the reference went on for ensemble_host.MORE iterations on a generator
               seeded SEED + 1 (what a sampler loaded from that file must reach)

ASSERTED here: every accept test with q < 1 + 1e-6 has |u - q| >= 1e-6 (no decision hangs on a rounding error); case b
reflects proposals at its bounds; case d has failed updates; and a file written by this package's `save` loads in the
reference with the same arrays.
"""
import os
import sys
import tempfile
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "inference-tools_amd"))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.mcmc import EnsembleSampler  # noqa: E402

import ensemble_host as eh  # noqa: E402

OUT = {}


def trace(name):
    sampler = eh.build(EnsembleSampler, name)
    rec = eh.Recorder(sampler)
    reflected = [0]
    if sampler.bounds is not None:
        reflect = sampler.process_proposal

        def process_proposal(prop):
            reflected[0] += not sampler.bounds.inside(prop)
            return reflect(prop)

        sampler.process_proposal = process_proposal
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sampler.advance(eh.CASES[name]["iterations"])
    for key, value in eh.state(sampler).items():
        OUT[f"{name}_{key}"] = value
    OUT[f"{name}_mode"] = sampler.mode()
    assert np.isfinite(OUT[f"{name}_sample"]).all() and np.isfinite(OUT[f"{name}_sample_probs"]).all(), name
    margin, largest = rec.margins()
    assert margin >= 1e-6, (name, margin)
    assert len(rec.tests) == OUT[f"{name}_total_proposals"].sum()
    print(f"{name}: {len(rec.tests)} proposals for {sampler.n_iterations} x {sampler.n_walkers} updates, "
          f"{int(OUT[f'{name}_failed_updates'].sum())} failed, {reflected[0]} reflected, margin {margin:.1e}, max |p| {largest:.3g}")
    return sampler, reflected[0]


def case_b():
    sampler, reflected = trace("b")
    assert reflected > 0
    OUT["b_parameter"] = sampler.get_parameter(1, burn=16, thin=3)
    OUT["b_probabilities"] = sampler.get_probabilities(burn=16, thin=3)
    OUT["b_sample_thinned"] = sampler.get_sample(burn=16, thin=3)
    OUT["b_parameter_default"] = sampler.get_parameter(2)
    OUT["b_interval_sample"], OUT["b_interval_probs"] = sampler.get_interval(interval=0.9, burn=16, thin=2)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reference.npz")
        sampler.save(path)
        with np.load(path, allow_pickle=False) as D:
            OUT["save_keys"] = np.array(sorted(D.keys()))
            for key in D.keys():
                OUT[f"save_b_{key}"] = D[key]
        # the other direction: a file of this package's sampler in the reference's `load`
        from inference_amd.mcmc import EnsembleSampler as Ours

        ours = eh.build(Ours, "b")
        ours.advance(eh.CASES["b"]["iterations"])
        path = os.path.join(tmp, "ours.npz")
        ours.save(path)
        back = EnsembleSampler.load(path, posterior=eh.post_b)
        for key in ("walker_positions", "walker_probs", "sample", "sample_probs"):
            assert np.array_equal(getattr(back, key), OUT[f"b_{key}"]), key
        assert np.array_equal(np.array(back.total_proposals), OUT["b_total_proposals"])
        assert back.n_iterations == sampler.n_iterations and back.max_attempts == 100 and float(back.alpha) == 3.0
        assert np.array_equal(back.bounds.lower, eh.LOWER_B) and np.array_equal(back.bounds.upper, eh.UPPER_B)
    sampler.rng = np.random.default_rng(eh.SEED + 1)
    sampler.advance(eh.MORE)
    for key, value in eh.state(sampler).items():
        OUT[f"more_{key}"] = value


def main():
    for name in ("a", "c"):
        trace(name)
    case_b()
    trace("d")
    assert OUT["d_failed_updates"].any()
    path = os.path.join(HERE, "ensemble.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
