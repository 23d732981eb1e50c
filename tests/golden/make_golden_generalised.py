"""
Fixtures of the generalised GP (GeneralisedGpRegressor), written beside this file.  Data only (allow_pickle=False).

Run in the build container only:   python tests/golden/make_golden_generalised.py

generalised.npz  the cases of tests/test_generalised_gpu.py (tests/generalised_host.py: CASES, make_case): per case the
    inputs (<case>_x, _y, _aux, _theta, _theta2, _pts, _offset), the NumPy mirror's quantities (<case>_logq, _grad, _f,
    _g, _mean, _var, _newton = [Newton steps, halvings]) and the allowance of each (<case>_allow_<quantity>): ten times
    the largest movement of the mirror's own quantity under 48 relative ripples of 1e-13 on the mirror's K (and
    cross-covariances), floored at 1e-10 of the quantity's scale.  The script asserts that every mirror run converges
    and takes the same number of Newton steps and halvings under all 48 ripples - only then may the device's counts be
    compared exactly - and that the outlier case halves a step at least once.  This part needs no reference.
generalised_pair.npz  the case of tests/test_pair_regime_gpu.py (generalised_host.PAIR_CASES: N = 5130, where a handle owns
    the CU-masked stream pair), by the same recipe with 12 ripples instead of 48 (a mirror run takes a dense N = 5130
    Cholesky per Newton step on the host): only the mirror's <case>_logq, _f, _g, _mean, _var, _newton, _offset and the
    allowances - no gradient, and no inputs: the test regenerates them from the seed (make_case).  Every ripple must
    take the plain mirror's Newton steps and halvings here too.  This part needs no reference either.
generalised_lik.npz  the reference's LogisticLikelihood(y, sigma, forward_model=identity)(f) (inference/likelihoods.py)
    at 24 seeded (y, sigma, f) triples of 16 points each, by IMPORTING the reference the way make_golden.py does.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (HERE, os.path.dirname(HERE), os.path.join(ROOT, "inference-tools_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import generalised_host as gh  # noqa: E402
from inference_amd.gp.likelihood import Binomial, Logistic, Poisson  # noqa: E402

LIKS = {"Logistic": Logistic, "Poisson": Poisson, "Binomial": Binomial}
N_RIPPLES = 48
N_RIPPLES_PAIR = 12
QUANTITIES = ("logq", "grad", "f", "g", "mean", "var")


def mirror_part():
    out = {}
    for name in gh.CASES:
        c = gh.make_case(name)
        lik = LIKS[c["lik_name"]](c["aux_arg"])
        aux = lik.bind(len(c["y"]))
        lik.check(c["y"])
        offset = lik.default_offset(c["y"], aux)
        q, log = gh.mirror_quantities(lik, aux, offset, c)
        if name == "logistic_m52":
            assert log[1] >= 1, "the outlier case must halve a step"
        moved = {k: 0.0 for k in QUANTITIES}
        for i in range(N_RIPPLES):
            qr, logr = gh.mirror_quantities(lik, aux, offset, c, ripple=gh.rippler(1000 + i))
            assert logr == log, f"{name}: ripple {i} took {logr} steps / halvings, the plain mirror {log}: another seed"
            for k in QUANTITIES:
                moved[k] = max(moved[k], float(np.abs(qr[k] - q[k]).max()))
        for k in ("x", "y", "theta", "theta2", "pts"):
            out[f"{name}_{k}"] = c[k]
        out[f"{name}_aux"] = c["aux_arg"]
        out[f"{name}_offset"] = np.array(offset)
        out[f"{name}_newton"] = np.array(log)
        for k in QUANTITIES:
            out[f"{name}_{k}"] = np.asarray(q[k])
            allow = max(10.0 * moved[k], 1e-10 * float(np.abs(q[k]).max()))
            out[f"{name}_allow_{k}"] = np.array(allow)
            print(f"{name:14s} {k:5s} scale {float(np.abs(q[k]).max()):10.3e}  moved {moved[k]:9.2e}  allowance {allow:9.2e}")
        print(f"{name:14s} Newton steps / halvings {log}")
    path = os.path.join(HERE, "generalised.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


def pair_part():
    out = {}
    quantities = tuple(k for k in QUANTITIES if k != "grad")
    for name in gh.PAIR_CASES:
        c = gh.make_case(name)
        lik = LIKS[c["lik_name"]](c["aux_arg"])
        aux = lik.bind(len(c["y"]))
        lik.check(c["y"])
        offset = lik.default_offset(c["y"], aux)
        q, log = gh.mirror_quantities(lik, aux, offset, c, want_grad=False)
        moved = {k: 0.0 for k in quantities}
        for i in range(N_RIPPLES_PAIR):
            qr, logr = gh.mirror_quantities(lik, aux, offset, c, ripple=gh.rippler(1000 + i), want_grad=False)
            assert logr == log, f"{name}: ripple {i} took {logr} steps / halvings, the plain mirror {log}: another seed"
            for k in quantities:
                moved[k] = max(moved[k], float(np.abs(qr[k] - q[k]).max()))
        out[f"{name}_offset"] = np.array(offset)
        out[f"{name}_newton"] = np.array(log)
        for k in quantities:
            out[f"{name}_{k}"] = np.asarray(q[k])
            allow = max(10.0 * moved[k], 1e-10 * float(np.abs(q[k]).max()))
            out[f"{name}_allow_{k}"] = np.array(allow)
            print(f"{name:16s} {k:5s} scale {float(np.abs(q[k]).max()):10.3e}  moved {moved[k]:9.2e}  allowance {allow:9.2e}")
        print(f"{name:16s} Newton steps / halvings {log}")
    path = os.path.join(HERE, "generalised_pair.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


def reference_part():
    import make_golden as mg  # noqa: F401  (imports the reference; exits when it is absent)
    from inference.likelihoods import LogisticLikelihood

    rng = np.random.default_rng(2024)
    y = rng.normal(0.0, 2.0, size=(24, 16))
    sigma = rng.uniform(0.05, 3.0, size=(24, 16))
    f = y + sigma * rng.normal(0.0, 4.0, size=(24, 16))  # residuals out to many sigma: both tails of the softplus
    value = np.array([LogisticLikelihood(y[k], sigma[k], forward_model=lambda t: t)(f[k]) for k in range(24)])
    path = os.path.join(HERE, "generalised_lik.npz")
    np.savez_compressed(path, y=y, sigma=sigma, f=f, value=value)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    mirror_part()
    pair_part()
    reference_part()
