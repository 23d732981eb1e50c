"""
Golden vectors of the reference's UnimodalPdf (pdf/unimodal.py), written to unimodal.npz beside this file by IMPORTING
the reference the way make_golden.py does (its module level sets that import up; the file itself is not changed).

Run in the build container only:   python tests/golden/make_golden_unimodal.py

Cases (prefix in the archive; `samples()` below draws every sample from a seed, and the tests carry the same recipe)
  gauss   Gaussian, n = 1500
  gamma   Gamma(3), n = 2000 (skewed)
  t3      Student-t with 3 degrees of freedom, n = 1800 (the fit ends with success=False)
  logn    log-normal, n = 5000: skip = 2, two passes
  big     Gaussian, n = 100 000: skip = 50 (only the first and last 8 samples are stored)
  tiny    n = 30
Per case: the guesses, bounds and sample moments; every theta `posterior` was asked for, in order, with the sum of the
log-densities, the value returned and the stride of the fitted samples; MAP, map_lognorm, the limits, the optimiser's
success flag; pdf and cdf at 400 points from below lwr_limit to above upr_limit and at one scalar; moments();
interval(0.5 / 0.9 / 0.95).

Rounding response.  The fit is path-sensitive, so the archive also holds the reference's own response to rounding-level
noise: the fit is repeated for NOISE_SEEDS seeds with `posterior` multiplied by (1 + 1e-12 u), u in [-1, 1] a hash of
(seed, theta), and the largest deviation from the noise-free fit is stored - of MAP (per component), of pdf / max pdf on
the 400 points and of the noise-free full-sample `posterior` at MAP.
"""
import hashlib
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.pdf import UnimodalPdf  # noqa: E402

OUT = {}
NOISE_SEEDS = 6
NOISE = 1e-12


def samples():
    rng = np.random.default_rng(20261017)
    return {
        "gauss": rng.normal(1.0, 2.0, 1500),
        "gamma": rng.gamma(3.0, 1.0, 2000),
        "t3": rng.standard_t(3, 1800),
        "logn": rng.lognormal(0.0, 0.5, 5000),
        "big": rng.normal(-2.0, 0.7, 100_000),
        "tiny": rng.normal(0.0, 1.0, 30),
    }


class Recorder(UnimodalPdf):
    """The reference's class with every posterior request recorded."""

    def posterior(self, theta):
        total = self.log_pdf_model(self.fitted_samples, theta).sum()
        value = super().posterior(theta)
        if not hasattr(self, "requests"):
            self.requests = []
        stride = 1 if self.fitted_samples.size == self.sample.size else self.skip
        self.requests.append((np.array(theta, dtype=float), float(total), float(value), stride))
        return value


def hash_unit(seed, theta):
    """A deterministic u in [-1, 1] from the bytes of theta."""
    digest = hashlib.blake2b(np.asarray(theta, dtype=np.float64).tobytes(), digest_size=8, salt=seed.to_bytes(8, "little"))
    return int.from_bytes(digest.digest(), "little") / 2.0**63 - 1.0


def noisy_class(seed):
    class Noisy(UnimodalPdf):
        def posterior(self, theta):
            return super().posterior(theta) * (1.0 + NOISE * hash_unit(seed, theta))

    return Noisy


def record(prefix, sample, store_sample=True, fractions=(0.5, 0.9, 0.95)):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pdf = Recorder(sample)
    requests = pdf.requests
    if store_sample:
        OUT[f"{prefix}_sample"] = np.asarray(sample, dtype=float)
    OUT[f"{prefix}_n"] = np.int64(sample.size)
    OUT[f"{prefix}_ends"] = np.concatenate([sample[:8], sample[-8:]])
    OUT[f"{prefix}_skip"] = np.int64(pdf.skip)
    OUT[f"{prefix}_u"] = pdf.u
    OUT[f"{prefix}_w"] = pdf.w
    pdf.fitted_samples = pdf.sample[:: pdf.skip]  # as when the guesses were made
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        guesses, bounds = pdf.generate_guesses_and_bounds()
    OUT[f"{prefix}_moments3"] = np.array(pdf.sample_moments(pdf.fitted_samples))
    pdf.fitted_samples = pdf.sample
    OUT[f"{prefix}_guesses"] = np.array(guesses)
    OUT[f"{prefix}_bounds"] = np.array(bounds)
    OUT[f"{prefix}_rec_theta"] = np.array([r[0] for r in requests])
    OUT[f"{prefix}_rec_sum"] = np.array([r[1] for r in requests])
    OUT[f"{prefix}_rec_post"] = np.array([r[2] for r in requests])
    OUT[f"{prefix}_rec_stride"] = np.array([r[3] for r in requests], dtype=np.int64)
    OUT[f"{prefix}_rec_norm"] = np.array([pdf.norm(r[0]) for r in requests])
    OUT[f"{prefix}_MAP"] = np.array(pdf.MAP)
    OUT[f"{prefix}_map_lognorm"] = np.float64(pdf.map_lognorm)
    OUT[f"{prefix}_limits"] = np.array([pdf.lwr_limit, pdf.upr_limit])
    OUT[f"{prefix}_success"] = np.bool_(pdf.min_result.success)
    span = pdf.upr_limit - pdf.lwr_limit
    x = np.linspace(pdf.lwr_limit - 0.15 * span, pdf.upr_limit + 0.15 * span, 400)
    OUT[f"{prefix}_x"] = x
    OUT[f"{prefix}_pdf"] = pdf(x)
    OUT[f"{prefix}_cdf"] = pdf.cdf(x)
    OUT[f"{prefix}_scalar"] = np.array([x[150], pdf(float(x[150])), pdf.cdf(float(x[150]))])
    OUT[f"{prefix}_moments"] = np.array(pdf.moments())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        OUT[f"{prefix}_intervals"] = np.array([pdf.interval(f) for f in fractions])
    OUT[f"{prefix}_fractions"] = np.array(fractions, dtype=float)
    post_map = UnimodalPdf.posterior(pdf, pdf.MAP)
    OUT[f"{prefix}_post_map"] = np.float64(post_map)

    # the reference's response to rounding-level noise in the objective
    d_map = np.zeros(6)
    d_pdf = d_post = 0.0
    peak = pdf(x).max()
    for seed in range(NOISE_SEEDS):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            noisy = noisy_class(seed)(sample)
        d_map = np.maximum(d_map, np.abs(noisy.MAP - pdf.MAP))
        d_pdf = max(d_pdf, float(np.abs(noisy(x) - pdf(x)).max() / peak))
        d_post = max(d_post, abs(float(UnimodalPdf.posterior(pdf, noisy.MAP)) - float(post_map)))
    OUT[f"{prefix}_spread_MAP"] = d_map
    OUT[f"{prefix}_spread_pdf"] = np.float64(d_pdf)
    OUT[f"{prefix}_spread_post"] = np.float64(d_post)
    print(f"{prefix:6s} n = {sample.size:6d} skip = {pdf.skip:2d} requests = {len(requests):5d} success = {pdf.min_result.success}"
          f"  spread: MAP {d_map.max():.2e} pdf {d_pdf:.2e} posterior {d_post:.2e}", flush=True)
    return pdf


def main():
    for prefix, s in samples().items():
        record(prefix, s, store_sample=s.size <= 5000)
    path = os.path.join(HERE, "unimodal.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
