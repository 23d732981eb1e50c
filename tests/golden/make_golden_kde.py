"""
Golden vectors of the reference's GaussianKDE (pdf/kde.py), sample_hdi (pdf/hdi.py) and the GibbsChain read-out
(mcmc/base.py:75-160, mcmc/gibbs.py:370-377), written to kde.npz beside this file by IMPORTING the reference the way
make_golden.py does (its module level sets that import up; the file itself is not changed).

Run in the build container only:   python tests/golden/make_golden_kde.py

Cases (prefix in the archive)
  bi      bimodal, n = 2000: pdf / cdf at ~1500 points from min - 2 to max + 2 (region edges included), the region table,
          mode, moments, interval(0.5 / 0.9 / 0.95); cross_validation=True with every (width, log-prob) requested
  big     n = 20 000 after numpy.random.seed, cross_validation=True: the subsample, h, three random() draws after
  n3, n8  tiny samples (no HDI bounds for the mode, tiny grids)
  tie     values rounded to 0.1 (many ties), with cross-validation
  t2      Student-t with 2 degrees of freedom, n = 4000 (hundreds of regions)
  bw      an explicit bandwidth
  ovf     two clusters 1e4 apart, n = 1000: the grid search reaches h = inf and the region table raises OverflowError
  chain   a GibbsChain with injected samples and probs: get_interval (burn, thin, samples=) after a seed, and mode()
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.pdf import GaussianKDE, sample_hdi  # noqa: E402
from inference.mcmc import GibbsChain  # noqa: E402

OUT = {}


class Recorder(GaussianKDE):
    """The reference's class with every cross-validation request recorded."""

    requests = []

    def cross_validation_logprob(self, samples, width, c=0.99):
        lp = super().cross_validation_logprob(samples, width, c)
        Recorder.requests.append((float(width), float(lp), samples))
        return lp


def eval_points(s, edges, m=1500):
    pts = np.linspace(s[0] - 2.0, s[-1] + 2.0, m - min(edges.size, 200))
    e = edges if edges.size <= 200 else edges[np.linspace(0, edges.size - 1, 200).astype(int)]
    return np.concatenate([pts, e, [s[0], s[-1]]])


def record(prefix, sample, cv=False, bandwidth=None, fractions=(0.5, 0.9, 0.95), max_cv=5000, points=True, store=True):
    Recorder.requests = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        kde = Recorder(sample, bandwidth=bandwidth, cross_validation=cv, max_cv_samples=max_cv)
    if store:  # (bi_rt and bw reuse bi's sample)
        OUT[f"{prefix}_sample"] = np.asarray(sample, dtype=float)
    OUT[f"{prefix}_h"] = np.float64(kde.h)
    OUT[f"{prefix}_edges"] = kde.tree.edges
    OUT[f"{prefix}_lwr"] = np.array([sl.start for sl in kde.slices])
    OUT[f"{prefix}_upr"] = np.array([sl.stop for sl in kde.slices])
    OUT[f"{prefix}_mode"] = np.float64(kde.mode)
    OUT[f"{prefix}_mode_warnings"] = np.int64(len(w))
    if cv:
        OUT[f"{prefix}_cv_widths"] = np.array([r[0] for r in Recorder.requests])
        OUT[f"{prefix}_cv_logp"] = np.array([r[1] for r in Recorder.requests])
    if points:
        x = eval_points(kde.sample, kde.tree.edges)
        OUT[f"{prefix}_x"] = x
        OUT[f"{prefix}_regions"] = kde.tree.regions[np.searchsorted(kde.tree.edges, x)]
        OUT[f"{prefix}_pdf"] = kde(x)
        OUT[f"{prefix}_cdf"] = kde.cdf(x)
    OUT[f"{prefix}_moments"] = np.array(kde.moments())
    iv = []
    for f in fractions:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            iv.append(kde.interval(f))
    OUT[f"{prefix}_fractions"] = np.array(fractions, dtype=float)
    OUT[f"{prefix}_intervals"] = np.array(iv)
    return kde


def main():
    rng = np.random.default_rng(20261016)
    bi = np.concatenate([rng.normal(-1.5, 0.6, 1200), rng.normal(2.0, 1.0, 800)])
    record("bi", bi, cv=True)
    record("bi_rt", bi, store=False)  # rule of thumb on the same sample

    np.random.seed(7)
    big = np.concatenate([np.random.normal(0.0, 1.0, 12000), np.random.normal(4.0, 0.5, 8000)])
    Recorder.requests = []
    kde = Recorder(big, cross_validation=True)
    OUT["big_sample"] = big
    OUT["big_h"] = np.float64(kde.h)
    # the subsample as positions in the sorted sample (no ties in a continuous draw)
    OUT["big_subsample"] = np.searchsorted(kde.sample, Recorder.requests[0][2]).astype(np.int32)
    OUT["big_cv_widths"] = np.array([r[0] for r in Recorder.requests])
    OUT["big_cv_logp"] = np.array([r[1] for r in Recorder.requests])
    OUT["big_draws"] = np.random.random(3)
    OUT["big_mode"] = np.float64(kde.mode)

    record("n3", np.array([0.3, -1.2, 2.5]), fractions=(0.5, 0.9))
    record("n8", rng.normal(size=8), fractions=(0.5, 0.9))
    record("tie", np.round(rng.normal(0.0, 1.0, 2000), 1), cv=True)
    record("t2", rng.standard_t(2, size=4000))
    record("bw", bi, bandwidth=0.37, store=False)

    ovf = np.concatenate([rng.normal(0.0, 1.0, 500), rng.normal(1e4, 1.0, 500)])
    Recorder.requests = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            Recorder(ovf, cross_validation=True)
            raised = ""
        except OverflowError as err:
            raised = str(err)
    OUT["ovf_sample"] = ovf
    OUT["ovf_error"] = np.array(raised)
    OUT["ovf_cv_widths"] = np.array([r[0] for r in Recorder.requests])
    OUT["ovf_cv_logp"] = np.array([r[1] for r in Recorder.requests])

    # GibbsChain with injected samples and probabilities
    chain = GibbsChain(posterior=lambda t: float(-0.5 * np.sum(np.asarray(t) ** 2)), start=np.zeros(3), display_progress=False)
    L = 1000
    S = rng.normal(size=(L, 3)) * np.array([1.0, 2.0, 0.5])
    P = -0.5 * np.sum(S**2, axis=1) + 0.1 * rng.normal(size=L)
    for i, p in enumerate(chain.params):
        p.samples = list(S[:, i])
    chain.probs = list(P)
    chain.chain_length = L
    OUT["chain_samples"] = S
    OUT["chain_probs"] = P
    OUT["chain_mode"] = chain.mode()
    runs = [(0.95, 1, 1, None), (0.9, 50, 3, None), (0.5, 10, 1, 120), (0.8, 0, 1, 2000), (0.95, 0, 1, 300)]
    for k, (iv, burn, thin, samples) in enumerate(runs):
        np.random.seed(100 + k)
        smp, prb = chain.get_interval(interval=iv, burn=burn, thin=thin, samples=samples)
        OUT[f"chain_iv{k}_args"] = np.array([iv, burn, thin, -1 if samples is None else samples], dtype=float)
        OUT[f"chain_iv{k}_sample"] = smp
        OUT[f"chain_iv{k}_probs"] = prb
        OUT[f"chain_iv{k}_draw"] = np.random.random(2)

    # sample_hdi
    OUT["hdi_2d"] = sample_hdi(S, 0.68)
    OUT["hdi_1d"] = sample_hdi(list(S[:, 1]), 0.9)

    path = os.path.join(HERE, "kde.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
