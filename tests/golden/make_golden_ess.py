"""
Golden vectors of the reference's effective_sample_size (mcmc/utilities.py:83-95), GibbsChain.estimate_burn_in and the
ESS of plot_diagnostics (mcmc/gibbs.py:405-431, :577-592), transition_matrix_plot (plotting.py:457-554) and
ParallelTempering.swap_diagnostics (mcmc/parallel.py:328-362), written to ess.npz beside this file by IMPORTING the
reference the way make_golden.py does.  Data only (allow_pickle=False).

Run in the build container only:   python tests/golden/make_golden_ess.py

The inputs are the seeded recipes of tests/ess_host.py (`case`); of each, the archive holds the first and last 8 values
(`<case>_ends`).  Per case `<case>_ess` is the reference's integer per column, and `<case>_f0`, `<case>_sum`,
`<case>_cut` come from the reference's own NumPy expressions (irfft(abs(rfft(x - mean(x))) ** 2), its first half, argmax
of f < 0, the sum of what is left).  For the odd-n cases the archive also holds the numbers of the direct lag sums of
tests/ess_host.py (`<case>_mirror_*`), because there the reference's f is not the autocorrelation of the sample.

Every even-n column is ASSERTED to keep its distance from the two places where a rounding error could change an
integer: min |f[k]| / f[0] over k <= cut and |n / tau - round(n / tau)| / (n / tau) are both at least 1e-7, 500 times
the tolerance of the GPU tests.  (A column with cut == 1 has sum == f[0] bit for bit on either route, so n / tau is n
exactly and safely so: the second bound is not asked of it.  tiny_4 is such a column - with n = 4 no other cut exists.)

Cases
  ar_<n>      AR(1) columns with phi = 1 - logspace(-3, 0, p), plus 5: (4096, 256), (20000, 8); odd: (4097, 8), (65, 8)
  ramp_<n>    arange(n) / 4 - 7 for n = 4096, 8190, 20000; odd: 8191
  cos_<c>     3 + 2 cos(2 pi t / n), n = 4 c - 2: the first negative lag is exactly c
  layout      (258, 129): every column count and view of the layout tests is a slice of it
  tiny_4      the shortest sample with an answer
  chain       the reference's GibbsChain run for 3000 steps on a correlated 3-parameter Gaussian (parameter 1 bounded,
              parameter 2 non-negative): samples, probs, the width logs, estimate_burn_in(), the ESS of plot_diagnostics
  tm_*        transition_matrix_plot of a seeded 4 x 4 matrix, read off the axis it drew on under Agg: whole, and
              upper-triangular without the diagonal
  swap_*      swap_diagnostics of counters made from the same matrix, read off the figure it drew
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import make_golden as mg  # noqa: E402,F401  (imports the reference; exits when it is absent)
import numpy as np  # noqa: E402
from inference.mcmc import GibbsChain, ParallelTempering  # noqa: E402
from inference.mcmc.utilities import effective_sample_size  # noqa: E402
from inference.plotting import transition_matrix_plot  # noqa: E402
from numpy.fft import irfft, rfft  # noqa: E402

import ess_host as eh  # noqa: E402

OUT = {}


def reference_numbers(x):
    """f0, sum, cut and the whole kept half f, by the expressions of utilities.py:85-94."""
    f = irfft(abs(rfft(x - np.mean(x))) ** 2)
    f = f[: len(f) // 2]
    cut = int(np.argmax(f < 0.0))
    return f[0], f[:cut].sum(), cut, f


def record(name, even):
    s = eh.case(name)
    n = s.shape[0]
    OUT[f"{name}_ends"] = eh.ends(s)
    OUT[f"{name}_ess"] = np.array([effective_sample_size(c) for c in s.T], dtype=np.int64)
    nums = [reference_numbers(c) for c in s.T]
    OUT[f"{name}_f0"] = np.array([v[0] for v in nums])
    OUT[f"{name}_sum"] = np.array([v[1] for v in nums])
    OUT[f"{name}_cut"] = np.array([v[2] for v in nums], dtype=np.int64)
    if even:
        lag_margin, int_margin = np.inf, np.inf
        for f0, total, cut, f in nums:
            assert cut >= 1, name
            lag_margin = min(lag_margin, np.abs(f[: cut + 1]).min() / f0)
            if cut > 1:
                q = n / (total / f0)
                int_margin = min(int_margin, abs(q - round(q)) / q)
        assert lag_margin >= eh.MARGIN and int_margin >= eh.MARGIN, (name, lag_margin, int_margin)
        print(f"{name:12s} cuts {OUT[f'{name}_cut'].min()} .. {OUT[f'{name}_cut'].max()}, ess {OUT[f'{name}_ess'].min()} .. "
              f"{OUT[f'{name}_ess'].max()}, margins {lag_margin:.1e} {int_margin:.1e}")
    else:
        f0, total, cut, ess = eh.mirror(s)
        OUT[f"{name}_mirror_f0"], OUT[f"{name}_mirror_sum"] = f0, total
        OUT[f"{name}_mirror_cut"], OUT[f"{name}_mirror_ess"] = cut, ess
        rel = np.abs(total / f0 - OUT[f"{name}_sum"] / OUT[f"{name}_f0"]) / (total / f0)
        print(f"{name:12s} reference {OUT[f'{name}_ess'].tolist()} mirror {ess.tolist()} (tau differs by up to {rel.max():.1e})")


def chain_case():
    mean = np.array([0.0, 1.0, 2.0])
    cov = np.array([[1.0, 0.6, -0.3], [0.6, 0.8, 0.2], [-0.3, 0.2, 1.5]])
    icov = np.linalg.inv(cov)

    def posterior(theta):
        d = theta - mean
        return float(-0.5 * d @ icov @ d)

    chain = GibbsChain(posterior=posterior, start=np.array([4.0, 2.5, 5.0]), display_progress=False)
    chain.set_boundaries(1, (-1.0, 3.0))
    chain.set_non_negative(2)
    chain.rng = np.random.default_rng(eh.SEED)
    for k, p in enumerate(chain.params):
        p.rng = np.random.default_rng(eh.SEED + 1 + k)
    chain.advance(3000)
    OUT["chain_samples"] = np.array([p.samples for p in chain.params]).T
    OUT["chain_probs"] = np.array(chain.probs)
    OUT["chain_sigma"] = np.array([p.sigma for p in chain.params])
    for k, p in enumerate(chain.params):
        OUT[f"chain_sigma_values_{k}"] = np.array(p.sigma_values)
        OUT[f"chain_sigma_checks_{k}"] = np.array(p.sigma_checks, dtype=np.float64)
    burn = chain.estimate_burn_in()
    OUT["chain_burn"] = np.array(burn)
    OUT["chain_ess"] = np.array([effective_sample_size(np.array(chain.get_parameter(i, burn=burn))) for i in range(3)],
                                dtype=np.int64)
    f0, total, cut, ess = eh.mirror(chain.get_sample(burn=burn))
    OUT["chain_mirror_f0"], OUT["chain_mirror_sum"], OUT["chain_mirror_cut"], OUT["chain_mirror_ess"] = f0, total, cut, ess
    print(f"chain: length {chain.chain_length}, burn {burn}, ess {OUT['chain_ess'].tolist()}, mirror {ess.tolist()}")


def read_axis(prefix, ax):
    pc = ax.collections[0]
    OUT[f"{prefix}_corners"] = np.array([p.vertices[0] for p in pc.get_paths()])
    OUT[f"{prefix}_sizes"] = np.array([p.vertices[2] - p.vertices[0] for p in pc.get_paths()])
    OUT[f"{prefix}_colors"] = np.array(pc.get_facecolor())
    OUT[f"{prefix}_labels"] = np.array([t.get_text() for t in ax.texts])
    OUT[f"{prefix}_label_xy"] = np.array([t.get_position() for t in ax.texts])
    OUT[f"{prefix}_limits"] = np.array([ax.get_xlim(), ax.get_ylim()])


def plot_cases():
    import matplotlib.pyplot as plt

    rng = np.random.default_rng(eh.SEED + 7)
    rates = rng.random((4, 4))
    OUT["tm_matrix"] = rates
    _, ax = plt.subplots()
    assert transition_matrix_plot(axis=ax, matrix=rates) is ax
    read_axis("tm_full", ax)
    _, ax = plt.subplots()
    transition_matrix_plot(axis=ax, matrix=rates, colormap="plasma", exclude_diagonal=True, upper_triangular=True)
    read_axis("tm_upper", ax)

    attempted = np.identity(4) + np.triu(rng.integers(20, 60, size=(4, 4)), 1)
    successful = np.triu(np.floor(rates * attempted), 1)
    OUT["swap_attempted"], OUT["swap_successful"] = attempted, successful
    ladder = object.__new__(ParallelTempering)  # (the constructor would start one process per chain)
    ladder.N_chains = 4
    ladder.attempted_swaps, ladder.successful_swaps = attempted, successful
    plt.close("all")
    ladder.swap_diagnostics()
    fig = plt.gcf()
    read_axis("swap_axis", fig.axes[0])
    OUT["swap_total"] = np.array([b.get_height() for b in fig.axes[1].patches])
    OUT["swap_rate_matrix"] = successful / attempted.clip(min=1)
    plt.close("all")


def main():
    for name in eh.EVEN + ["layout", "tiny_4"]:
        record(name, even=True)
    for name in eh.ODD:
        record(name, even=False)
    for name in ("const", "tiny_2"):
        OUT[f"{name}_ends"] = eh.ends(eh.case(name))
    chain_case()
    plot_cases()
    path = os.path.join(HERE, "ess.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, {len(OUT)} arrays")


if __name__ == "__main__":
    main()
