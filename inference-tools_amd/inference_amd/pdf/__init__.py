"""
Density estimation of 1D and 2D samples (reference: inference/pdf): `GaussianKDE` evaluates its pdf and cdf and runs its
cross-validated bandwidth search on the device (csrc/kde.hip through the gpmi_kde_* entry points), and `KDE2D` its
untruncated sums at scattered points, at its own samples and on grids (csrc/kde2d.hip, gpmi_kde2d_*); `sample_hdi` and
the searches for the mode and the highest-density interval run on the host.  `UnimodalPdf` and `plot_summary` are not
provided.
"""
from inference_amd.pdf.base import DensityEstimator
from inference_amd.pdf.hdi import sample_hdi
from inference_amd.pdf.kde import GaussianKDE
from inference_amd.pdf.kde2d import KDE2D

__all__ = ["DensityEstimator", "GaussianKDE", "KDE2D", "sample_hdi"]
