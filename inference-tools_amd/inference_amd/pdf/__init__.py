"""
Density estimation of 1D samples (reference: inference/pdf): `GaussianKDE` evaluates its pdf and cdf and runs its
cross-validated bandwidth search on the device (csrc/kde.hip through the gpmi_kde_* entry points); `sample_hdi` and the
searches for the mode and the highest-density interval run on the host.  `UnimodalPdf`, `KDE2D` and `plot_summary` are
not provided.
"""
from inference_amd.pdf.base import DensityEstimator
from inference_amd.pdf.hdi import sample_hdi
from inference_amd.pdf.kde import GaussianKDE

__all__ = ["DensityEstimator", "GaussianKDE", "sample_hdi"]
