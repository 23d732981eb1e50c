"""
Density estimation of 1D and 2D samples (reference: inference/pdf): `GaussianKDE` evaluates its pdf and cdf and runs its
cross-validated bandwidth search on the device (csrc/kde.hip through the gpmi_kde_* entry points), and `KDE2D` its
untruncated sums at scattered points, at its own samples and on grids (csrc/kde2d.hip, gpmi_kde2d_*); `sample_hdi` and
the searches for the mode and the highest-density interval run on the host, and `sample_hdi_batch` sorts the columns of
a sample and finds their narrowest windows on the device (csrc/hdi.hip, gpmi_hdi_columns).  `UnimodalPdf` fits its six-parameter curve
with every sum over the sample on the device (csrc/unimodal.hip, gpmi_unimodal_*) and the Nelder-Mead driving, the
normalisation, the cdf and the moments on the host.  `DensityEstimator.plot_summary` draws either 1D estimate.
"""
from inference_amd.pdf.base import DensityEstimator
from inference_amd.pdf.hdi import sample_hdi, sample_hdi_batch
from inference_amd.pdf.kde import GaussianKDE
from inference_amd.pdf.kde2d import KDE2D
from inference_amd.pdf.unimodal import UnimodalPdf

__all__ = ["DensityEstimator", "GaussianKDE", "KDE2D", "UnimodalPdf", "sample_hdi", "sample_hdi_batch"]
