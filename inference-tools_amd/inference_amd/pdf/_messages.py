"""Error / warning texts of the density estimators.  The wording, line breaks and indentation follow the reference
(pdf/kde.py:53-60, pdf/base.py:41-48, pdf/hdi.py:27-91) so that callers that match on messages keep working."""


def _framed(indent: int, owner: str, kind: str, *lines: str) -> str:
    pad = " " * indent
    body = "".join(f"{pad}\r>> {line}\n" for line in lines)
    return f"\n\n{pad}\r[ {owner} {kind} ]\n{body}{pad}"


def kde_too_few_samples() -> str:
    return _framed(16, "GaussianKDE", "error", "Not enough samples were given to estimate the PDF.",
                   "At least 3 samples are required.")


def interval_bad_fraction(owner: str, fraction) -> str:
    return _framed(16, owner, "error", "The 'fraction' argument must have a value greater than",
                   f"zero and less than one, but the value given was {fraction}.")


def hdi_bad_fraction(fraction) -> str:
    return _framed(12, "sample_hdi", "error", "The 'fraction' argument must be a float between 0 and 1,",
                   f"but the value given was {fraction}.")


def hdi_bad_type(kind) -> str:
    return _framed(12, "sample_hdi", "error", "The 'sample' argument should be a numpy.ndarray or a",
                   "Sequence which can be converted to an array, but", f"instead has type {kind}.")


def hdi_bad_ndim(ndim) -> str:
    return _framed(12, "sample_hdi", "error", "The 'sample' argument should be a numpy.ndarray",
                   "with either one or two dimensions, but the given", f"array has dimensionality {ndim}.")


def hdi_too_short() -> str:
    return _framed(12, "sample_hdi", "error", "The first dimension of the given 'sample' array must ",
                   "have have a length of at least 2.")


def hdi_insufficient() -> str:
    return _framed(12, "sample_hdi", "warning", "The given number of samples is insufficient to estimate the interval",
                   "for the given fraction.")


def hdi_inaccurate() -> str:
    return _framed(12, "sample_hdi", "warning",
                   "n_samples * (1 - fraction) is small - calculated interval may be inaccurate.")


def marginal_unimodal() -> str:
    return ("\n\n[ GibbsChain error ]\n>> unimodal=True asks for a UnimodalPdf, which inference_amd does not provide:"
            "\n>> use the default GaussianKDE marginal (unimodal=False).\n")
