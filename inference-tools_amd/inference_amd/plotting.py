"""
The matrix plot of a set of variables: every 1D and 2D marginal distribution (reference: plotting.py:19-303).

`matrix_plot_data` computes everything the plot shows - axis limits and arrays, the 1D estimates, the 2D densities and
the highest-density levels - as plain arrays; that is where the device works (`GaussianKDE`, `KDE2D.grid` and
`KDE2D.at_samples`).  `matrix_plot` is the renderer over those arrays.

The highest-density bands of a set of model realisations and the trace plot (reference: plotting.py:306-454) are split
the same way: `hdi_plot_data` and `trace_plot_data` ask the device for every interval of every column in one call
(`sample_hdi_batch`), and `hdi_plot` and `trace_plot` draw the arrays.  matplotlib is imported inside the renderers
only: importing this module, or the package, never needs it.

`transition_matrix_plot` (reference: plotting.py:457-554) draws a matrix of transition rates as coloured, labelled
squares; `ParallelTempering.swap_diagnostics` uses it for the acceptance rates of the swaps.
"""
from itertools import cycle, product
from math import ceil, sqrt
from warnings import warn

import numpy as np
from numpy import array, linspace, percentile

from inference_amd.pdf import _messages as msg
from inference_amd.pdf.hdi import sample_hdi, sample_hdi_batch
from inference_amd.pdf.kde import GaussianKDE
from inference_amd.pdf.kde2d import KDE2D

STYLES = ("contour", "hdi", "histogram", "scatter")
AXIS_POINTS = 200  # points of a parameter's axis array; the 2D densities take every fourth
GRID_STEP = 4


def _check_hdi_fractions(hdi_fractions):
    iterable = hasattr(hdi_fractions, "__iter__")
    if not iterable or not all(0 < f < 1 for f in hdi_fractions):
        raise ValueError(msg.matrix_plot_hdi_fractions())


def matrix_plot_data(samples, plot_style="contour", hdi_fractions=(0.35, 0.65, 0.95), *, device=None):
    """
    Everything `matrix_plot` draws for `samples` (a list of 1D arrays, one per parameter), as a dict of plain arrays:

    - "axis_limits" (N, 2): the 98 % highest-density interval of each parameter, widened by 0.3 of its width;
    - "axis_arrays" (N, 200): the axis of each parameter (the interval widened by 0.35);
    - "marginals" (N, 200): the `GaussianKDE` estimate of each parameter on its axis;
    - "pairs": for the styles "contour" and "hdi", a dict keyed (i, j), i > j, of dicts with "x" and "y" (every fourth
      axis value of parameters j and i) and "prob" (50, 50), the `KDE2D(x=samples[j], y=samples[i])` density on their
      grid; for "hdi" also "levels": the percentiles 100 (1 - f) of the density at the samples for f in
      `hdi_fractions`, with the grid's maximum appended, sorted.  Empty for "histogram" and "scatter".
    """
    if plot_style not in STYLES:
        raise ValueError(msg.matrix_plot_style())
    _check_hdi_fractions(hdi_fractions)
    samples = [np.asarray(s) for s in samples]
    axis_limits, axis_arrays, marginals = [], [], []
    for sample in samples:
        # the 98% HDI sets the plot limits
        lwr, upr = sample_hdi(sample, fraction=0.98)
        axis_limits.append([lwr - (upr - lwr) * 0.3, upr + (upr - lwr) * 0.3])
        axis_arrays.append(linspace(lwr - (upr - lwr) * 0.35, upr + (upr - lwr) * 0.35, AXIS_POINTS))
        marginals.append(array(GaussianKDE(sample, device=device)(axis_arrays[-1])))

    pairs = {}
    if plot_style in ("contour", "hdi"):
        for i in range(len(samples)):
            for j in range(i):
                pdf = KDE2D(x=samples[j], y=samples[i], device=device)
                x_ax = axis_arrays[j][::GRID_STEP]
                y_ax = axis_arrays[i][::GRID_STEP]
                entry = {"x": x_ax, "y": y_ax}
                if plot_style == "hdi":
                    sample_probs = pdf.at_samples()
                    pcts = [100 * (1 - f) for f in hdi_fractions]
                    levels = [lv for lv in percentile(sample_probs, pcts)]
                entry["prob"] = prob = pdf.grid(x_ax, y_ax)
                if plot_style == "hdi":
                    levels.append(prob.max())
                    entry["levels"] = array(sorted(levels))
                pairs[(i, j)] = entry
    return {"axis_limits": array(axis_limits), "axis_arrays": array(axis_arrays), "marginals": array(marginals),
            "pairs": pairs}


def matrix_plot(samples, labels=None, show=True, reference=None, filename=None, plot_style="contour", colormap="Blues",
                show_ticks=None, point_colors=None, hdi_fractions=(0.35, 0.65, 0.95), point_size=1, label_size=10, *,
                device=None):
    """
    Construct a 'matrix plot' for a set of variables which shows all possible 1D and 2D marginal distributions, and
    return the figure.

    :param samples: A list of array-like objects containing the samples for each variable.
    :param labels: A list of strings to be used as axis labels for each parameter being plotted.
    :param bool show: Sets whether the plot is displayed.
    :param reference: A list of reference values for each parameter which will be over-plotted.
    :param str filename: File path to which the matrix plot will be saved (if specified).
    :param str plot_style: The type of plot of the 2D marginals: 'contour' for filled contours, 'hdi' for
        highest-density interval contours, 'histogram' for a hexagonal-bin histogram, 'scatter' for a scatterplot.
    :param str colormap: The name of a colormap in ``matplotlib.colormaps``.
    :param bool show_ticks: Axis ticks are shown for fewer than 6 variables unless this is set to True or False.
    :param point_colors: Data which sets the colors of the points of the 'scatter' style.
    :param point_size: The size of the points of the 'scatter' style.
    :param hdi_fractions: The highest-density intervals of the 'hdi' style, as the fraction of the total probability
        contained in each: an iterable of floats, each in the range [0, 1].
    :param int label_size: The font-size used for axis labels.
    :param device: (not in the reference) device index of the density estimates.
    """
    N_par = len(samples)
    if labels is None:  # default axis labels
        labels = [f"p{i}" for i in range(N_par)] if N_par >= 10 else [f"param {i}" for i in range(N_par)]
    elif len(labels) != N_par:
        raise ValueError(msg.matrix_plot_labels())
    if reference is not None and len(reference) != N_par:
        raise ValueError(msg.matrix_plot_reference())
    # an unknown style falls back to the contours
    if plot_style not in STYLES:
        plot_style = "contour"
        warn(msg.matrix_plot_style())
    _check_hdi_fractions(hdi_fractions)
    if show_ticks is None:  # ticks are suppressed from 6 parameters on, to keep things tidy
        show_ticks = N_par < 6

    import matplotlib.pyplot as plt
    from matplotlib import colormaps

    if colormap in colormaps:
        cmap = colormaps[colormap]
    else:
        cmap = colormaps["Blues"]
        warn(msg.matrix_plot_colormap(colormap))
    # the darker end of the colormap draws the 1D marginals
    marginal_color = min(cmap(10), cmap(245), key=lambda c: sum(c[:-1]))

    samples = [np.asarray(s) for s in samples]
    data = matrix_plot_data(samples, plot_style=plot_style, hdi_fractions=hdi_fractions, device=device)

    fig = plt.figure(figsize=(8, 8))
    grid = fig.add_gridspec(N_par, N_par)
    axes = {}
    # bottom row and left column first: the other panels share their axes
    cells = sorted(((i, j) for i in range(N_par) for j in range(i + 1)), key=lambda c: (c[0] != N_par - 1, c[1] != 0))
    for i, j in cells:
        share_x = axes[(N_par - 1, j)] if i < N_par - 1 else None
        share_y = axes[(i, 0)] if (j > 0 and i != j) else None  # the diagonal keeps its own y axis
        axes[(i, j)] = fig.add_subplot(grid[i, j], sharex=share_x, sharey=share_y)

    for (i, j), ax in axes.items():
        if i == j:
            curve = 0.9 * (data["marginals"][i] / data["marginals"][i].max())
            ax.plot(data["axis_arrays"][i], curve, lw=1, color=marginal_color)
            ax.fill_between(data["axis_arrays"][i], curve, color=marginal_color, alpha=0.1)
            if reference is not None:
                ax.plot([reference[i], reference[i]], [0, 1], lw=1.5, ls="dashed", color="red")
            ax.set_ylim([0, 1])
        else:
            x, y = samples[j], samples[i]
            if plot_style == "contour":
                pair = data["pairs"][(i, j)]
                ax.set_facecolor(cmap(256 // 20))
                ax.contourf(pair["x"], pair["y"], pair["prob"], 10, cmap=cmap)
            elif plot_style == "hdi":
                pair = data["pairs"][(i, j)]
                ax.contourf(pair["x"], pair["y"], pair["prob"], levels=pair["levels"], cmap=cmap)
                ax.contour(pair["x"], pair["y"], pair["prob"], levels=pair["levels"], alpha=0.2)
            elif plot_style == "histogram":
                ax.set_facecolor(cmap(0))
                ax.hexbin(x, y, gridsize=35, cmap=cmap)
            elif point_colors is None:
                ax.scatter(x, y, color=marginal_color, s=point_size)
            else:
                ax.scatter(x, y, c=point_colors, s=point_size, cmap=cmap)
            if reference is not None:  # a red ring on a white one
                for edge, width in (("white", 3.5), ("red", 2)):
                    ax.plot(reference[j], reference[i], marker="o", markersize=7, markerfacecolor="none",
                            markeredgecolor=edge, markeredgewidth=width)

        if i == N_par - 1:  # bottom row: labels and limits in x
            ax.set_xlabel(labels[j], fontsize=label_size)
            ax.set_xlim(data["axis_limits"][j])
        if j == 0 and i != 0:  # left column, except the top-left corner: labels and limits in y
            ax.set_ylabel(labels[i], fontsize=label_size)
            ax.set_ylim(data["axis_limits"][i])
        if show_ticks:
            if i < N_par - 1:
                plt.setp(ax.get_xticklabels(), visible=False)
            if j > 0:
                plt.setp(ax.get_yticklabels(), visible=False)
            if i == j:
                ax.set_yticks([])
        else:
            ax.set_xticks([])
            ax.set_yticks([])

    fig.tight_layout()
    fig.subplots_adjust(wspace=0.0, hspace=0.0)
    if filename is not None:
        fig.savefig(filename)
    if show:
        plt.show()
    return fig


def hdi_plot_data(x, sample, intervals=(0.65, 0.95), *, device=None):
    """
    Everything `hdi_plot` draws, as a dict of plain arrays: "x", "intervals" (the fractions, highest first), and "lower"
    and "upper", both of shape ``(len(intervals), len(x))``: the bounds of the highest-density interval of the sample at
    each x, one row per fraction.  `sample` has shape ``(n, len(x))``; one of shape ``(len(x), n)`` is transposed (as a
    view: the device reads either layout in place).  All the intervals of all the columns come from one device call.
    """
    # order the intervals from highest to lowest
    intervals = array(intervals)
    intervals.sort()
    intervals = intervals[::-1]
    if not all((intervals > 0.0) & (intervals < 1.0)):
        raise ValueError(msg.hdi_plot_intervals())
    s = np.asarray(sample)
    if s.shape[1] != len(x):
        if s.shape[0] == len(x):
            s = s.T
        else:
            raise ValueError(msg.hdi_plot_dimensions())
    bands = sample_hdi_batch(s, [float(f) for f in intervals], device=device)
    return {"x": x, "intervals": intervals, "lower": bands[:, 0, :], "upper": bands[:, 1, :]}


def hdi_plot(x, sample, intervals=(0.65, 0.95), colormap="Blues", axis=None, label_intervals=True, color_levels=None, *,
             device=None):
    """
    Plot highest-density intervals for a given sample of model realisations, and return the axis.

    :param x: The x-axis locations of the sample data as a ``numpy.ndarray``.
    :param sample: A ``numpy.ndarray`` containing the sample data, which has shape ``(n, len(x))`` where ``n`` is the
        number of samples.
    :param intervals: A tuple containing the fractions of the total probability for each interval.
    :param str colormap: The colormap to be used for plotting the intervals: the name of a colormap present in
        ``matplotlib.colormaps``.
    :param axis: A ``matplotlib.pyplot`` axis object which will be used to plot the intervals.
    :param bool label_intervals: If ``True``, labels are assigned to each interval plot such that they appear in the
        legend when using ``matplotlib.pyplot.legend``.
    :param color_levels: A list of integers in the range [0,255] which specify the color value within the chosen color
        map to be used for each of the intervals.
    :param device: (not in the reference) device index of the interval computation.
    """
    data = hdi_plot_data(x, sample, intervals, device=device)
    intervals = data["intervals"]

    import matplotlib.pyplot as plt
    from matplotlib import colormaps

    if colormap in colormaps:
        cmap = colormaps[colormap]
    else:
        cmap = colormaps["Blues"]
        warn(msg.matrix_plot_colormap(colormap))
    if color_levels is None:  # the colors of the intervals
        lwr = 0.20
        upr = 1.0
        color_levels = 255 * ((upr - lwr) * (1 - intervals) + lwr)
    colors = [cmap(int(c)) for c in color_levels]
    if axis is None:
        _, axis = plt.subplots()
    for frac, col, lower, upper in zip(intervals, colors, data["lower"], data["upper"]):
        lab = f"{int(100 * frac)}% HDI" if label_intervals else None
        axis.fill_between(x, lower, upper, color=col, label=lab)
    return axis


def trace_plot_data(samples, *, device=None):
    """
    The y-limits and y-ticks `trace_plot` gives each parameter of `samples` (a list of 1D arrays), as a dict of the
    arrays "limits" (N, 2) and "ticks" (N, 3): with (lwr, upr) the 99 % highest-density interval and mid the centre of
    the 10 % one, the limits are lwr - 0.7 (mid - lwr) and upr + 0.7 (upr - mid), the ticks lwr - 0.5 (mid - lwr), mid and
    upr + 0.5 (upr - mid).  Samples of equal length are answered by one device call with both fractions; a ragged list
    takes one call per sample.
    """
    samples = [np.asarray(s, dtype=np.float64) for s in samples]
    fractions = (0.99, 0.10)
    if samples and all(s.ndim == 1 for s in samples) and len({s.size for s in samples}) == 1:
        hdis = sample_hdi_batch(array(samples).T, fractions, device=device)  # one column per parameter
    else:
        hdis = np.stack([sample_hdi_batch(s, fractions, device=device) for s in samples], axis=-1) if samples \
            else np.empty((2, 2, 0))
    lwr, upr = hdis[0]
    mid = 0.5 * (0 + hdis[1, 0] + hdis[1, 1])
    limits = np.stack([lwr - (mid - lwr) * 0.7, upr + (upr - mid) * 0.7], axis=-1)
    ticks = np.stack([lwr - (mid - lwr) * 0.5, mid, upr + (upr - mid) * 0.5], axis=-1)
    return {"limits": limits, "ticks": ticks}


def trace_plot(samples, labels=None, show=True, filename=None, *, device=None):
    """
    Construct a 'trace plot' for a set of variables which displays the value of the variables as a function of step
    number in the chain, and return the figure.

    :param samples: A list of array-like objects containing the samples for each variable.
    :param labels: A list of strings to be used as axis labels for each parameter being plotted.
    :param bool show: Sets whether the plot is displayed.
    :param str filename: File path to which the plot will be saved (if specified).
    :param device: (not in the reference) device index of the interval computation.
    """
    N_par = len(samples)
    if labels is None:
        labels = [f"p{i}" for i in range(N_par)] if N_par >= 10 else [f"param {i}" for i in range(N_par)]
    elif len(labels) != N_par:
        raise ValueError(msg.trace_plot_labels())
    data = trace_plot_data(samples, device=device)

    import matplotlib.pyplot as plt

    # if for 'n' columns we allow up to m = 2*n rows, set 'n' to be as small as possible given the number of
    # parameters, then make m as small as we can
    n = int(ceil(sqrt(0.5 * N_par)))
    m = int(ceil(float(N_par) / float(n)))

    fig = plt.figure(figsize=(12, 8))
    grid_inds = product(range(m), range(n))
    colors = cycle(["C0", "C1", "C2", "C3", "C4"])
    axes = {}
    for k, (s, label, (i, j), col) in enumerate(zip(samples, labels, grid_inds, colors)):
        share = {} if (i == 0 and j == 0) else {"sharex": axes[(0, 0)]}
        ax = axes[(i, j)] = plt.subplot2grid((m, n), (i, j), **share)
        ax.plot(s, ".", markersize=4, alpha=0.15, c=col)
        ax.set_ylabel(label)
        ax.set_ylim(list(data["limits"][k]))
        ax.set_yticks(list(data["ticks"][k]))
        if i < m - 1:
            plt.setp(ax.get_xticklabels(), visible=False)
        else:
            ax.set_xlabel("chain step #")
    fig.tight_layout()
    if filename is not None:
        plt.savefig(filename)
    if show:
        plt.show()
    return fig


def transition_matrix_plot(axis=None, matrix=None, colormap="viridis", exclude_diagonal=False, upper_triangular=False):
    """
    Plot the transition matrix of a Markov chain, one unit square per element centred on ``(i + 1, j + 1)``, and return
    the axis.

    :param axis: A ``matplotlib.pyplot`` axis object on which the matrix will be plotted.  If not specified, a new
        axis is created for the plot.
    :param matrix: A 2D ``numpy.ndarray`` of the transition probabilities, which should be in the range [0, 1].
    :param str colormap: The name of a colormap in ``matplotlib.colormaps``; any other name warns and draws viridis.
    :param bool exclude_diagonal: If ``True`` the diagonal of the matrix is not plotted.
    :param bool upper_triangular: If ``True`` only the elements with ``i <= j`` are plotted.
    """
    if type(matrix) is not np.ndarray:
        raise TypeError(msg.transition_matrix_type())
    if len(matrix.shape) != 2:
        raise ValueError(msg.transition_matrix_ndim())
    if matrix.shape[0] != matrix.shape[1]:
        raise ValueError(msg.transition_matrix_square())
    if matrix.shape[0] == 1:
        raise ValueError(msg.transition_matrix_size())

    import matplotlib.pyplot as plt
    from matplotlib import colormaps, patheffects
    from matplotlib.collections import PatchCollection
    from matplotlib.patches import Rectangle

    N = matrix.shape[0]
    cells = [(i, j) for i in range(N) for j in range(N)
             if (i <= j or not upper_triangular) and (i != j or not exclude_diagonal)]
    first = [i for i, _ in cells]
    second = [j for _, j in cells]

    if colormap in colormaps:
        cmap = colormaps[colormap]
    else:
        cmap = colormaps["viridis"]
        warn(msg.matrix_plot_colormap(colormap))

    top = matrix.max()
    squares = PatchCollection([Rectangle((i + 0.5, j + 0.5), 1, 1) for i, j in cells],
                              facecolors=[cmap(matrix[i, j] / top) for i, j in cells], edgecolors=["black"] * N)
    if axis is None:
        _, axis = plt.subplots()
    axis.add_collection(squares)
    axis.set_xlim([min(first) + 0.5, max(first) + 1.5])
    axis.set_ylim([min(second) + 0.5, max(second) + 1.5])

    if N < 11:  # the rates as text, white with a black outline, while they are still legible
        outline = [patheffects.Stroke(linewidth=1.5, foreground="black"), patheffects.Normal()]
        for i, j in cells:
            label = axis.text(i + 1, j + 1, "{}%".format(int(matrix[i, j] * 100)), horizontalalignment="center",
                              verticalalignment="center", color="white", fontsize=20 - N)
            label.set_path_effects(outline)
    return axis
