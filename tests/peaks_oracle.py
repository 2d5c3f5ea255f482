"""Numpy restatement of PeakFinding.argrelextrema/3 (lib/nx_signal/peak_finding.ex), vectorised over the whole tensor: the mask is
the AND over s = 1 .. shifts of cmp(x, x[clip(i + s)]) and cmp(x, x[clip(i - s)]) along the axis (shifts = max(0, ceil(order))),
then the coordinates of the marked elements in row-major order (np.argwhere) padded with -1 rows to size."""
import math

import numpy as np

COMPARATORS = {"less": np.less, "greater": np.greater, "less_equal": np.less_equal, "greater_equal": np.greater_equal}


def shifts(order):
    return 0 if order <= 0 else int(math.ceil(order))


def mask(x, comparator="less", axis=0, order=1):
    x = np.asarray(x)
    cmp = COMPARATORS[comparator] if isinstance(comparator, str) else comparator
    axis %= x.ndim
    n = x.shape[axis]
    locs = np.arange(n)
    out = np.ones(x.shape, bool)
    with np.errstate(invalid="ignore"):
        for s in range(1, min(shifts(order), max(n - 1, 1)) + 1):   # more shifts clip to the same neighbours
            out &= np.asarray(cmp(x, np.take(x, np.clip(locs + s, 0, n - 1), axis=axis))).astype(bool)
            out &= np.asarray(cmp(x, np.take(x, np.clip(locs - s, 0, n - 1), axis=axis))).astype(bool)
    return out


def nonzero(m):
    m = np.asarray(m).astype(bool)
    idx = np.full((m.size, m.ndim), -1, np.int32)
    hits = np.argwhere(m)
    idx[: len(hits)] = hits
    return idx, np.uint32(len(hits))


def argrelextrema(x, comparator="less", axis=0, order=1):
    return nonzero(mask(x, comparator, axis, order))
