"""PeakFinding.find_peaks in plain numpy / Python: the rules of include/nxsig.h (scipy.signal.find_peaks 1.15, restated in DESIGN.md
section 3.14) one line at a time, in double on the exactly widened samples, with the sequential distance rule and the library's tie
rule (among equal heights the larger index is visited first).  No scipy here: tests/test_find_peaks_host.py holds this file to the
recorded SciPy results of tests/golden/find_peaks_vectors.json, the GPU tests hold the kernels to this file."""
import math

import numpy as np

F64_PROPS = ("peak_heights", "left_thresholds", "right_thresholds", "prominences", "width_heights", "left_ips", "right_ips", "widths")
S32_PROPS = ("left_bases", "right_bases", "left_edges", "right_edges", "plateau_sizes")
WIDTH_PROPS = ("width_heights", "left_ips", "right_ips", "widths")


def _pair(v):
    try:
        lo, hi = v
    except TypeError:
        lo, hi = v, None
    return lo, hi


def _select(values, lo, hi):
    keep = np.ones(len(values), bool)
    if lo is not None:
        keep &= lo <= values
    if hi is not None:
        keep &= values <= hi
    return keep


def local_maxima(x):
    n, mids, lefts, rights = len(x), [], [], []
    i = 1
    while i < n - 1:
        if x[i - 1] < x[i]:
            j = i + 1
            while j < n - 1 and x[j] == x[i]:
                j += 1
            if x[j] < x[i]:
                lefts.append(i)
                rights.append(j - 1)
                mids.append((i + j - 1) // 2)
                i = j
        i += 1
    return np.array(mids, np.int64), np.array(lefts, np.int64), np.array(rights, np.int64)


def by_distance(x, peaks, distance):
    """the sequential rule: from the highest to the lowest, among equal heights the larger index first"""
    d = math.ceil(distance)
    keep = np.ones(len(peaks), bool)
    order = sorted(range(len(peaks)), key=lambda k: (x[peaks[k]], peaks[k]), reverse=True)
    for j in order:
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and peaks[j] - peaks[k] < d:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < len(peaks) and peaks[k] - peaks[j] < d:
            keep[k] = False
            k += 1
    return keep


def prominences(x, peaks, wlen=None):
    n = len(x)
    w = -1 if wlen is None else math.ceil(wlen)
    prom, lb, rb = np.empty(len(peaks)), np.empty(len(peaks), np.int64), np.empty(len(peaks), np.int64)
    for k, p in enumerate(peaks):
        i_min, i_max = 0, n - 1
        if w >= 2:
            i_min, i_max = max(p - w // 2, 0), min(p + w // 2, n - 1)
        i = lb[k] = p
        left_min = x[p]
        while i_min <= i and x[i] <= x[p]:
            if x[i] < left_min:
                left_min, lb[k] = x[i], i
            i -= 1
        i = rb[k] = p
        right_min = x[p]
        while i <= i_max and x[i] <= x[p]:
            if x[i] < right_min:
                right_min, rb[k] = x[i], i
            i += 1
        prom[k] = x[p] - max(left_min, right_min)
    return prom, lb, rb


def widths(x, peaks, rel_height, prom, lb, rb):
    out = {k: np.empty(len(peaks)) for k in WIDTH_PROPS}
    for k, p in enumerate(peaks):
        h = float(x[p]) - float(prom[k]) * float(rel_height)
        i = int(p)
        while lb[k] < i and h < x[i]:
            i -= 1
        left = float(i)
        if x[i] < h:
            left += (h - float(x[i])) / (float(x[i + 1]) - float(x[i]))
        i = int(p)
        while i < rb[k] and h < x[i]:
            i += 1
        right = float(i)
        if x[i] < h:
            right -= (h - float(x[i])) / (float(x[i - 1]) - float(x[i]))
        out["width_heights"][k], out["left_ips"][k], out["right_ips"][k], out["widths"][k] = h, left, right, right - left
    return out


def line(x, height=None, threshold=None, distance=None, prominence=None, width=None, wlen=None, rel_height=0.5, plateau_size=None):
    """(peaks, properties) of one line, as scipy.signal.find_peaks returns them"""
    with np.errstate(invalid="ignore"):
        x = np.asarray(x).astype(np.float64)
        if distance is not None and distance < 1:
            raise ValueError("`distance` must be greater or equal to 1")
        if wlen is not None and not 1 < wlen:
            raise ValueError(f"`wlen` must be larger than 1, was {wlen}")
        if rel_height < 0:
            raise ValueError("`rel_height` must be greater or equal to 0.0")
        peaks, le, re = local_maxima(x)
        props = {}

        def cut(keep):
            nonlocal peaks
            peaks = peaks[keep]
            for k in props:
                props[k] = props[k][keep]

        if plateau_size is not None:
            props.update(plateau_sizes=re - le + 1, left_edges=le, right_edges=re)
            cut(_select(props["plateau_sizes"], *_pair(plateau_size)))
        if height is not None:
            props["peak_heights"] = x[peaks]
            cut(_select(props["peak_heights"], *_pair(height)))
        if threshold is not None:
            lo, hi = _pair(threshold)
            lt, rt = x[peaks] - x[peaks - 1], x[peaks] - x[peaks + 1]
            props.update(left_thresholds=lt, right_thresholds=rt)
            keep = np.ones(len(peaks), bool)
            if lo is not None:
                keep &= lo <= np.minimum(lt, rt)
            if hi is not None:
                keep &= np.maximum(lt, rt) <= hi
            cut(keep)
        if distance is not None:
            cut(by_distance(x, peaks, distance))
        if prominence is not None or width is not None:
            prom, lb, rb = prominences(x, peaks, wlen)
            props.update(prominences=prom, left_bases=lb, right_bases=rb)
        if prominence is not None:
            cut(_select(props["prominences"], *_pair(prominence)))
        if width is not None:
            w = widths(x, peaks, rel_height, props["prominences"], props["left_bases"], props["right_bases"])
            props.update(widths=w["widths"], width_heights=w["width_heights"], left_ips=w["left_ips"], right_ips=w["right_ips"])
            cut(_select(props["widths"], *_pair(width)))
        return peaks, props


def tensor(x, axis=-1, **opts):
    """every line of x along `axis`: (coordinates int32 (count, rank) in row-major order, {property: (count,)})"""
    x = np.asarray(x)
    axis %= x.ndim
    moved = np.moveaxis(x, axis, -1)
    rows, names = [], None
    for lead in np.ndindex(*moved.shape[:-1]):
        peaks, props = line(moved[lead], **opts)
        names = list(props)
        for k, p in enumerate(peaks):
            coord = list(lead)
            coord.insert(axis, int(p))
            rows.append((tuple(coord), {name: props[name][k] for name in names}))
    if names is None:
        names = list(line(np.zeros(3), **opts)[1])
    rows.sort(key=lambda r: r[0])
    coords = np.array([r[0] for r in rows], np.int32).reshape(len(rows), x.ndim)
    out = {name: np.array([r[1][name] for r in rows], np.int32 if name in S32_PROPS else np.float64) for name in names}
    return coords, out
