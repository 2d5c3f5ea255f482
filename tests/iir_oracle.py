"""f64 oracle of Filters.sosfilt / sosfilt_zi / sosfiltfilt: scipy.signal 1.15's definitions restated in numpy, vectorised over rows
(tests/test_iir_host.py holds it to recorded scipy results, tests/test_gpu_iir.py holds the kernels to it).  Rows are [rows, n]; states
are [rows, n_sections, 2].  `sos` is [n_sections, 6], or [rows, n_sections, 6] to run a different cascade on every row (cascades of
different lengths are filled up with identity sections, which pass a sample through exactly)."""
import numpy as np

IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def sosfilt(sos, x, zi=None):
    """(y, zf).  Every section runs scipy's transposed direct form II recurrence, y = b0 x + z0; z0 = b1 x - a1 y + z1;
    z1 = b2 x - a2 y, in this order of operations.  The loop runs over time once: at step t section k handles sample t - k, so all
    sections (and all rows) advance in one set of array operations."""
    sos = np.asarray(sos, np.float64)
    x = np.asarray(x, np.float64)
    rows, n = x.shape
    S = sos.shape[-2]
    b0, b1, b2, a1, a2 = (sos[..., k] for k in (0, 1, 2, 4, 5))
    z = np.zeros((rows, S, 2)) if zi is None else np.array(np.broadcast_to(np.asarray(zi, np.float64), (rows, S, 2)))
    z0, z1 = z[..., 0].copy(), z[..., 1].copy()
    xin, y, out = np.zeros((rows, S)), np.zeros((rows, S)), np.empty((rows, n))
    with np.errstate(all="ignore"):
        for t in range(n + S - 1):
            lo, hi = max(0, t - n + 1), min(S - 1, t) + 1   # the sections that have a sample at this step
            if hi > 1:
                xin[:, 1:hi] = y[:, 0:hi - 1]
            if lo == 0:
                xin[:, 0] = x[:, t]
            sl = slice(lo, hi)
            xs = xin[:, sl]
            ys = b0[..., sl] * xs + z0[:, sl]
            z0[:, sl] = b1[..., sl] * xs - a1[..., sl] * ys + z1[:, sl]
            z1[:, sl] = b2[..., sl] * xs - a2[..., sl] * ys
            y[:, sl] = ys
            if t >= S - 1:
                out[:, t - S + 1] = ys[:, -1]
    return out, np.stack([z0, z1], axis=-1)


def sosfilt_backward(sos, x, zi=None):
    """the same filter run from the end of each row towards its start (direction = 1 of the C ABI)"""
    y, zf = sosfilt(sos, np.asarray(x, np.float64)[:, ::-1], zi)
    return y[:, ::-1], zf


def sosfilt_zi(sos):
    """[n_sections, 2]: scipy's lfilter_zi of every section — the solution of (I - A^T) z = B with A the companion matrix of a —
    times the DC gain of the sections ahead of it.  A pole at z = 1 makes the system singular: numpy raises LinAlgError, as scipy does"""
    sos = np.asarray(sos, np.float64)
    zi = np.empty((sos.shape[0], 2))
    scale = 1.0
    for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        i_minus_at = np.array([[1.0 + a1, -1.0], [a2, 1.0]])
        zi[s] = scale * np.linalg.solve(i_minus_at, np.array([b1 - a1 * b0, b2 - a2 * b0]))
        scale = scale * ((b0 + b1 + b2) / (1.0 + a1 + a2))
    return zi


def default_padlen(sos):
    sos = np.asarray(sos, np.float64)
    return 3 * (2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def extend(x, padtype, edge):
    x = np.asarray(x, np.float64)
    if padtype is None or edge == 0:
        return x
    left, right = x[:, edge:0:-1], x[:, -2:-(edge + 2):-1]
    if padtype == "odd":
        return np.concatenate([2 * x[:, :1] - left, x, 2 * x[:, -1:] - right], axis=1)
    if padtype == "even":
        return np.concatenate([left, x, right], axis=1)
    ones = np.ones((1, edge))
    return np.concatenate([x[:, :1] * ones, x, x[:, -1:] * ones], axis=1)


def sosfiltfilt(sos, x, padtype="odd", padlen=None):
    sos = np.asarray(sos, np.float64)
    x = np.asarray(x, np.float64)
    edge = 0 if padtype is None else (default_padlen(sos) if padlen is None else int(padlen))
    assert x.shape[1] > edge
    ext = extend(x, padtype, edge)
    zi = sosfilt_zi(sos)
    y, _ = sosfilt(sos, ext, zi[None] * ext[:, :1, None])
    y, _ = sosfilt(sos, y[:, ::-1], zi[None] * y[:, -1:, None])
    y = y[:, ::-1]
    return y[:, edge:y.shape[1] - edge]


def pad_sections(sos, n_sections):
    """sos filled up to n_sections with identity sections at its end"""
    sos = np.asarray(sos, np.float64)
    return np.concatenate([sos, np.tile(IDENTITY, (n_sections - sos.shape[0], 1))], axis=0)


def nerr(got, ref):
    """the project's error measure: per row, the largest error over the row's largest reference magnitude; the worst row"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    return float((np.abs(got - ref) / np.where(scale > 0, scale, 1.0)).max())
