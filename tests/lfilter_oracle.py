"""f64 oracle of Filters.lfilter / lfilter_zi / filtfilt / lfiltic: scipy.signal 1.15's definitions restated in numpy, vectorised over
rows (tests/test_lfilter_host.py holds it to recorded scipy results, tests/test_gpu_lfilter.py holds the kernels to it).  Rows are
[rows, n]; states are [rows, order].  The same recurrence can be run in another type (dtype=np.longdouble: the yardstick of the
conditioning figures), and scan_emulated plays the time-parallel scheme of lfilter.scan WITHOUT its conditioning guard, which is how the
tests find a filter the guard has to catch."""
import numpy as np


def normalise(b, a, dtype=np.float64):
    """(b, a, order): both divided by a[0] and filled up with zeros to order + 1 coefficients"""
    b, a = np.atleast_1d(np.asarray(b, dtype)), np.atleast_1d(np.asarray(a, dtype))
    n = max(b.shape[0], a.shape[0]) - 1
    bn, an = np.zeros(n + 1, dtype), np.zeros(n + 1, dtype)
    bn[:b.shape[0]] = b / a[0]
    an[:a.shape[0]] = a / a[0]
    return bn, an, n


def lfilter(b, a, x, zi=None, dtype=np.float64):
    """(y, zf).  scipy's transposed direct form II in scipy's order of operations:
    y = z[0] + b0 x;  z[i] = z[i + 1] + x b[i + 1] - y a[i + 1];  z[n - 1] = x b[n] - y a[n]"""
    b, a, n = normalise(b, a, dtype)
    x = np.asarray(x, dtype)
    rows, m = x.shape
    z = np.zeros((rows, n), dtype) if zi is None else np.array(np.broadcast_to(np.asarray(zi, dtype), (rows, n)))
    y = np.empty((rows, m), dtype)
    if n == 0:
        return b[0] * x, z
    bt, at = b[1:][None, :], a[1:][None, :]
    nxt = np.zeros((rows, n), dtype)   # z[i + 1], with the zero that stands behind the last state
    with np.errstate(all="ignore"):
        for t in range(m):
            xt = x[:, t:t + 1]
            yt = z[:, 0:1] + b[0] * xt
            nxt[:, :n - 1] = z[:, 1:]
            last = xt * bt[:, n - 1:] - yt * at[:, n - 1:]
            z = nxt + xt * bt - yt * at
            z[:, n - 1:] = last   # scipy forms the last state without the zero term (0 + v == v except for v = -0)
            y[:, t] = yt[:, 0]
    return y, z


def lfilter_backward(b, a, x, zi=None):
    """the same filter run from the end of each row towards its start (direction = 1 of the C ABI)"""
    y, zf = lfilter(b, a, np.asarray(x, np.float64)[:, ::-1], zi)
    return y[:, ::-1], zf


def companion(a_norm):
    """A of z[m + 1] = A z[m] + B x[m]: A[i][0] = -a[i + 1], A[i][i + 1] = 1 (scipy's companion(a).T)"""
    n = a_norm.shape[0] - 1
    A = np.zeros((n, n), a_norm.dtype)
    A[:, 0] = -a_norm[1:]
    for i in range(n - 1):
        A[i, i + 1] = 1
    return A


def lfilter_zi(b, a):
    """scipy's: the solution of (I - A) zi = B, B = b[1:] - a[1:] b0.  A pole at z = 1 makes it singular: numpy raises LinAlgError"""
    b, a, n = normalise(b, a)
    if n == 0:
        return np.zeros(0)
    return np.linalg.solve(np.eye(n) - companion(a), b[1:] - a[1:] * b[0])


def lfiltic(b, a, y, x=None):
    b, a = np.atleast_1d(np.asarray(b, np.float64)), np.atleast_1d(np.asarray(a, np.float64))
    N, M = a.shape[0] - 1, b.shape[0] - 1
    y = np.asarray(y, np.float64)
    x = np.zeros(M) if x is None else np.asarray(x, np.float64)
    x = np.r_[x, np.zeros(max(0, M - x.size))]
    y = np.r_[y, np.zeros(max(0, N - y.size))]
    zi = np.zeros(max(M, N))
    for m in range(M):
        zi[m] = np.sum(b[m + 1:] * x[:M - m])
    for m in range(N):
        zi[m] -= np.sum(a[m + 1:] * y[:N - m])
    return zi


def default_padlen(b, a):
    return 3 * max(np.atleast_1d(b).shape[0], np.atleast_1d(a).shape[0])


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


def filtfilt(b, a, x, padtype="odd", padlen=None, f32_rows=False):
    """scipy's method="pad".  f32_rows: the extension and the forward result are rounded to f32, as the device keeps them"""
    x = np.asarray(x, np.float64)
    edge = 0 if padtype is None else (default_padlen(b, a) if padlen is None else int(padlen))
    assert x.shape[1] > edge
    r = (lambda v: v.astype(np.float32).astype(np.float64)) if f32_rows else (lambda v: v)
    ext = r(extend(x, padtype, edge))
    zi = lfilter_zi(b, a)
    y, _ = lfilter(b, a, ext, zi[None] * ext[:, :1])
    y = r(y)
    y, _ = lfilter(b, a, y[:, ::-1], zi[None] * y[:, -1:])
    y = y[:, ::-1]
    return y[:, edge:y.shape[1] - edge]


def nerr(got, ref):
    """the project's error measure: per row, the largest error over the row's largest reference magnitude; the worst row"""
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    return float((np.abs(got - ref) / np.where(scale > 0, scale, 1.0)).max())


# ---- lfilter.scan without its guard, on one row: chunks of C samples per lane, tiles of 64 chunks, at most 64 tiles (one tile per lane
# of the carry).  The powers of A are formed by squaring in long double and rounded to double once, as the library forms them.
LANES, LEVELS = 64, 6


def _matpow(A, e):
    A = A.astype(np.longdouble)
    R = np.eye(A.shape[0], dtype=np.longdouble)
    while e:
        if e & 1:
            R = R @ A
        e >>= 1
        if e:
            A = A @ A
    return R


def _levels(A, e):
    P, out = _matpow(A, e), []
    for _ in range(LEVELS):
        out.append(P.astype(np.float64))
        P = P @ P
    return out


def _scan(v, M):
    """v [lanes, n] <- sum over j <= i of B^(i - j) v_j, level by level as the wave does it"""
    for k in range(LEVELS):
        w = v.copy()
        v[1 << k:] += w[:-(1 << k)] @ M[k].T
    return v


def scan_emulated(b, a, x, chunk):
    """y of one row (1-D x) through pass 1, the carry and pass 2; non-finite tables are used as they are"""
    bn, an, n = normalise(b, a)
    x = np.asarray(x, np.float64)
    m, T = x.shape[0], chunk * LANES
    tiles = -(-m // T)
    assert n >= 1 and tiles <= LANES
    A = companion(an)
    with np.errstate(all="ignore"):
        mc, mt = _levels(A, chunk), _levels(A, T)
        xp = np.zeros(tiles * T)
        xp[:m] = x
        ch = xp.reshape(tiles * LANES, chunk)
        _, ends = lfilter(bn, an, ch)                       # pass 1: every chunk from a zero state
        P = np.stack([_scan(ends[t * LANES:(t + 1) * LANES].copy(), mc) for t in range(tiles)])
        acc = np.zeros((LANES, n))
        acc[:tiles] = P[:, LANES - 1]
        acc = _scan(acc, mt)                                # the carry: one tile per lane, the row starts at zero
        start = np.zeros((tiles, n))
        start[1:] = acc[:tiles - 1]
        states = np.empty((tiles * LANES, n))
        for t in range(tiles):                              # pass 2
            u = np.zeros((LANES, n))
            u[0] = start[t]
            u = _scan(u, mc)
            u[1:] += P[t, :-1]
            states[t * LANES:(t + 1) * LANES] = u
        y, _ = lfilter(bn, an, ch, states)
    return y.reshape(-1)[:m]
