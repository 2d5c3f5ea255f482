"""Per-frame accuracy of the transforms against a single-precision FFT model (no GPU needed).

The value tests of the suite ask `max |got - ref| / max |ref|` over a whole tensor of white noise for 1e-5.  That metric does not see
(1) how far one frame's energy reaches: the reference transforms frame by frame (lib/nx_signal.ex:94-102, :609), the tuned kernels
    pack several frames into one complex transform, and a frame's bins then carry the round-off of its partners at THEIR level;
(2) a transform that is 10 ... 70 x less accurate than single precision allows (twiddles from an f32 angle or a recurrence).

This module holds what tests/test_accuracy_model_host.py (CPU), tests/test_gpu_frame_isolation.py and
tests/test_gpu_frame_accuracy.py share:

* the REFERENCE: plain double precision.  Frames from `oracle.nx_oracle.as_windowed`, the window product rounded to f32 as the
  reference forms it (:101), then np.fft in complex128 and NOT rounded to c64 (that rounding alone is 4.5e-8, a third of what is
  measured here).  `Nx.fft` / `Nx.ifft`'s 1e-10 clean-up is applied to the double result as the oracle applies it: the samples of an
  inverse transform of 1e-4-level bins are ~4e-6, and a component the clean-up zeroes moves by up to 1e-10 = 2e-5 of that —
  part of the operation (kernel and model do it too), not transform error.
* the MODEL: the same operation through scipy.fft on complex64 input (pocketfft runs natively in single precision at any length).
  For istft the oracle's own chain with its inverse transform swapped for scipy's; for FIR rows scipy.signal.fftconvolve on float32
  operands against `oracle.nx_oracle.direct_convolve_f64`.
* the METRIC: `frame_errors` / `segment_errors`: per frame (per hop-segment of an istft output), max norm and l2 norm of the
  difference over the same norm of the reference, the latter maximised over the frames of the SAME ROW within `reach` of the frame.
  reach = 1 is the frame's own level.  The neighbourhood form does not depend on how a kernel aligns its units.
* `REACH`: how many consecutive frames of a row can share one complex transform in every dispatch family, read off the kernels.
* the mixed-level inputs of the isolation tests and numpy stand-ins for a kernel (textbook radix-2 in f32, its pair-packed form, and
  degraded variants) that show the metric bites.
* the long rows of kernels_nd.hip (FFT_ROWS_LONG and the tables beside it): `fourstep_f32`, a four-step split like the kernel's with
  its two-level twiddle table, the table re-seeded recurrence of pass A and degraded forms of it; `bluestein_f32`, the chirp-z chain in
  single precision (the floor of fft.big.blue's algorithm, part of that family's model); `long_impulse_rows`.

The margin of every test is 3 x the model's figure on the same data and statistic: correct f32 FFTs of different factorisation and
packing lie within 1.2 x of each other, an f32 Bluestein built from scipy's transforms at 1.0-1.7 x of the direct transform (0.6-1.9 x at the
lengths of fft.big.blue, where pocketfft's own transform of a prime length is the less accurate of the two), the
sloppy variants at 2.2 x and above (tests/test_accuracy_model_host.py measures them)."""
import os

import numpy as np
import scipy.fft
import scipy.signal

from oracle import nx_oracle as O

f32, f64, c64, c128 = np.float32, np.float64, np.complex64, np.complex128

MARGIN = 3.0
PROBE = os.environ.get("NXSIG_ACCURACY_PROBE") == "1"

# Consecutive frames of one row that can share one complex transform, per dispatch family (the prefixes of
# tests/test_gpu_dispatch_table.py; a record "stft.pair.1r+stft.pair.1r.edge" belongs to "stft.pair").  An int, or {frame length: int}.
REACH = {
    # ---- stft, f32 samples
    "stft.pair": 2,            # nx_signal_amd/csrc/wave_stft.hpp:108 (kModePair: two adjacent real frames as re / im), :571 (FPU)
    "stft.quad2": 4,           # wave_stft.hpp:110-112 (kModeQuad: 2J frames, the J complex sequences INTERLEAVED into one C-point
    "stft.quad4": 8,           # wave_stft.hpp:110-112: transform z[J n + j] = c_j[n], separated by a lane-local inverse radix-J butterfly,
    "stft.quad8": 16,          # wave_stft.hpp:571 (FPU = 2 J): the unit is 2J frames, not J transforms of two
    "stft.real2x": 1,          # wave_stft.hpp:109 (kModeReal2x: ONE real frame as even / odd samples)
    "stft.real2x.4k": 1,       # wave_stft.hpp:109, :1569 (the same front-end on the 2048-point core)
    "stft.8k": 1,              # kernels_wave_8k.hip:1-8 (one wave = one real frame, four passes through the core)
    "stft.r20": 2,             # kernels_wave_r20.hip:6-7 (two real frames as re / im of one 20 x 20 transform; the three transforms
                               #   of a wave live in separate 20-lane groups, :21)
    "stft.rab": 2,             # wave_rab.hpp:14 (two real frames per transform; T transforms per wave in separate lane groups, :70)
    "stft.blue": 2,            # wave_stft.hpp:1193-1194, :1257 (u = frame A + i frame B through one chirp-z convolution)
    "stft.generic.blue": 1,    # kernels_generic.hip:1378 (grid = one workgroup per frame)
    "stft.generic.pow2": 1,    # kernels_generic.hip:143-152 (F frames per workgroup, each its own K-point rows), :83
    "stft.generic.dft": 1,     # kernels_generic.hip:1385 (one workgroup per frame)
    # sinks of the same front-ends (wave_stft.hpp:1570: "<sink>.<front-end>")
    "mag.pair": 2,             # wave_stft.hpp:108, :571 (the pair front-end feeding k_stft_mag_wave), :1570
    "mag.quad2": 4,            # wave_stft.hpp:110-112, :571 (the quad front-end, J = 2), :1570
    # ---- stft, c64 samples
    "stft_c64.rab": 1,         # wave_rab.hpp:560-561 (one complex frame per transform, nothing to untangle)
    "stft_c64.rows": 1,        # kernels_wave_rows.hip:275 (the row kernels of Nx.fft: one wave per row)
    # ---- istft
    "istft.wave": 1,           # kernels_wave.hip:9-10 (per frame: c64 load -> inverse FFT); also .deep / .filt
    "istft.wave.mask": 1,      # kernels_wave_mask.hip:120 (one inverse core per frame of the run), kernels_generic.hip:612
    "istft.half": 2,           # kernels_wave.hip:309-311 (TWO consecutive frames per 1024-point inverse FFT)
    "istft.quad": {256: 4, 128: 8},   # kernels_wave.hip:454-457 (J = 1024 / N consecutive frames per 1024-point inverse FFT)
    "istft.dbl": 1,            # kernels_wave.hip:733 (ONE frame per TWO inverse FFTs)
    "istft.4k": 1,             # kernels_wave.hip:190-191 (four passes through the core per frame)
    "istft.r20": 1,            # kernels_wave_r20.hip:396-397 (ONE complex frame per 20-lane group)
    "istft.rab": 1,            # wave_rab.hpp:762 (ONE complex frame per max(A, B)-lane group)
    "istft.rab.q": 1,          # wave_rab.hpp:999 (k_istft_rab_q: the same transform per frame, overlap-add in registers)
    "istft.generic": 1,        # kernels_generic.hip:1438, :1420 (row transforms of nxsig_fft: a row is a frame)
    # ---- rows (the reference itself transforms a row once: no frame-level reach inside a row, none across rows)
    "fft.rows_wave": 1,        # kernels_wave_rows.hip:275 (one wave per row)
    "fft.rows_generic": 1,     # kernels_generic.hip:1420, :1438
    # ---- rows, columns and frames beyond the LDS-resident kernels: the unit is always ONE row / column / frame
    "fft.tiled": 1,            # kernels_nd.hip:287-289 (a tile is T columns of ONE batch row, sequence t in its own LDS lane p * TP + t), :474
    "fft.tiled.columns": 1,    # kernels_nd.hip:502-504 (sequences = the `inner` columns of one plane, one pass of k_fft_tile)
    "fft.big.blue": 1,         # kernels_nd.hip:553-559 (row r is its own P-point chirp-z convolution A[r][.], k_blue_in :134)
    "fft.transpose": 1,        # kernels_nd.hip:236-244 (the five-pass four-step: rows * K2 transforms of K1 points, then rows * K1 of K2)
    "stft.big": 1,             # kernels_nd.hip:1061-1062 (every windowed frame is a row of launch_fft_big)
    "fir.long": 1,             # kernels_nd.hip:749-765 through api.cpp:307-308 (one launch_fftconvolve_nd per row)
    "fftconvolve_nd": 1,       # kernels_nd.hip:749-765 (fft_nd of each operand, product, ifft_nd: a fold of row / column transforms)
    # sinks of the two-frames-per-transform front-ends: the unit is the front-end's
    "mag.r20": 2,              # kernels_wave_r20.hip:6-7, :376 (the r20 front-end feeding the magnitude / one-sided sink)
    "mag.rab": 2,              # wave_rab.hpp:14, :536
    "mag.blue": 2,             # wave_stft.hpp:1193-1194, :1817
}

_SUFFIXES = ("", ".1r", ".edge", ".1r.edge", ".deep", ".h4")


def family_of(record):
    """the REACH key of a dispatch record: the family of its leading entry"""
    first = record.split("+")[0]
    best = None
    for fam in REACH:
        if first == fam or (first.startswith(fam) and first[len(fam):] in _SUFFIXES) or (fam == "fft.rows_generic" and first.startswith(fam + ".")):
            if best is None or len(fam) > len(best):
                best = fam
    return best


def reach_of(family, n=None):
    r = REACH[family]
    return r[n] if isinstance(r, dict) else r


# --------------------------------------------------------------------------------------------------------------- reference and model
def windowed_frames(x, w, hop, padding="valid"):
    """frames of x times the window, each product rounded to f32 (c64 samples: componentwise) -> f32 / c64 [..., M, N]"""
    x = np.asarray(x)
    w = np.asarray(w).astype(f32)
    fr = O.as_windowed(x, w.shape[0], hop, padding)
    if np.iscomplexobj(fr):
        fr = fr.astype(c64)
        return ((fr.real * w) + 1j * (fr.imag * w)).astype(c64)
    return (fr.astype(f32) * w).astype(f32)


def clean(z):
    """Nx.fft's |component| <= 1e-10 -> 0 on a finished transform, in the array's own type"""
    return O._eps_clean(np.asarray(z).astype(c128), O.FFT_EPS).astype(np.asarray(z).dtype)


def stft_reference(x, w, hop, K, padding="valid"):
    """c128 [..., M, K]: double-precision transform of the f32 window products, not rounded"""
    fr = windowed_frames(x, w, hop, padding)
    return O._eps_clean(np.fft.fft(fr.astype(c128 if np.iscomplexobj(fr) else f64), n=K, axis=-1), O.FFT_EPS)


def stft_model(x, w, hop, K, padding="valid"):
    """c64 [..., M, K]: the same frames through a native single-precision transform"""
    fr = windowed_frames(x, w, hop, padding)
    z = scipy.fft.fft(fr.astype(c64), n=K, axis=-1)
    assert z.dtype == c64
    return O._eps_clean(z.astype(c128), O.FFT_EPS).astype(c64)


def _ola(t, hop):
    return O.overlap_and_add(t, t.shape[-1] - hop, dtype=t.dtype)


def _istft_den(w, lead, hop):
    """the reference's guarded normaliser, formed in f32 as the reference forms it (:630-635): data of the operation, not transform error"""
    w = np.asarray(w).astype(f32)
    den = O.overlap_and_add(np.broadcast_to(O._pow32(np.abs(w), 2), lead + (w.shape[0],)), w.shape[0] - hop, dtype=f32)
    return np.where(den > f32(1.0e-10), den, f32(1.0)).astype(f32)


def istft_reference(z, w, hop):
    """c128 [..., M hop + N - hop]: inverse transform, window product and overlap-add in double; the f32 normaliser of the reference"""
    z = np.asarray(z).astype(c64).astype(c128)
    w = np.asarray(w).astype(f32)
    fr = O._eps_clean(np.fft.ifft(z, axis=-1), O.FFT_EPS) * w.astype(f64)
    return _ola(fr, hop) / _istft_den(w, z.shape[:-1], hop).astype(f64)


def istft_model(z, w, hop, ifft=None):
    """c64: oracle.nx_oracle.istft's chain (:609-637, scaling nil) with the inverse transform swapped for a single-precision one"""
    z = np.asarray(z).astype(c64)
    w = np.asarray(w).astype(f32)
    fr = (scipy.fft.ifft(z, axis=-1) if ifft is None else ifft(z)).astype(c64)
    assert fr.dtype == c64
    fr = O._eps_clean(fr.astype(c128), O.FFT_EPS).astype(c64)
    re, im = (fr.real.astype(f32) * w).astype(f32), (fr.imag.astype(f32) * w).astype(f32)
    num = _ola(re.astype(f64) + 1j * im.astype(f64), hop).astype(c64)
    den = _istft_den(w, z.shape[:-1], hop)
    return (num.real.astype(f32) / den + 1j * (num.imag.astype(f32) / den)).astype(c64)


def fir_reference(x, h):
    """f64 [rows, L]: the :same slice (start div(taps - 1, 2), convolution.ex:296) of the full convolution in double"""
    x, h = np.asarray(x, f32), np.asarray(h, f32)
    s = (h.shape[0] - 1) // 2
    return np.stack([O.direct_convolve_f64(r, h)[s: s + x.shape[-1]] for r in x])


def fir_model(x, h):
    """f32 [rows, L]: one single-precision transform per row, like the reference's fftconvolve"""
    x, h = np.asarray(x, f32), np.asarray(h, f32)
    s = (h.shape[0] - 1) // 2
    y = np.stack([scipy.signal.fftconvolve(r, h, mode="full")[s: s + x.shape[-1]] for r in x])
    assert y.dtype == f32
    return y


# ------------------------------------------------------------------------------------------------------------------------- metric
def _neighbourhood_max(v, half):
    """max of v[..., g] over |g - f| <= half, along the last axis"""
    if half <= 0:
        return v
    n = v.shape[-1]
    pad = np.full(v.shape[:-1] + (half,), -np.inf)
    vp = np.concatenate([pad, v, pad], axis=-1)
    out = v.copy()
    for s in range(2 * half + 1):
        out = np.maximum(out, vp[..., s: s + n])
    return out


def _norms(d):
    return np.max(np.abs(d), axis=-1), np.sqrt(np.sum(np.abs(d) ** 2, axis=-1))


def frame_errors(got, ref, reach):
    """got, ref [..., M, K] (leading axes are rows).  For every frame f of every row
    (max_k |got_f - ref_f|, l2 of the difference), each over the same norm of ref_g maximised over the frames g of the SAME row with
    |g - f| < reach.  -> two f64 arrays [..., M]"""
    got, ref = np.asarray(got).astype(c128), np.asarray(ref).astype(c128)
    assert got.shape == ref.shape and got.ndim >= 2 and reach >= 1, (got.shape, ref.shape, reach)
    dm, d2 = _norms(got - ref)
    rm, r2 = _norms(ref)
    tiny = np.finfo(f64).tiny
    return dm / np.maximum(_neighbourhood_max(rm, reach - 1), tiny), d2 / np.maximum(_neighbourhood_max(r2, reach - 1), tiny)


def segments(y, hop):
    """[..., Lout] -> [..., ceil(Lout / hop), hop], the ragged last segment padded with zeros (they add nothing to either norm)"""
    y = np.asarray(y)
    n = -(-y.shape[-1] // hop)
    yp = np.concatenate([y, np.zeros(y.shape[:-1] + (n * hop - y.shape[-1],), y.dtype)], axis=-1)
    return yp.reshape(y.shape[:-1] + (n, hop))


def segment_errors(got, ref, hop, n, reach):
    """istft outputs got, ref [..., M hop + n - hop].  Per hop-segment s: the frames that cover it are s - R + 1 .. s, R = ceil(n / hop);
    the frames within `reach` of those touch the segments s - (R + reach - 2) .. s + (R + reach - 2): the neighbourhood whose loudest
    segment is the denominator.  -> two f64 arrays [..., segments]"""
    got, ref = np.asarray(got).astype(c128), np.asarray(ref).astype(c128)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    dm, d2 = _norms(segments(got - ref, hop))
    rm, r2 = _norms(segments(ref, hop))
    half = -(-n // hop) + reach - 2
    tiny = np.finfo(f64).tiny
    return dm / np.maximum(_neighbourhood_max(rm, half), tiny), d2 / np.maximum(_neighbourhood_max(r2, half), tiny)


def interior_segments(n, hop, M):
    """the segments covered by a full set of R = ceil(n / hop) frames: R - 1 .. M - 1.  At the ends of a row the normaliser falls to
    w^2 of ONE frame (1e-9 under a Hann window), which multiplies the round-off of any single-precision inverse by up to 1e5 — the model's
    included — and the kernels recompute exactly those samples in double (k_istft_edge_chunks): a bound taken over all segments is
    therefore the model's edge figure and says little about the transform.  The inverse tests assert both: every segment against the
    model's worst segment, and the interior against the model's interior."""
    return slice(-(-n // hop) - 1, M)


def inverse_check(family, shape, inp, model_errs, kernel_errs, n, hop, M):
    check(family, shape, inp, worst(model_errs), worst(kernel_errs))
    s = interior_segments(n, hop, M)
    check(family, shape, inp + ":interior", worst((model_errs[0][..., s], model_errs[1][..., s])),
          worst((kernel_errs[0][..., s], kernel_errs[1][..., s])))


def row_errors(got, ref):
    """per row: (max |got - ref| / max |ref|, l2 / l2) over the row's own samples -> two f64 arrays [rows]"""
    em, e2 = frame_errors(np.asarray(got)[:, None, :], np.asarray(ref)[:, None, :], 1)
    return em[:, 0], e2[:, 0]


def worst(pair):
    return float(np.max(pair[0])), float(np.max(pair[1]))


# --------------------------------------------------------------------------------------------------------------------------- inputs
LOUD, QUIET = 1.0, 1.0e-4   # 1e-4 keeps every component far above the 1e-10 clean-up


def mixed_frames_geometry(K, hop, reach, padding="valid", M=None):
    """(M, H, h1, h2): M frames (odd: the last unit of any packing is ragged) over H hops of samples, with one-hop bursts at hop
    indices h1 (even) and h2 (odd) whose frames are at least 4 * reach frames apart and that far from both ends of the row"""
    R = -(-K // hop)
    shift = R // 2 if padding == "reflect" else 0      # :reflect puts K / 2 samples in front of the row
    lo = 4 * reach + R - 1 + shift
    h1 = lo + (lo & 1)
    h2 = h1 + 4 * reach + R - 1
    h2 += 1 - (h2 & 1)
    m_min = max(6 * reach + 13, h2 + shift + 4 * reach + 1)
    m_min += 1 - (m_min & 1)
    if M is None:
        M = m_min
    assert M % 2 == 1 and M >= m_min, (M, m_min)
    if padding == "reflect":
        H = M - 1
        assert hop * R == K and K % 2 == 0
    else:
        H = M - 1 + R
    return M, H, h1, h2


def mixed_signal(K, hop, reach, padding="valid", M=None, seed=0, cplx=False):
    """Four rows: 0 quiet noise, 1 the same noise with two one-hop bursts at level 1, 2 loud throughout, 3 quiet again (the row seam
    behind a loud row).  -> (x f32 / c64 [4, L], M)"""
    M, H, h1, h2 = mixed_frames_geometry(K, hop, reach, padding, M)
    L = H * hop if padding == "reflect" else (M - 1) * hop + K
    rng = np.random.default_rng(seed)

    def noise():
        v = rng.standard_normal(L)
        return v + 1j * rng.standard_normal(L) if cplx else v
    n0, n2, n3 = noise(), noise(), noise()
    x = np.stack([QUIET * n0, QUIET * n0, LOUD * n2, QUIET * n3])
    for h in (h1, h2):
        x[1, h * hop: (h + 1) * hop] = LOUD * n0[h * hop: (h + 1) * hop]
    assert (h2 + 1) * hop <= L
    return np.ascontiguousarray(x.astype(c64 if cplx else f32)), M


def mixed_spectra(N, M, seed=0, loud_frames=(13, 30)):
    """c64 [4, M, N]: noise at 1e-4, frames `loud_frames` of row 1 and all of row 2 at level 1"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((4, M, N)) + 1j * rng.standard_normal((4, M, N))
    lvl = np.full((4, M, 1), QUIET)
    lvl[1, list(loud_frames)] = LOUD
    lvl[2] = LOUD
    return np.ascontiguousarray((z * lvl).astype(c64))


def mixed_rows(L, burst, seed=0, cplx=False):
    """[4, L]: rows 0 and 3 quiet, row 2 loud, row 1 quiet with one burst of `burst` loud samples in its middle (burst = L: loud)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((4, L)) + (1j * rng.standard_normal((4, L)) if cplx else 0)
    lvl = np.full((4, L), QUIET)
    lvl[2] = LOUD
    lvl[1, (L - burst) // 2: (L - burst) // 2 + burst] = LOUD
    return np.ascontiguousarray((v * lvl).astype(c64 if cplx else f32))


def impulse_positions(K, M, seed=0):
    """one position per frame: 0, 1, K/2 - 1, K/2, K - 1, then seeded random ones"""
    fixed = [0, 1 % K, K // 2 - 1, K // 2, K - 1]
    rng = np.random.default_rng(seed)
    p = fixed + [int(v) for v in rng.integers(0, K, max(0, M - len(fixed)))]
    return np.array(p[:M], dtype=np.int64)


def impulse_signal(K, M, rows=2, seed=0, N=None):
    """f32 [rows, M N] for a rectangular window of N samples (default K) at hop = N: frame m of row r holds one 1.0 at position
    p_(m + r) — every output bin is one twiddle chain of magnitude 1, so the max norm is a per-bin figure.  N < K: the frame is
    zero-padded to K by the transform, positions beyond N - 1 fall on N - 1"""
    N = K if N is None else N
    x = np.zeros((rows, M, N), f32)
    for r in range(rows):
        p = np.minimum(np.roll(impulse_positions(K, M, seed), r), N - 1)
        x[r, np.arange(M), p] = 1.0
    return x.reshape(rows, M * N)


def tone_signal(K, hop, M, rows=2, seed=0):
    """f32 [rows, L]: a bin-centred tone plus an off-bin tone at 1e-3 of it (different bins per row)"""
    L = (M - 1) * hop + K
    t = np.arange(L, dtype=f64)
    rng = np.random.default_rng(seed)
    x = []
    for r in range(rows):
        k0 = int(rng.integers(2, max(3, K // 2 - 2)))
        k1 = float(rng.uniform(2, K / 2 - 2))
        x.append(np.cos(2 * np.pi * k0 * t / K + 0.3 * (r + 1)) + 1.0e-3 * np.cos(2 * np.pi * k1 * t / K + 1.1))
    return np.ascontiguousarray(np.array(x).astype(f32))


def impulse_spectra(N, M, rows=2, seed=0):
    """c64 [rows, M, N]: the spectrum of a unit impulse at p_m per frame (every bin of magnitude 1)"""
    k = np.arange(N)
    z = np.zeros((rows, M, N), c64)
    for r in range(rows):
        p = np.roll(impulse_positions(N, M, seed), r)
        z[r] = np.exp(-2j * np.pi * (p[:, None] * k[None, :] % N) / N).astype(c64)
    return z


def one_bin_spectra(N, M, rows=2, seed=0):
    """c64 [rows, M, N]: one bin of magnitude 1 per frame plus a second one at 1e-3 of it"""
    rng = np.random.default_rng(seed)
    z = np.zeros((rows, M, N), c64)
    for r in range(rows):
        for m in range(M):
            k0, k1 = rng.choice(N, 2, replace=False)
            z[r, m, k0] = np.exp(1j * rng.uniform(0, 2 * np.pi))
            z[r, m, k1] = 1.0e-3 * np.exp(1j * rng.uniform(0, 2 * np.pi))
    return z


# ------------------------------------------------------------------------------------------------- numpy stand-ins for a kernel (f32)
def _twiddles(K, kind):
    """w_K^k, k < K / 2 as c64.  "exact": rounded from double; "f32angle": cos / sin of an angle formed in f32;
    "recurrence": w^(k+1) = w^k * w in c64"""
    k = np.arange(K // 2)
    if kind == "exact":
        return np.exp(-2j * np.pi * k / K).astype(c64)
    if kind == "f32angle":
        a = (f32(-2.0) * f32(np.pi) * k.astype(f32) / f32(K)).astype(f32)   # rounded angle: an error of up to ulp(pi) / 2 at k ~ K / 2
        return (np.cos(a.astype(f64)) + 1j * np.sin(a.astype(f64))).astype(c64)
    if kind == "recurrence":
        w = np.empty(K // 2, c64)
        w[0] = 1.0
        step = c64(np.exp(-2j * np.pi / K))
        for i in range(1, K // 2):
            w[i] = c64(w[i - 1] * step)
        return w
    raise KeyError(kind)


def fft_radix2_f32(x, twiddles="exact"):
    """textbook decimation-in-time radix-2 over the last axis (a power of two), every operation in c64"""
    x = np.asarray(x).astype(c64)
    K = x.shape[-1]
    assert K & (K - 1) == 0
    bits = K.bit_length() - 1
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) if bits else 0 for i in range(K)])
    a = x[..., rev]
    w = _twiddles(K, twiddles) if K > 1 else None
    n = 2
    while n <= K:
        a = a.reshape(x.shape[:-1] + (K // n, n))
        tw = w[:: K // n]
        lo, hi = a[..., : n // 2], (a[..., n // 2:] * tw).astype(c64)
        a = np.concatenate([(lo + hi).astype(c64), (lo - hi).astype(c64)], axis=-1).reshape(x.shape)
        n *= 2
    return a


def untangle_pairs(Z):
    """Z [..., K] = FFT(a + i b) for real a, b -> (A, B) in c64 arithmetic"""
    P = np.conj(np.roll(Z[..., ::-1], 1, axis=-1))          # conj Z[(K - k) mod K]
    h = c64(0.5)
    return ((Z + P) * h).astype(c64), ((Z - P) * c64(-0.5j)).astype(c64)


def stft_pair_packed_f32(fr, stride=1, across_rows=False, twiddles="exact"):
    """fr f32 [rows, M, K] windowed frames.  Pairs frame f with frame f + stride inside blocks of 2 * stride frames (stride = 1: the
    pair kernel's packing; stride = 2: a kernel that shares a transform one frame further than it says).  across_rows: the rows are
    flattened first, so the last frame of a row of odd M rides with the first frame of the next row (a seam bug).  A frame
    without a partner rides alone."""
    fr = np.asarray(fr, f32)
    rows, M, K = fr.shape
    flat = fr.reshape(1, rows * M, K) if across_rows else fr
    out = np.empty(flat.shape, c64)
    n = flat.shape[1]
    done = np.zeros(n, bool)
    for f in range(n):
        if done[f]:
            continue
        g = f + stride
        if g < n and not done[g] and (f // stride) % 2 == 0:
            A, B = untangle_pairs(fft_radix2_f32(flat[:, f] + 1j * flat[:, g], twiddles))
            out[:, f], out[:, g] = A, B
            done[f] = done[g] = True
        else:
            out[:, f] = fft_radix2_f32(flat[:, f], twiddles)
            done[f] = True
    return out.reshape(rows, M, K)


def next_pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


def _pad_rows(x, K):
    """rows of n_in samples as c64 rows of K (zero-padded / truncated, like a transform of length K)"""
    x = np.asarray(x).astype(c64)
    out = np.zeros(x.shape[:-1] + (K,), c64)
    n = min(K, x.shape[-1])
    out[..., :n] = x[..., :n]
    return out


def bluestein_f32(x, K, inverse=False):
    """the chirp-z chain of fft.big.blue through scipy.fft on complex64: the floor of the ALGORITHM in single precision.  The chirp
    exp(-i pi n^2 / K) from the exact phase index (n n) mod 2K, evaluated in double and rounded to c64; the spectrum of its conjugate
    formed in double and rounded once (kernels_nd.hip:528-537); two P-point transforms, P the power of two >= 2K - 1.  x [..., n_in]"""
    n = np.arange(K, dtype=np.int64)
    ang = -np.pi * ((n * n) % (2 * K)).astype(f64) / K
    chirp = np.exp(1j * ang).astype(c64)
    P = next_pow2(2 * K - 1)
    b = np.zeros(P, c128)
    b[:K] = np.exp(-1j * ang)
    b[P - K + 1:] = b[1:K][::-1]
    Bf = np.fft.fft(b).astype(c64)
    u = _pad_rows(x, K)
    if inverse:
        u = np.conj(u)
    a = np.zeros(u.shape[:-1] + (P,), c64)
    a[..., :K] = u * chirp
    A = scipy.fft.fft(a, axis=-1)
    assert A.dtype == c64
    v = scipy.fft.ifft((A * Bf).astype(c64), axis=-1)
    assert v.dtype == c64
    z = (v[..., :K] * chirp).astype(c64)
    if inverse:
        z = (np.conj(z) / f32(K)).astype(c64)
    return z


def _fourstep_twiddles(lg, twiddles, reseed):
    """c64 [K1, K2]: w_K^(k1 n2) as pass A of the four-step applies it (kernels_nd.hip:402-426).
    "table": tw_hi[j >> 13] * tw_lo[j & 8191] in c64 at every element (:181-182, :420)
    "recurrence": w[k1] = w[k1 - 1] * w[1] in c64 along k1, taken from the table product where k1 % reseed == 0 (reseed None: only k1 = 0)
    "f32angle": cos / sin of the angle -2 pi j / K formed in f32"""
    K = 1 << lg
    K1 = 1 << ((lg + 1) // 2)
    K2 = K // K1
    j = np.arange(K1, dtype=np.int64)[:, None] * np.arange(K2, dtype=np.int64)[None, :]      # < K
    if twiddles == "f32angle":
        a = (f32(-2.0) * f32(np.pi) * j.astype(f32) / f32(K)).astype(f32)
        return (np.cos(a.astype(f64)) + 1j * np.sin(a.astype(f64))).astype(c64)
    t = np.arange(8192)
    lo = np.exp(-2j * np.pi * (t % K) / K).astype(c64)
    hi = np.exp(-2j * np.pi * ((np.arange((K + 8191) // 8192) * 8192) % K) / K).astype(c64)
    table = (hi[j >> 13] * lo[j & 8191]).astype(c64)
    if twiddles == "table":
        return table
    assert twiddles == "recurrence", twiddles
    w = np.empty_like(table)
    for k1 in range(K1):
        w[k1] = table[k1] if (k1 == 0 or (reseed and k1 % reseed == 0)) else (w[k1 - 1] * table[1]).astype(c64)
    return w


def fourstep_f32(x, lg, reseed=8, twiddles="recurrence"):
    """a forward transform of 2^lg points split like fft.tiled (K1 = 2^ceil(lg / 2) points down the columns n2, the twiddle
    w_K^(n2 k1), K2 points along the rows k1, X[k1 + K1 k2]) with scipy's complex64 sub-transforms: only the twiddle differs
    between the forms, see _fourstep_twiddles.  x c64 [..., 2^lg]"""
    x = np.asarray(x).astype(c64)
    K = 1 << lg
    K1 = 1 << ((lg + 1) // 2)
    K2 = K // K1
    assert x.shape[-1] == K
    y = scipy.fft.fft(x.reshape(x.shape[:-1] + (K1, K2)), axis=-2)             # [k1, n2]
    y = (y * _fourstep_twiddles(lg, twiddles, reseed)).astype(c64)
    z = scipy.fft.fft(y, axis=-1)                                              # [k1, k2]
    assert z.dtype == c64
    return np.ascontiguousarray(np.swapaxes(z, -1, -2)).reshape(x.shape)


def long_impulse_positions(K, count, seed=0):
    """1, K2 - 1, K2 + 1, K / 2 + 1, K - 1 (K2 = 2^floor(log2 K / 2): the row length of the four-step view), then seeded random ones.
    n mod K2 is the column of pass A: at K2 - 1 and K - 1 the twiddle recurrence walks at its longest stride"""
    K2 = 1 << ((int(K).bit_length() - 1) // 2)
    fixed = [1, K2 - 1, K2 + 1, K // 2 + 1, K - 1]
    rng = np.random.default_rng(seed)
    return np.array((fixed + [int(v) for v in rng.integers(0, K, max(0, count - len(fixed)))])[:count], dtype=np.int64)


def long_impulse_rows(K, rows, seed=0):
    """c64 [rows, K]: one unit impulse per row, row r at long_impulse_positions(K, rows, seed)[r] — every output bin is one chain of
    twiddles of magnitude 1, so the max norm is a per-bin figure"""
    x = np.zeros((rows, K), c64)
    x[np.arange(rows), long_impulse_positions(K, rows, seed)] = 1.0
    return x


def fft_rows_reference(x, K, inverse):
    """c128 [rows, K]: np.fft in double on the rows zero-padded to K, with Nx.fft's clean-up"""
    xd = np.asarray(x).astype(c64).astype(c128)
    return clean(np.fft.ifft(xd, n=K, axis=-1) if inverse else np.fft.fft(xd, n=K, axis=-1))


def fft_rows_model_errors(x, K, inverse, ref, family):
    """(max, l2) of the model, worst row.  The direct complex64 transform; for fft.big.blue the larger, per statistic, of that and the
    single-precision chirp-z chain (bluestein_f32), the floor of the algorithm the family is built on"""
    x = np.asarray(x).astype(c64)
    direct = clean(scipy.fft.ifft(x, n=K, axis=-1) if inverse else scipy.fft.fft(x, n=K, axis=-1))
    assert direct.dtype == c64
    m = worst(row_errors(direct, ref))
    if family == "fft.big.blue":
        b = worst(row_errors(clean(bluestein_f32(x, K, inverse)), ref))
        m = (max(m[0], b[0]), max(m[1], b[1]))
    return m


# ------------------------------------------------------------------------------------------------ cases shared by the two GPU modules
# the three launch geometries of tests/test_gpu_stft_pair_loop.py: HOP4 and the general loop both run
PAIR_GEOMETRIES = {
    "headline": {"NXSIG_WAVE_SMALL_W": 0, "NXSIG_WAVE_UNITS_PER_WAVE": 2},
    "three-per-wave": {"NXSIG_WAVE_SMALL_W": 0},
    "one-round": {},
}

# id -> (K, hop, family, options): one case per f32 stft family of the dispatch table (+ the c64 composite kernel), hop = K / 4
FORWARD = {
    "pair-headline": (1024, 256, "stft.pair", {"geometry": "headline", "M": 45}),
    "pair-three-per-wave": (1024, 256, "stft.pair", {"geometry": "three-per-wave", "M": 45}),
    "pair-one-round": (1024, 256, "stft.pair", {"geometry": "one-round", "M": 45}),
    "quad2": (512, 128, "stft.quad2", {}),
    "quad4": (256, 64, "stft.quad4", {}),
    "quad8": (128, 32, "stft.quad8", {}),
    "real2x": (2048, 512, "stft.real2x", {}),
    "real2x-4k": (4096, 1024, "stft.real2x.4k", {}),
    "8k": (8192, 2048, "stft.8k", {"M": 25}),
    "r20": (400, 100, "stft.r20", {}),
    "rab960": (960, 240, "stft.rab", {}),
    # the impulse input needs frames that share no samples.  The 21 x 21 kernel stages a unit's span (5 hops + the frame) in registers
    # and declines spans above 2560 samples (wave_rab.hpp:457), i.e. hop = 441: its impulse frames are 420 samples at hop 420, zero-
    # padded to 441 points by the transform (the positions 0, 1, K/2 - 1, K/2 stay; K - 1 falls on 419)
    "rab441": (441, 110, "stft.rab", {"impulse_N": 420}),
    "blue443": (443, 110, "stft.blue", {}),
    "generic-blue2310": (2310, 577, "stft.generic.blue", {}),
    "generic-pow2-16": (16, 4, "stft.generic.pow2", {}),
    "c64-rab512": (512, 128, "stft_c64.rab", {"cplx": True}),
}
# frames that share no samples, a :reflect case for the pair kernel, and the sinks of the pair and quad2 shapes
FORWARD_EXTRA = {
    "pair-hop-K": (1024, 1024, "stft.pair", {}),
    "quad2-hop-K": (512, 512, "stft.quad2", {}),
    "rab960-hop-K": (960, 960, "stft.rab", {}),
    "pair-reflect": (1024, 256, "stft.pair", {"padding": "reflect"}),
    "pair-magnitude": (1024, 256, "mag.pair", {"sink": "magnitude", "M": 45}),
    "pair-onesided": (1024, 256, "mag.pair", {"sink": "onesided", "M": 45}),
    "quad2-magnitude": (512, 128, "mag.quad2", {"sink": "magnitude"}),
    "quad2-onesided": (512, 128, "mag.quad2", {"sink": "onesided"}),
    "r20-magnitude": (400, 100, "mag.r20", {"sink": "magnitude"}),
    "rab960-onesided": (960, 240, "mag.rab", {"sink": "onesided"}),
    "blue443-magnitude": (443, 110, "mag.blue", {"sink": "magnitude"}),
}
# the sinks of the r20 / rab / Bluestein front-ends: also measured on noise next to the FORWARD cases
FORWARD_SINKS = ("r20-magnitude", "rab960-onesided", "blue443-magnitude")

# id -> (N, hop, family, M, options)
INVERSE = {
    "wave-deep": (1024, 256, "istft.wave", 61, {"lead": "istft.wave.deep"}),
    "wave-mask": (1024, 256, "istft.wave.mask", 61, {"mask": True}),
    "wave-several-runs": (1024, 256, "istft.wave", 41, {}),
    "half": (512, 128, "istft.half", 61, {}),
    "quad": (256, 64, "istft.quad", 61, {}),
    "dbl": (2048, 512, "istft.dbl", 61, {}),
    "4k": (4096, 1024, "istft.4k", 61, {}),
    "r20": (400, 160, "istft.r20", 61, {}),
    "rab960": (960, 240, "istft.rab", 61, {}),
    "rab512-hop160": (512, 160, "istft.rab", 61, {}),
    "rab-q2880": (2880, 720, "istft.rab.q", 61, {}),
    "generic443": (443, 110, "fft.rows_generic", 61, {}),
}

FIR = {33: "fir.wave32", 257: "fir.pair", 513: "fir.r2k", 4097: "fir.dline"}
FIR_L, FIR_BURST = 60000, 2000
FFT_ROWS = {1024: "fft.rows_wave", 4096: "fft.rows_wave", 1000: "fft.rows_generic"}

# rows beyond the LDS-resident kernels (kernels_nd.hip).  id -> (K, family, tuning switches, rows): the smallest shapes that reach
# each distinct piece of arithmetic of launch_fft_big
_NT256, _E2048 = {"NXSIG_FFT_TILE_NT": 256}, {"NXSIG_FFT_TILE_ELEMS": 2048}
FFT_ROWS_LONG = {
    "8192": (8192, "fft.tiled", {}, 2),                    # the smallest tiled length (launch_fft_big's `small` excludes it)
    "2^14": (1 << 14, "fft.tiled", {}, 2),                 # even log2: K1 = K2
    "2^15": (1 << 15, "fft.tiled", {}, 2),                 # odd log2: K1 = 2 K2
    "2^20": (1 << 20, "fft.tiled", {}, 2),                 # the largest tiled length: the high table fully used
    "2^14-nt256": (1 << 14, "fft.tiled", _NT256, 2),       # another stride of the pass-A twiddle recurrence
    "2^17-nt256": (1 << 17, "fft.tiled", _NT256, 2),
    "2^14-elems2048": (1 << 14, "fft.tiled", _E2048, 2),   # and another
    "2^17-elems2048": (1 << 17, "fft.tiled", _E2048, 2),
    "2^14-five-pass": (1 << 14, "fft.transpose", {"NXSIG_FFT_TILED": 0}, 2),
    "2^21": (1 << 21, "fft.transpose", {}, 2),             # the five-pass form where it runs by default
    "blue5000": (5000, "fft.big.blue", {}, 2),             # P = 16384, even
    "blue10007": (10007, "fft.big.blue", {}, 2),           # prime
    "blue4097": (4097, "fft.big.blue", {}, 2),             # the first length past the LDS Bluestein, P = 16384
}
LONG_IMPULSES = 6   # rows of the impulse input: the five named positions of long_impulse_positions and one seeded random one

# id -> (shape [outer, na, inner] or any rank, axes, lengths, family): transforms along an axis that is not the fastest one
COLUMNS = {
    "2x1024x8": ((2, 1024, 8), [1], None, "fft.tiled.columns"),
    "3x16x64": ((3, 16, 64), [1], None, "fft.tiled.columns"),
    "2x100x24-to-128": ((2, 100, 24), [1], [128], "fft.tiled.columns"),
    "2x64x72-two-axes": ((2, 64, 72), [0, 1], [4, 64], "fft.transpose"),   # axis 0 (4 points) goes through transposes, axis 1 is tiled
}

# id -> (N, K, hop, stft family, istft family): M = 5 frames, 2 rows
LONG_FRAMES = {
    "16384": (16384, 16384, 4096, "stft.big", "fft.tiled"),
    "5000": (5000, 5000, 1250, "stft.big", "fft.big.blue"),
}
LONG_FRAMES_M = 5

# id -> (taps, L, switches): more taps than the overlap-save kernels take; the record leads with fir.long
FIR_LONG = {
    "4097-generic": (4097, 30000, {"NXSIG_DISABLE_WAVE": 1}),
    "32770": (32770, 1 << 15, {}),          # the smallest tap count that reaches fir.long by default (launch_fir: taps > 32769)
}

# (shape of in1, shape of in2)
CONV_ND = [((40, 300), (7, 31)), ((64, 64), (9, 9)), ((6, 20, 33), (3, 5, 7))]


def context(switches=None):
    import nx_signal_amd as S
    ctx = S.Context(0)
    for name, v in (switches or {}).items():
        ctx.set_tuning(name, v)
    return ctx


def forward_frames(K, hop, family, opts):
    """M of a forward case (odd, the last unit ragged) for the family's reach"""
    return mixed_frames_geometry(K, hop, reach_of(family), opts.get("padding", "valid"), opts.get("M"))[0]


def run_stft(ctx, x, w, hop, K, padding="valid", sink="spectrum"):
    """-> (host result, dispatch record).  sink "spectrum": c64 [rows, M, K]; "onesided": its bins below K / 2; "magnitude": their |.|"""
    import nx_signal_amd as S
    opts = dict(overlap_length=int(np.asarray(w).shape[0]) - hop, fft_length=K, window_padding=padding)
    if sink == "spectrum":
        z = S.stft(x, w, ctx=ctx, **opts)[0]
    elif sink == "onesided":
        z = S.stft_onesided(x, w, ctx=ctx, **opts)[0]
    else:
        z = S.spectrogram(x, w, ctx=ctx, kind="magnitude", **opts)[0]
    return np.asarray(z), ctx.last_dispatch()


def through_sink(z, sink):
    """a full spectrum (reference c128 or model c64) as the sink would deliver it"""
    if sink == "spectrum":
        return z
    half = z[..., : z.shape[-1] // 2]
    return half if sink == "onesided" else np.abs(half)


def run_istft(ctx, z, w, hop, mask=False):
    import nx_signal_amd as S
    N = int(np.asarray(w).shape[0])
    if mask:
        y = S.istft_masked(z, np.ones(z.shape, f32), w, ctx=ctx, overlap_length=N - hop, fft_length=N)
    else:
        y = S.istft(z, w, ctx=ctx, overlap_length=N - hop, fft_length=N)
    return np.asarray(y), ctx.last_dispatch()


def assert_family(record, family, lead=None):
    if PROBE:
        print(f"\nDISPATCH {family:<18} [{record}]")
        return
    assert family_of(record) == family, f"dispatched to [{record}], the case is about [{family}]"
    if lead:
        assert record.split("+")[0] == lead, (record, lead)


def assert_noted(record, entry):
    """a case whose kernel is not the record's first entry (an n-D fold leads with its first axis): the entry is in the record"""
    if PROBE:
        print(f"\nDISPATCH {entry:<18} [{record}]")
        return
    assert entry in record.split("+"), f"dispatched to [{record}], the case is about [{entry}]"


# ---------------------------------------------------------------------------------------------------------------- probe / recording
def record(rows, family, shape, inp, model, kernel):
    """one line per (case, norm) for profiles/accuracy/per_frame_accuracy.txt; printed under NXSIG_ACCURACY_PROBE=1"""
    for norm, m, k in (("max", model[0], kernel[0]), ("l2", model[1], kernel[1])):
        line = f"{family:<18} {shape:<28} {inp:<14} {norm:<3} model {m:.3e}  kernel {k:.3e}  ratio {k / m if m > 0 else float('inf'):6.2f}"
        rows.append(line)
        if PROBE:
            print("\nACCURACY " + line)


def check(family, shape, inp, model, kernel, rows=None):
    """kernel (max, l2) <= MARGIN x model (max, l2); under the probe the figures are printed and nothing is asserted"""
    record([] if rows is None else rows, family, shape, inp, model, kernel)
    if PROBE:
        return
    assert kernel[0] <= MARGIN * model[0], f"{family} {shape} {inp}: max norm {kernel[0]:.3e} > {MARGIN} x model {model[0]:.3e}"
    assert kernel[1] <= MARGIN * model[1], f"{family} {shape} {inp}: l2 norm {kernel[1]:.3e} > {MARGIN} x model {model[1]:.3e}"
