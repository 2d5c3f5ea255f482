"""numpy f64 oracle of Spectral.lombscargle: scipy.signal.lombscargle of SciPy 1.15.3 restated line by line — its two passes, its order
of operations, its clamp at finfo(float64).epsneg — and vectorised over rows that share one time base.  tests/test_lombscargle_host.py
holds it to recorded SciPy results (tests/golden/lombscargle_vectors.json); the GPU tests hold the kernels to it.  Never imported by
the product."""
import numpy as np

NORMALIZES = (False, True, "power", "normalize", "amplitude")
# the 24 option combinations of the tests: precenter x floating_mean x weights x the three normalisations
COMBOS = [(pre, fm, wts, norm) for pre in (False, True) for fm in (False, True) for wts in (False, True)
          for norm in ("power", "normalize", "amplitude")]


def combo_name(pre, fm, wts, norm):
    return f"{norm}{'_pre' if pre else ''}{'_fm' if fm else ''}{'_w' if wts else ''}"


def lombscargle(x, y, freqs, precenter=False, normalize=False, weights=None, floating_mean=False, parts=False):
    """pgram [..., F] of the rows y [..., n] (f64, or c128 under "amplitude"); with parts=True also the shifted CC and SS (F,) ahead of
    the clamp, which tell where the result is conditioned."""
    x = np.asarray(x, np.float64)
    y = np.array(y, np.float64)
    freqs = np.asarray(freqs, np.float64)
    weights = np.ones(x.shape, np.float64) if weights is None else np.array(weights, np.float64)
    if not (x.ndim == 1 and x.size > 0 and y.ndim >= 1 and y.shape[-1] == x.shape[0] and weights.shape == x.shape):
        raise ValueError("Parameters x, y, weights must be 1-D arrays of equal non-zero length!")
    if not (freqs.ndim == 1 and freqs.size > 0):
        raise ValueError("Parameter freqs must be a 1-D array of non-zero length!")
    if not (np.all(weights >= 0) and np.sum(weights) > 0):
        raise ValueError("Parameter weights must have only non-negative entries which sum to a positive value!")
    if isinstance(normalize, (bool, np.bool_)):
        normalize = "normalize" if normalize else "power"
    if normalize not in ("power", "normalize", "amplitude"):
        raise ValueError("Normalize must be: False (or 'power'), True (or 'normalize'), or 'amplitude'.")
    lead = y.shape[:-1]
    y = y.reshape(-1, x.shape[0]).T.copy()    # (n, R): a column per row
    weights *= 1.0 / weights.sum()
    if precenter:
        y -= y.mean(axis=0)
    freqs = freqs.reshape(1, -1)
    x = x.reshape(-1, 1)
    weights = weights.reshape(-1, 1)
    weights_y = weights * y                   # (n, R)
    freqst = freqs * x
    coswt = np.cos(freqst)
    sinwt = np.sin(freqst)
    with np.errstate(all="ignore"):
        Y = np.dot(weights.T, y).reshape(-1, 1)        # (R, 1)
        CC = np.dot(weights.T, coswt * coswt)
        SS = 1.0 - CC
        CS = np.dot(weights.T, coswt * sinwt)
        if floating_mean:
            C = np.dot(weights.T, coswt)
            S = np.dot(weights.T, sinwt)
            CC -= C * C
            SS -= S * S
            CS -= C * S
        tau = 0.5 * np.arctan2(2.0 * CS, CC - SS)
        freqst_tau = freqst - tau
        coswt_tau = np.cos(freqst_tau)
        sinwt_tau = np.sin(freqst_tau)
        YC = np.dot(weights_y.T, coswt_tau)   # (R, F)
        YS = np.dot(weights_y.T, sinwt_tau)
        CC = np.dot(weights.T, coswt_tau * coswt_tau)
        SS = 1.0 - CC
        if floating_mean:
            C = np.dot(weights.T, coswt_tau)
            S = np.dot(weights.T, sinwt_tau)
            YC -= Y * C
            YS -= Y * S
            CC -= C * C
            SS -= S * S
        cc_shifted, ss_shifted = CC[0].copy(), SS[0].copy()
        epsneg = np.finfo(np.float64).epsneg
        CC[CC < epsneg] = epsneg
        SS[SS < epsneg] = epsneg
        a = YC / CC
        b = YS / SS
        pgram = 2.0 * (a * YC + b * YS)
        if normalize == "power":
            pgram *= float(x.shape[0]) / 4.0
        elif normalize == "normalize":
            YY = np.sum(weights_y * y, axis=0).reshape(-1, 1)
            if floating_mean:
                YY -= Y * Y
            pgram *= 0.5 / YY
        else:
            pgram = (a + 1j * b) * np.exp(1j * tau)
    pgram = pgram.reshape(lead + (freqs.shape[1],))
    return (pgram, cc_shifted, ss_shifted) if parts else pgram


def row_error(got, want):
    """largest |got - want| of each row over the row's largest |want| (1 where that is 0); NaN where exactly one of the two is NaN"""
    got, want = np.asarray(got), np.asarray(want)
    both = np.isnan(got) & np.isnan(want)
    diff = np.where(both, 0.0, np.abs(got - want))
    scale = np.max(np.where(np.isnan(want), 0.0, np.abs(want)), axis=-1, keepdims=True)
    return np.max(diff / np.where(scale > 0, scale, 1.0), axis=-1)


def parity_inputs():
    """the seeded inputs of the parity tests: times uniform in [0, 100), 96 angular frequencies in (0.01, 20), weights in [0.25, 2) and
    three rows of 257 samples (a sinusoid of angular frequency 1.25 in noise, offset 1.5), as f64"""
    rng = np.random.Generator(np.random.PCG64(2024))
    x = rng.uniform(0.0, 100.0, 257)
    freqs = np.sort(rng.uniform(0.01, 20.0, 96))
    weights = rng.uniform(0.25, 2.0, 257)
    y = 1.5 + rng.standard_normal((3, 257)) + np.sin(1.25 * x)
    return x, y, freqs, weights


def conditioned(cc, ss, floor=1e-3):
    """where "amplitude" is compared: the oracle's shifted CC and SS both at least `floor`"""
    return (np.asarray(cc) >= floor) & (np.asarray(ss) >= floor)
