"""Float64 NumPy restatement of PyWavelets 1.x `dwt` / `idwt` / `wavedec` / `waverec` for the Daubechies family and the
modes symmetric, reflect, periodic, constant and zero: the contract of the device wavelet transform (parity unpinned:
PyWavelets is not a dependency; tests/test_dwt_ref.py pins this file by self-checks and published known answers).

Written independently of sygnals_amd/_wavelets.py and of the kernels: the signal is extended explicitly with np.pad, a
level is one np.convolve of the extended signal followed by decimation, and the inverse is a convolution of the
zero-stuffed coefficients."""
import numpy as np
from numpy.polynomial import polynomial as npoly
from scipy.special import comb

MODES = ("symmetric", "reflect", "periodic", "constant", "zero")
WAVELETS = ("haar",) + tuple(f"db{n}" for n in range(1, 11))
_PAD = {"symmetric": "symmetric", "reflect": "reflect", "periodic": "wrap", "constant": "edge", "zero": "constant"}


def _vanishing_moments(name):
    if name == "haar":
        return 1
    if name in WAVELETS:
        return int(name[2:])
    raise ValueError(f"unknown wavelet {name!r}")


def wavelet_filters(name):
    """(dec_lo, dec_hi, rec_lo, rec_hi): the minimum-phase Daubechies scaling filter with N vanishing moments."""
    N = _vanishing_moments(name)
    # |H(w)|^2 = cos^2N(w/2) P(sin^2(w/2)); every root y of P gives the pair z, 1/z with z + 1/z = 2 - 4 y
    P = np.array([comb(N - 1 + k, k, exact=True) for k in range(N)], dtype=np.float64)
    h = npoly.polyfromroots([-1.0] * N)
    for y in (npoly.polyroots(P) if N > 1 else []):
        pair = npoly.polyroots([1.0, -(2.0 - 4.0 * y), 1.0])
        z = pair[np.argmin(np.abs(pair))]
        h = npoly.polymul(h, [-z, 1.0])
    h = np.real(h)[::-1]                      # descending powers: h[0] multiplies z^(2N-1)
    rec_lo = h * np.sqrt(2.0) / np.sum(h)
    F = rec_lo.size
    dec_lo = rec_lo[::-1].copy()
    dec_hi = np.array([(-1.0) ** (k + 1) * rec_lo[k] for k in range(F)])
    rec_hi = dec_hi[::-1].copy()
    return dec_lo, dec_hi, rec_lo, rec_hi


def dwt_coeff_len(n, filter_len):
    return (n + filter_len - 1) // 2


def dwt_max_level(n, filter_len):
    if filter_len < 2 or n < filter_len - 1:
        return 0
    return int(np.floor(np.log2(n / (filter_len - 1.0)) + 1e-12))


def extend(x, pad, mode):
    """x with `pad` samples of the mode's extension on either side."""
    x = np.asarray(x, dtype=np.float64)
    if mode not in _PAD:
        raise ValueError(f"unknown mode {mode!r}")
    if mode == "reflect" and x.size == 1:
        mode = "constant"
    return np.pad(x, pad, mode=_PAD[mode])


def dwt(x, wavelet, mode="symmetric"):
    x = np.asarray(x, dtype=np.float64)
    dec_lo, dec_hi, _, _ = wavelet_filters(wavelet)
    F = dec_lo.size
    e = extend(x, F - 1, mode)
    K = dwt_coeff_len(x.size, F)
    # full[n] = sum_j f[j] e[n - j]; sample 2 o + 1 of x is e[2 o + F]
    return np.convolve(e, dec_lo)[F::2][:K].copy(), np.convolve(e, dec_hi)[F::2][:K].copy()


def idwt(a, d, wavelet):
    a = np.asarray(a, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    if a.size != d.size:
        raise ValueError("approximation and detail lengths differ")
    _, _, rec_lo, rec_hi = wavelet_filters(wavelet)
    F = rec_lo.size
    K = a.size
    ua = np.zeros(2 * K)
    ud = np.zeros(2 * K)
    ua[::2] = a
    ud[::2] = d
    full = np.convolve(ua, rec_lo) + np.convolve(ud, rec_hi)
    return full[F - 2:2 * K].copy()


def wavedec(x, wavelet, level=None, mode="symmetric"):
    """[cA_n, cD_n, ..., cD_1]"""
    x = np.asarray(x, dtype=np.float64)
    F = wavelet_filters(wavelet)[0].size
    if level is None:
        level = max(1, dwt_max_level(x.size, F))
    out = []
    a = x
    for _ in range(level):
        a, d = dwt(a, wavelet, mode)
        out.append(d)
    return [a] + out[::-1]


def level_inputs(x, wavelet, level, mode="symmetric"):
    """[a_0 = x, a_1, ..., a_{level-1}]: the input of every level."""
    a = np.asarray(x, dtype=np.float64)
    ins = []
    for _ in range(level):
        ins.append(a)
        a = dwt(a, wavelet, mode)[0]
    return ins


def waverec(coeffs, wavelet):
    a = np.asarray(coeffs[0], dtype=np.float64)
    for d in coeffs[1:]:
        d = np.asarray(d, dtype=np.float64)
        if a.size == d.size + 1:
            a = a[:-1]
        if a.size != d.size:
            raise ValueError("coefficient shape mismatch")
        a = idwt(a, d, wavelet)
    return a
