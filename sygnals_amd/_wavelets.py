"""Host tables of the discrete wavelet transform: Daubechies filter banks, coefficient lengths, levels and modes.

The filters are computed in float64 by spectral factorisation (Daubechies 1988): the roots y of
P(y) = sum_{k<N} C(N-1+k, k) y^k, for each the root of z^2 - (2 - 4y) z + 1 inside the unit circle, and
h = poly([-1] * N + those roots) scaled to sum sqrt(2).  That h is PyWavelets' `rec_lo`; the other three follow from it.
Other families (symlets, coiflets, biorthogonal) need PyWavelets' own tables and are refused rather than guessed.
"""
from __future__ import annotations

import functools
import math
import warnings

import numpy as np

WAVELETS = ("haar",) + tuple(f"db{n}" for n in range(1, 11))
# name -> SYG_DWT_* of include/sygnals_hip.h
MODES = {"zero": 0, "constant": 1, "symmetric": 2, "reflect": 3, "periodic": 4}
MODE_NAMES = ("symmetric", "reflect", "periodic", "constant", "zero")


def _order(wavelet) -> int:
    if isinstance(wavelet, str):
        name = wavelet.lower()
        if name == "haar":
            return 1
        if name in WAVELETS:
            return int(name[2:])
    raise ValueError(f"Unknown wavelet {wavelet!r}: the wavelets served are {', '.join(WAVELETS)}")


@functools.lru_cache(maxsize=None)
def _rec_lo(N: int) -> np.ndarray:
    if N == 1:
        h = np.array([1.0, 1.0])
    else:
        P = [math.comb(N - 1 + k, k) for k in range(N)]            # ascending powers of y
        zs = []
        for y in np.roots(P[::-1]):
            b = 2.0 - 4.0 * y
            s = np.sqrt(b * b - 4.0 + 0j)
            z1, z2 = (b + s) / 2.0, (b - s) / 2.0
            zs.append(z1 if abs(z1) < abs(z2) else z2)
        h = np.real(np.poly([-1.0] * N + zs))
    h = h * (math.sqrt(2.0) / h.sum())
    h.setflags(write=False)
    return h


def filters(wavelet):
    """(dec_lo, dec_hi, rec_lo, rec_hi) float64, PyWavelets' conventions."""
    rec_lo = _rec_lo(_order(wavelet))
    F = rec_lo.size
    dec_lo = rec_lo[::-1].copy()
    dec_hi = rec_lo * np.where(np.arange(F) % 2 == 0, -1.0, 1.0)      # (-1)^(k + 1) rec_lo[k]
    rec_hi = dec_hi[::-1].copy()
    return dec_lo, dec_hi, rec_lo.copy(), rec_hi


def filter_length(wavelet) -> int:
    return 2 * _order(wavelet)


def mode_code(mode) -> int:
    if isinstance(mode, str) and mode in MODES:
        return MODES[mode]
    raise ValueError(f"Unsupported signal extension mode {mode!r}: the modes served are {', '.join(MODE_NAMES)}")


def dwt_coeff_len(n: int, filter_len: int) -> int:
    return (int(n) + int(filter_len) - 1) // 2


def dwt_max_level(n: int, filter_len: int) -> int:
    """floor(log2(n / (filter_len - 1))), 0 when n < filter_len - 1 (pywt.dwt_max_level)."""
    n, f = int(n), int(filter_len) - 1
    if f < 1 or n < f:
        return 0
    level = 0
    while (f << (level + 1)) <= n:
        level += 1
    return level


def resolve_level(n: int, filter_len: int, level) -> int:
    """`level=None` -> max(1, maximum); a level below 1 or not an integer raises; one above the maximum warns."""
    mx = dwt_max_level(n, filter_len)
    if level is None:
        return max(1, mx)
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 1:
        raise ValueError(f"Decomposition level must be an integer >= 1, got {level}.")
    if level > mx:
        warnings.warn(f"Level value of {level} is too high: all coefficients will experience boundary effects.",
                      UserWarning, stacklevel=3)
    return int(level)


def wavedec_lengths(n: int, filter_len: int, level: int):
    """[len(cA_n), len(cD_n), ..., len(cD_1)]."""
    lens = []
    for _ in range(level):
        n = dwt_coeff_len(n, filter_len)
        lens.append(n)
    return [lens[-1]] + lens[::-1]


def waverec_length(lens, filter_len: int) -> int:
    """Output length of waverec for coefficient lengths [a_n, d_n, ..., d_1]; ValueError where pywt refuses them."""
    lens = [int(v) for v in lens]
    if len(lens) < 2:
        raise ValueError("Coefficient list too short (minimum 2 arrays required).")
    a = lens[0]
    for i, d in enumerate(lens[1:]):
        if a == d + 1:
            a = d
        if a != d:
            raise ValueError(f"coefficient shape mismatch at level {i}: approximation {a}, detail {d}")
        if d < filter_len // 2:
            raise ValueError(f"level {i} has {d} coefficients, fewer than half the filter length ({filter_len // 2})")
        a = 2 * d - filter_len + 2
    return a
