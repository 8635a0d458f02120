"""Host rules of the loudness meter (csrc/loudness.hip; include/sygnals_hip.h states the entry points): the K-weighting
design of ITU-R BS.1770 per sample rate, the segment arithmetic, the channel weights and the true-peak oversampling tier.
Pure NumPy, float64 throughout.  No device and no library here, so the rules are tested on the CPU."""
from __future__ import annotations

import functools
from math import pi, tan

import numpy as np

FS_MIN, FS_MAX = 8000, 384000            # served rates (the library's SYG_LOUDNESS_FS_MIN / _MAX; tests hold them equal)
MOMENTARY, SHORT_TERM = 4, 30            # 100 ms segments of a 400 ms and of a 3 s block
ABSOLUTE_GATE = -70.0                    # LUFS
OFFSET = -0.691                          # l = OFFSET + 10 log10 z

# the analogue prototype BS.1770's 48 kHz table is the bilinear image of; redesigned per rate through K = tan(pi f0 / fs)
SHELF_F0, SHELF_GAIN_DB, SHELF_Q, SHELF_VB_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773

SURROUND_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)    # L R C Ls Rs


def check_fs(fs, who: str = "loudness") -> int:
    """fs as an int; a rate that is not served raises ValueError naming what is."""
    try:
        ok = not isinstance(fs, bool) and float(fs) == int(fs) and FS_MIN <= int(fs) <= FS_MAX
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        low = ""
        try:
            if 0 < float(fs) < FS_MIN:
                low = " (resample first: a 100 ms segment must span more than one 256-sample chunk)"
        except (TypeError, ValueError, OverflowError):
            pass
        raise ValueError(f"{who}: fs={fs!r} is not served; served: integer sampling rates from {FS_MIN} to {FS_MAX} Hz{low}")
    return int(fs)


@functools.lru_cache(maxsize=64)
def _k_weighting(fs: int) -> np.ndarray:
    K = tan(pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = [(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]
    K = tan(pi * HIGHPASS_F0 / fs)
    a0 = 1.0 + K / HIGHPASS_Q + K * K
    highpass = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HIGHPASS_Q + K * K) / a0]
    sos = np.array([shelf, highpass], dtype=np.float64)
    sos.setflags(write=False)
    return sos


def k_weighting_sos(fs) -> np.ndarray:
    """The K-weighting cascade at fs as scipy's sos [2, 6] (shelf, then high-pass), float64 (the caller's own copy)."""
    return _k_weighting(check_fs(fs, "k_weighting_sos")).copy()


def segment_start(j, fs: int):
    """s_j = j fs div 10: first sample of 100 ms segment j (j an int or an integer array)."""
    return (np.asarray(j, dtype=np.int64) * int(fs)) // 10 if isinstance(j, np.ndarray) else (int(j) * int(fs)) // 10


def n_segments(L: int, fs: int) -> int:
    """Whole segments of a row of L samples, 10 L div fs."""
    return (int(L) * 10) // int(fs)


def n_blocks(L: int, fs: int, segments: int) -> int:
    """Blocks of `segments` segments (MOMENTARY or SHORT_TERM) that a row of L samples holds."""
    return max(0, n_segments(L, fs) - (segments - 1))


def channel_weights(C: int, weights=None) -> np.ndarray:
    """The channel weights G_c [C] float64: ones for C <= 3, BS.1770's L R C Ls Rs for C = 5, else `weights`."""
    if weights is None:
        if C <= 3:
            return np.ones(C, dtype=np.float64)
        if C == 5:
            return np.array(SURROUND_WEIGHTS, dtype=np.float64)
        raise ValueError(f"loudness: {C} channels have no default weights (1 to 3 channels weigh 1, 5 channels are "
                         f"L R C Ls Rs = {list(SURROUND_WEIGHTS)}); pass channel_weights")
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (C,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError(f"loudness: channel_weights must be {C} finite non-negative numbers, one per channel")
    return np.ascontiguousarray(w)


def true_peak_up(fs: int) -> int:
    """Oversampling factor of the true-peak estimate: 4 below 96 kHz, 2 below 192 kHz, 1 (the sample peak) from there."""
    return 4 if fs < 96000 else (2 if fs < 192000 else 1)


def lra_ranks(n: int):
    """EBU Tech 3342's nearest ranks among n ascending values, floor((n - 1) p + 1/2) at p = 0.10 and 0.95, in integers."""
    return ((n - 1) + 5) // 10, ((n - 1) * 19 + 10) // 20
