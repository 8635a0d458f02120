"""Host side of the rhythm family (tempogram, tempo, beat tracking): the tables the kernels of beat.hip read and the argument
rules, judged without a device.  Everything here is float64 NumPy; the kernels get the tables as they stand."""
from __future__ import annotations

import numpy as np
import scipy.signal

WIN_MIN, WIN_MAX = 2, 2048              # SYG_BEAT_WIN_MAX
PERIOD_MAX = 2047                       # SYG_BEAT_PERIOD_MAX
LOG_TABLE = 4096                        # SYG_BEAT_LOG_TABLE
MAX_ELEMS = 1 << 31                     # SYG_BEAT_MAX_ELEMS

SERVED = "served: the autocorrelation tempogram with norm inf / None, win_length 2 .. 2048; tempo with aggregate mean / None " \
         "and the log-normal prior of start_bpm / std_bpm / max_tempo; beat_track with a constant tempo, tightness > 0, bpm > 0"


def log_table() -> np.ndarray:
    """log of 1 .. LOG_TABLE: the one table host and device take the transition costs from."""
    return np.log(np.arange(1, LOG_TABLE + 1, dtype=np.float64))


def window_table(window, win_length: int) -> np.ndarray:
    """scipy's periodic window in float64, rounded once to float32."""
    return scipy.signal.get_window(window, win_length, fftbins=True).astype(np.float64).astype(np.float32)


def check_win_length(win_length, who: str) -> int:
    if not isinstance(win_length, (int, np.integer)) or isinstance(win_length, bool) or not WIN_MIN <= win_length <= WIN_MAX:
        raise ValueError(f"{who}: win_length={win_length!r} is outside {WIN_MIN} .. {WIN_MAX} ({SERVED})")
    return int(win_length)


def check_norm(norm, who: str) -> int:
    """0: none, 1: inf."""
    if norm is None:
        return 0
    if isinstance(norm, (int, float, np.floating)) and norm == np.inf:
        return 1
    raise ValueError(f"{who}: norm={norm!r} is not served ({SERVED})")


def check_aggregate(aggregate, who: str) -> bool:
    """True: the mean over frames; False: one value per frame."""
    if aggregate is None:
        return False
    if aggregate is np.mean or aggregate == "mean":
        return True
    raise ValueError(f"{who}: aggregate={aggregate!r} is not served ({SERVED})")


def check_frames(T: int, win_length: int, center: bool, who: str) -> int:
    n = T if center else T - win_length + 1
    if T < 1 or n <= 0:
        raise ValueError(f"{who}: {T} frames are fewer than win_length={win_length} without centering")
    return n


def check_size(B: int, win_length: int, n: int, who: str) -> None:
    if B * win_length * n > MAX_ELEMS:
        raise ValueError(f"{who}: the result [{B}, {win_length}, {n}] has more than 2^31 elements; call it on fewer rows")


def tempo_win_length(ac_size: float, sr: float, hop_length: int, who: str) -> int:
    if not (sr > 0 and hop_length >= 1 and ac_size > 0):
        raise ValueError(f"{who}: sr, hop_length and ac_size must be positive")
    return check_win_length(int(np.floor(ac_size * sr / hop_length)), who)


def tempo_prior(win_length: int, sr: float, hop_length: int = 512, start_bpm: float = 120.0, std_bpm: float = 1.0,
                max_tempo=320.0):
    """(bpms, logprior), float64 [win_length]: bpms[0] = inf, bpms[k] = 60 sr / (hop k); the log-normal prior around
    start_bpm, -inf for the lags faster than max_tempo."""
    if not (start_bpm > 0 and np.isfinite(start_bpm)):
        raise ValueError("tempo: start_bpm must be strictly positive")
    if not (std_bpm > 0 and np.isfinite(std_bpm)):
        raise ValueError("tempo: std_bpm must be strictly positive")
    if max_tempo is not None and not max_tempo > 0:
        raise ValueError("tempo: max_tempo must be strictly positive or None")
    bpms = np.full(win_length, np.inf)
    bpms[1:] = 60.0 * sr / (hop_length * np.arange(1.0, win_length))
    with np.errstate(divide="ignore", invalid="ignore"):
        logprior = -0.5 * ((np.log2(bpms) - np.log2(float(start_bpm))) / float(std_bpm)) ** 2
    if max_tempo is not None:
        logprior[:int(np.argmax(bpms < max_tempo))] = -np.inf
    return bpms, logprior


def check_tightness(tightness, who: str) -> float:
    if not (isinstance(tightness, (int, float, np.integer, np.floating)) and np.isfinite(tightness) and tightness > 0):
        raise ValueError(f"{who}: tightness={tightness!r} must be strictly positive ({SERVED})")
    return float(tightness)


def periods_from_bpm(bpm, B: int, sr: float, hop_length: int, who: str) -> np.ndarray:
    """int32 [B]: round(60 fps / bpm), half to even, of a scalar or of one value per row."""
    v = np.asarray(bpm, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(B, float(v))
    if v.shape != (B,):
        raise ValueError(f"{who}: bpm must be a scalar or {B} values, one per row")
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError(f"{who}: bpm must be strictly positive ({SERVED})")
    p = np.round(60.0 * (float(sr) / hop_length) / v)
    if (p < 2).any():
        raise ValueError(f"{who}: bpm={float(v[np.argmin(p)])} gives a beat period below 2 frames at {sr} Hz / hop {hop_length}: "
                         "the search window would reach offset 0")
    if (p > PERIOD_MAX).any():
        raise ValueError(f"{who}: bpm={float(v[np.argmax(p)])} gives a beat period above {PERIOD_MAX} frames")
    return p.astype(np.int32)


def check_periods(period, B: int, who: str) -> np.ndarray:
    p = np.asarray(period)
    if p.ndim == 0:
        p = np.full(B, p)
    if p.shape != (B,) or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"{who}: period must be an integer or {B} integers, one per row")
    if (p > PERIOD_MAX).any() or (p < 0).any():
        raise ValueError(f"{who}: a period is outside 0 .. {PERIOD_MAX} frames")
    return p.astype(np.int32)
