"""Host constants and float64 tables of the pitch trackers (librosa 0.10 `yin` / `pyin`, restated).

One module for both sides: the device path (ops.pitch_yin / ops.pitch_pyin) and the float64 restatement in
tests/pitch_ref.py take every constant from here, so that floor / ceil / round of the same expressions cannot disagree
between them.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from .ops import num_frames  # noqa: F401  (the one frame-count rule, under the name callers of this module use)

TINY = float(np.finfo(np.float64).tiny)
N_THRESHOLDS = 100
BETA = (2, 18)
BOLTZMANN = 2.0
RESOLUTION = 0.1
MAX_TRANSITION_RATE = 35.92
SWITCH_PROB = 0.01
NO_TROUGH_PROB = 0.01
BINS_PER_SEMITONE = int(math.ceil(1.0 / RESOLUTION))      # 10


def note_hz(midi: int) -> float:
    """librosa.note_to_hz for a MIDI number: 440 * 2^((midi - 69) / 12)."""
    return 440.0 * 2.0 ** ((midi - 69) / 12.0)


C2 = note_hz(36)
C7 = note_hz(96)


def periods(sr: float, fmin: float, fmax: float, frame_length: int, win_length: int):
    """(min_period, max_period) of the lag search."""
    min_p = int(math.floor(sr / fmax))
    max_p = min(int(math.ceil(sr / fmin)), frame_length - win_length - 1)
    return min_p, max_p


def n_pitch_bins(fmin: float, fmax: float) -> int:
    return int(math.floor(12 * BINS_PER_SEMITONE * math.log2(fmax / fmin))) + 1


def transition_width(sr: float, hop: int) -> int:
    """round(35.92 * 12 * hop / sr) * 10 + 1 (Python's round: half to even)."""
    return int(round(MAX_TRANSITION_RATE * 12 * hop / sr)) * BINS_PER_SEMITONE + 1


def cand_stride(n_lag: int) -> int:
    """K = ceil(n_lag / 2) + 1: troughs are at least two lags apart, so a frame has at most this many."""
    return (n_lag + 1) // 2 + 1


@lru_cache(maxsize=None)
def beta_probs() -> np.ndarray:
    from scipy.stats import beta
    return np.diff(beta.cdf(np.linspace(0, 1, N_THRESHOLDS + 1), BETA[0], BETA[1]))


def thresholds() -> np.ndarray:
    return np.linspace(0, 1, N_THRESHOLDS + 1)[1:]


def boltzmann_pmf(pos, n):
    """scipy.stats.boltzmann.pmf(pos, lambda, n) = (1 - e^-l) / (1 - e^-l n) * e^(-l pos); 0 where n == 0."""
    pos = np.asarray(pos, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fact = (1 - np.exp(-BOLTZMANN)) / (1 - np.exp(-BOLTZMANN * n))
    return np.where(n > 0, fact * np.exp(-BOLTZMANN * pos), 0.0)


def no_trough_mass() -> np.ndarray:
    """[101]: no_trough_prob * sum(beta_probs[:M]), M = 0..100."""
    bp = beta_probs()
    return np.array([NO_TROUGH_PROB * np.sum(bp[:M]) for M in range(N_THRESHOLDS + 1)])


@lru_cache(maxsize=None)
def pyin_device_table(K: int) -> np.ndarray:
    """Float64 table of the frame kernel: thresholds [100], beta_probs [100], no-trough masses [101],
    Boltzmann factors (1 - e^-l) / (1 - e^-l n) for n = 0..K (0 at n = 0), then e^(-l pos) for pos = 0..K."""
    n = np.arange(K + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fact = np.where(n > 0, (1 - np.exp(-BOLTZMANN)) / (1 - np.exp(-BOLTZMANN * n)), 0.0)
    ek = np.exp(-BOLTZMANN * n)
    return np.concatenate([thresholds(), beta_probs(), no_trough_mass(), fact, ek]).astype(np.float64)


@lru_cache(maxsize=None)
def transition_local(n: int, width: int) -> np.ndarray:
    """librosa.sequence.transition_local(n, width, window='triangle', wrap=False): a triangle window of `width`
    centred on the diagonal, cut to |j - i| <= width // 2 and to the matrix, every row renormalised.  The row sum is
    math.fsum (correctly rounded, so rows with the same entries get bit-identical values wherever they sit)."""
    from scipy.signal import get_window
    win = get_window("triangle", width, fftbins=False)
    T = np.zeros((n, n), dtype=np.float64)
    lpad = (n - width) // 2
    for i in range(n):
        row = np.zeros(n, dtype=np.float64)
        if width <= n:
            row[lpad:lpad + width] = win
        else:                                    # librosa.util.pad_center cannot pad: the window is cut to n, its centre
            c0 = width // 2 - (n - 1) // 2       # at (n - 1) // 2 where pad_center puts it, so the roll lands it on i
            row[:] = win[c0:c0 + n]
        row = np.roll(row, n // 2 + i + 1)
        row[min(n, i + width // 2 + 1):] = 0
        row[:max(0, i - width // 2)] = 0
        T[i] = row
    for i in range(n):
        T[i] = T[i] / math.fsum(T[i])
    return T


def switch_matrix() -> np.ndarray:
    """librosa.sequence.transition_loop(2, 1 - switch_prob)."""
    p = 1 - SWITCH_PROB
    return np.array([[p, (1 - p) / 1], [(1 - p) / 1, p]])


@lru_cache(maxsize=None)
def transition_tables(n: int, width: int):
    """Band tables of log(kron(switch, T) + tiny) for the Viterbi kernel: ([2, R, 2h + 1] float64, R, h).
    Table row r holds source row i = r (i < h), the interior pattern (r = h), i = n - 1 - 2h + r (r > h); with
    n <= 2h + 1 every row is its own (R = n).  Column o + h is the transition i -> i + o."""
    h = width // 2
    T = transition_local(n, width)
    sw = switch_matrix()
    R = n if n <= 2 * h + 1 else 2 * h + 1
    rows = list(range(n)) if R == n else list(range(h)) + [h] + list(range(n - h, n))
    out = np.full((2, R, 2 * h + 1), math.log(TINY), dtype=np.float64)
    for b, p in enumerate((sw[0, 0], sw[0, 1])):
        for r, i in enumerate(rows):
            for o in range(-h, h + 1):
                j = i + o
                if 0 <= j < n:
                    out[b, r, o + h] = np.log(p * T[i, j] + TINY)
    if R != n:                                   # every interior row is the stored pattern
        for b, p in enumerate((sw[0, 0], sw[0, 1])):
            pat = out[b, h]
            for i in (h + 1, n // 2, n - 1 - h):
                if h <= i <= n - 1 - h:
                    vals = np.log(p * T[i, i - h:i + h + 1] + TINY)
                    assert np.array_equal(vals, pat), "transition rows are not shift-invariant"
    return out, R, h


def log_consts(n: int) -> np.ndarray:
    """{log(tiny), log(p_init voiced = 0 + tiny), log(p_init unvoiced = 1/n + tiny)}."""
    return np.array([np.log(TINY), np.log(0.0 + TINY), np.log(1.0 / n + TINY)], dtype=np.float64)
