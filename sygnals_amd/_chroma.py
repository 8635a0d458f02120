"""Host side of the tonal family (chroma, CENS, tonnetz, tuning): the tables the kernels of chroma.hip read and the argument
rules, judged without a device.  Everything here is float64 NumPy after librosa 0.10's filters.chroma / cq_to_chroma /
tonnetz / chroma_cens / pitch_tuning; the kernels get the tables rounded once to float32."""
from __future__ import annotations

import numpy as np
import scipy.signal

NC_MAX = 36                             # SYG_CHROMA_NC_MAX
CENS_WIN_MAX = 257                      # SYG_CHROMA_CENS_WIN_MAX (win_len_smooth + 2)
HIST_BINS_MAX = 1024                    # SYG_CHROMA_HIST_BINS_MAX
MAX_ELEMS = 1 << 31                     # SYG_CHROMA_MAX_ELEMS
NORMS = {None: 0, "inf": 1, 1: 2, 2: 3}            # the codes of syg_chroma_fold_*_f32

SERVED = "served: 1 <= n_chroma <= 36; norm inf, 1, 2 or None; any n_fft >= 2 with zero padding; the full CQT " \
         "(cqt_mode='full') with bins_per_octave a multiple of n_chroma; win_len_smooth None or 1 .. 255; ref=None in piptrack"


def c1_hz() -> float:
    """librosa.note_to_hz('C1')."""
    return 440.0 * 2.0 ** ((24 - 69) / 12.0)


def hz_to_octs(f, tuning: float = 0.0, bins_per_octave: int = 12):
    a440 = 440.0 * 2.0 ** (float(tuning) / bins_per_octave)
    return np.log2(np.asarray(f, dtype=np.float64) / (a440 / 16.0))


def hz_to_midi(f):
    return 12.0 * (np.log2(np.asarray(f, dtype=np.float64)) - np.log2(440.0)) + 69.0


def check_n_chroma(n_chroma, who: str) -> int:
    if not isinstance(n_chroma, (int, np.integer)) or isinstance(n_chroma, bool) or not 1 <= n_chroma <= NC_MAX:
        raise ValueError(f"{who}: n_chroma={n_chroma!r} is outside 1 .. {NC_MAX} ({SERVED})")
    return int(n_chroma)


def check_norm(norm, who: str) -> int:
    """The kernel's code: 0 none, 1 inf, 2 L1, 3 L2."""
    if norm is None:
        return 0
    if isinstance(norm, (int, float, np.integer, np.floating)) and not isinstance(norm, bool):
        if norm == np.inf:
            return 1
        if norm in (1, 2):
            return 1 + int(norm)
    raise ValueError(f"{who}: norm={norm!r} is not served ({SERVED})")


def check_threshold(threshold, who: str):
    """(has_threshold, value)."""
    if threshold is None:
        return 0, 0.0
    if isinstance(threshold, (int, float, np.integer, np.floating)) and not isinstance(threshold, bool) and np.isfinite(threshold):
        return 1, float(threshold)
    raise ValueError(f"{who}: threshold={threshold!r} must be None or a finite number")


def check_tuning(tuning, who: str) -> float:
    if isinstance(tuning, (int, float, np.integer, np.floating)) and not isinstance(tuning, bool) and np.isfinite(tuning):
        return float(tuning)
    raise ValueError(f"{who}: tuning={tuning!r} must be a finite number (or None: estimated per clip)")


def check_n_fft(n_fft, who: str) -> int:
    if not isinstance(n_fft, (int, np.integer)) or isinstance(n_fft, bool) or n_fft < 2:
        raise ValueError(f"{who}: n_fft={n_fft!r} must be an integer >= 2 ({SERVED})")
    return int(n_fft)


def check_pad_mode(pad_mode, who: str) -> None:
    if pad_mode not in ("constant", "zeros"):
        raise ValueError(f"{who}: pad_mode={pad_mode!r} is not served: the device STFT pads with zeros ({SERVED})")


def check_merge(bins_per_octave, n_chroma: int, who: str) -> int:
    if not isinstance(bins_per_octave, (int, np.integer)) or isinstance(bins_per_octave, bool) or bins_per_octave < 1:
        raise ValueError(f"{who}: bins_per_octave={bins_per_octave!r} must be a positive integer")
    if bins_per_octave % n_chroma:
        raise ValueError(f"{who}: incompatible CQ merge: input bins must be an integer multiple of output bins "
                         f"(bins_per_octave={bins_per_octave}, n_chroma={n_chroma}; {SERVED})")
    return int(bins_per_octave)


def check_cqt_mode(cqt_mode, who: str) -> None:
    if cqt_mode != "full":
        raise ValueError(f"{who}: cqt_mode={cqt_mode!r} is not served ({SERVED})")


def chroma_filterbank(sr, n_fft: int, n_chroma: int = 12, tuning: float = 0.0, ctroct: float = 5.0, octwidth=2, norm=2,
                      base_c: bool = True) -> np.ndarray:
    """librosa.filters.chroma in float64, rounded once: float32 [n_chroma, 1 + n_fft // 2]."""
    fr = np.linspace(0, float(sr), n_fft, endpoint=False)[1:]
    fb = n_chroma * hz_to_octs(fr, tuning, n_chroma)
    fb = np.concatenate(([fb[0] - 1.5 * n_chroma], fb))
    bw = np.concatenate((np.maximum(fb[1:] - fb[:-1], 1.0), [1.0]))
    D = np.subtract.outer(fb, np.arange(0, n_chroma, dtype=np.float64)).T
    n2 = np.round(float(n_chroma) / 2)
    D = np.remainder(D + n2 + 10 * n_chroma, n_chroma) - n2
    w = np.exp(-0.5 * (2 * D / bw[None, :]) ** 2)
    w = normalize(w, norm, axis=0)
    if octwidth is not None:
        w = w * np.exp(-0.5 * (((fb / n_chroma - ctroct) / octwidth) ** 2))[None, :]
    if base_c:
        w = np.roll(w, -3 * (n_chroma // 12), axis=0)
    return np.ascontiguousarray(w[:, :1 + n_fft // 2]).astype(np.float32)


def normalize(x, norm, axis=0):
    """librosa.util.normalize in float64 (norm inf, 1, 2 or None)."""
    x = np.asarray(x, dtype=np.float64)
    if norm is None:
        return x
    mag = np.abs(x)
    if norm == np.inf:
        length = mag.max(axis=axis, keepdims=True)
    elif norm == 1:
        length = mag.sum(axis=axis, keepdims=True)
    elif norm == 2:
        length = np.sqrt((mag ** 2).sum(axis=axis, keepdims=True))
    else:
        raise ValueError(f"norm={norm!r} is not served ({SERVED})")
    length = np.where(length < float(np.finfo(np.float32).tiny), 1.0, length)
    return x / length


def cq_to_chroma(n_input: int, bins_per_octave: int = 12, n_chroma: int = 12, fmin=None, window=None,
                 base_c: bool = True) -> np.ndarray:
    """librosa.filters.cq_to_chroma: float32 [n_chroma, n_input]."""
    m = check_merge(bins_per_octave, n_chroma, "cq_to_chroma") // n_chroma
    fmin = c1_hz() if fmin is None else float(fmin)
    w = np.repeat(np.eye(n_chroma), m, axis=1)
    w = np.roll(w, -(m // 2), axis=1)
    w = np.tile(w, int(np.ceil(float(n_input) / bins_per_octave)))[:, :n_input]
    midi0 = np.mod(hz_to_midi(fmin), 12)
    roll = midi0 if base_c else midi0 - 9
    w = np.roll(w, int(np.round(roll * (n_chroma / 12.0))), axis=0)
    if window is not None:
        w = scipy.signal.convolve(w, np.atleast_2d(np.asarray(window, dtype=np.float64)), mode="same")
    return np.ascontiguousarray(w).astype(np.float32)


def tonnetz_phi(n_chroma: int = 12) -> np.ndarray:
    """The tonnetz transform: float32 [6, n_chroma]."""
    dim = np.linspace(0, 12, num=n_chroma, endpoint=False)
    V = np.multiply.outer(np.array([7.0 / 6, 7.0 / 6, 3.0 / 2, 3.0 / 2, 2.0 / 3, 2.0 / 3]), dim)
    V[::2] -= 0.5
    return (np.array([1, 1, 1, 1, 0.5, 0.5])[:, None] * np.cos(np.pi * V)).astype(np.float32)


def check_win_len_smooth(win_len_smooth, who: str) -> int:
    """0: no smoothing."""
    if win_len_smooth is None:
        return 0
    if not isinstance(win_len_smooth, (int, np.integer)) or isinstance(win_len_smooth, bool) or \
            not 0 <= win_len_smooth <= CENS_WIN_MAX - 2:
        raise ValueError(f"{who}: win_len_smooth={win_len_smooth!r} must be None or an integer in 1 .. {CENS_WIN_MAX - 2} ({SERVED})")
    return int(win_len_smooth)


def cens_window(win_len_smooth, smoothing_window="hann"):
    """(taps float32 [n], left): out[t] = sum_j taps[j] q[t - left + j] is scipy.ndimage.convolve(q, win, mode="constant") with
    win = get_window(smoothing_window, win_len_smooth + 2, fftbins=False) / its sum.  No smoothing: ([1], 0)."""
    if not win_len_smooth:
        return np.ones(1, dtype=np.float32), 0
    n = int(win_len_smooth) + 2
    win = scipy.signal.get_window(smoothing_window, n, fftbins=False).astype(np.float64)
    win = win / win.sum()
    # ndimage.convolve: out[t] = sum_i win[i] q[t + n // 2 - i]; with j = n - 1 - i the taps are win reversed and
    # left = n - 1 - n // 2
    return np.ascontiguousarray(win[::-1]).astype(np.float32), n - 1 - n // 2


def check_resolution(resolution, who: str) -> int:
    """Bins of the tuning histogram."""
    if not (isinstance(resolution, (float, np.floating)) and 0 < resolution < 1):
        raise ValueError(f"{who}: resolution={resolution!r} must be a float in (0, 1)")
    n = int(np.ceil(1.0 / resolution))
    if n > HIST_BINS_MAX:
        raise ValueError(f"{who}: resolution={resolution!r} asks for {n} histogram bins, above {HIST_BINS_MAX}")
    return n


def tuning_bins(resolution: float = 0.01) -> np.ndarray:
    """pitch_tuning's bin edges: float64 [ceil(1 / resolution) + 1]."""
    return np.linspace(-0.5, 0.5, int(np.ceil(1.0 / resolution)) + 1)


def pip_bins(sr, n_fft: int, fmin: float = 150.0, fmax: float = 4000.0):
    """piptrack's admissible bins [k_lo, k_hi): fmin <= rfftfreq[k] < min(fmax, sr / 2)."""
    if not sr > 0:
        raise ValueError("piptrack: sr must be positive")
    fmin = max(float(fmin), 0.0)
    fmax = min(float(fmax), float(sr) / 2)
    f = np.fft.rfftfreq(n_fft, 1.0 / float(sr))
    ok = np.nonzero((fmin <= f) & (f < fmax))[0]
    if len(ok) == 0:
        return 0, 0
    return int(ok[0]), int(ok[-1]) + 1


def check_pip(threshold, ref, who: str) -> float:
    if ref is not None:
        raise ValueError(f"{who}: ref={ref!r} is not served: the reference is threshold * max over the frame ({SERVED})")
    if not (isinstance(threshold, (int, float, np.integer, np.floating)) and not isinstance(threshold, bool) and
            np.isfinite(threshold) and threshold >= 0):
        raise ValueError(f"{who}: threshold={threshold!r} must be a finite number >= 0")
    return float(threshold)


def pitch_tuning(frequencies, resolution: float = 0.01, bins_per_octave: int = 12) -> float:
    """librosa.pitch_tuning on the host (float64): the left edge of the first fullest bin of the residuals."""
    import warnings
    n = check_resolution(resolution, "pitch_tuning")
    f = np.atleast_1d(np.asarray(frequencies, dtype=np.float64))
    f = f[f > 0]
    if not f.any():
        warnings.warn("Trying to estimate tuning from empty frequency set.", stacklevel=2)
        return 0.0
    r = np.mod(bins_per_octave * hz_to_octs(f), 1.0)
    r[r >= 0.5] -= 1.0
    edges = np.linspace(-0.5, 0.5, n + 1)
    counts, _ = np.histogram(r, edges)
    return float(edges[np.argmax(counts)])
