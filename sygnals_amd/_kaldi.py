"""Host side of the Kaldi-compatible front end (csrc/kaldi_front.hip): the sizes and frame-count rules, the argument
checks, and the float64 tables (window, HTK mel banks, DCT x lifter), rounded to float32 once and cached.

The definition is torchaudio.compliance.kaldi.fbank / mfcc (Kaldi's feature-window.cc / mel-computations.cc), restated in
tests/kaldi_ref.py, which is the contract and takes its sizes, frame counts and eps from here, so that int() / floor of
the same expression cannot disagree between the two sides.  No device is needed here."""
from __future__ import annotations

import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

from . import _tables as T

EPS = float(np.finfo(np.float32).eps)                 # 1.1920929e-07: the floor of every logarithm
LOG_EPS = float(np.float32(math.log(EPS)))            # the float32 nearest to log(eps): what a floor cell holds
N_SERVED = (256, 512, 1024, 2048)
MEL_MIN, MEL_MAX = 3, 256
WINDOWS = ("hamming", "hanning", "povey", "rectangular", "blackman")
LAYOUTS = ("ct", "tc")
SERVED = ("served: a frame_length whose next power of two is 256, 512, 1024 or 2048 samples (8 ... 48 kHz at 25 ms), "
          "frame_shift of at least one sample, 3 <= num_mel_bins <= 256, 1 <= num_ceps <= num_mel_bins, window_type "
          "hamming, hanning, povey, rectangular or blackman, round_to_power_of_two=True, vtln_warp=1.0")

# torchaudio's keywords and defaults (fbank; mfcc has no use_log_fbank / use_power and adds the last two)
_COMMON = dict(blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0,
               htk_compat=False, low_freq=20.0, min_duration=0.0, num_mel_bins=23, preemphasis_coefficient=0.97,
               raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True, snip_edges=True, subtract_mean=False,
               use_energy=False, vtln_high=-500.0, vtln_low=100.0, vtln_warp=1.0, window_type="povey")
FBANK_DEFAULTS = dict(_COMMON, use_log_fbank=True, use_power=True)
MFCC_DEFAULTS = dict(_COMMON, cepstral_lifter=22.0, num_ceps=13)

Spec = namedtuple("Spec", "mfcc sr wl hop N M low high window_type blackman_coeff preemph remove_dc raw_energy use_power "
                          "use_log use_energy htk_compat energy_floor dither snip_edges subtract_mean min_duration num_ceps "
                          "lifter C")


def sizes(sr: float, frame_length: float = 25.0, frame_shift: float = 10.0):
    """(wl, hop, N): window and shift in samples (torchaudio's int(sr ms 0.001)) and the next power of two >= wl."""
    wl = int(sr * frame_length * 0.001)
    hop = int(sr * frame_shift * 0.001)
    N = 1
    while N < wl:
        N *= 2
    return wl, hop, N


def num_frames(L: int, wl: int, hop: int, snip_edges: bool = True) -> int:
    if snip_edges:
        return 0 if L < wl else 1 + (L - wl) // hop
    return (L + hop // 2) // hop


def frame_start(t, wl: int, hop: int, snip_edges: bool = True):
    return t * hop if snip_edges else t * hop + hop // 2 - wl // 2


def reflect_index(s, L: int):
    """Kaldi's reflection of indices outside [0, L) (s <- -s - 1 or 2 L - 1 - s until inside), in closed form."""
    r = np.mod(np.asarray(s, dtype=np.int64), 2 * L)
    return np.where(r < L, r, 2 * L - 1 - r)


def _real(who, name, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
        raise ValueError(f"{who}: {name} must be a finite real number (got {v!r})")
    return float(v)


def _flag(who, name, v) -> bool:
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{who}: {name} must be True or False (got {v!r})")
    return bool(v)


def _int(who, name, v) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{who}: {name} must be an integer (got {v!r}; {SERVED})")
    return int(v)


def check(who: str, mfcc: bool, sr, kw: dict) -> Spec:
    """The call's parameters, checked: torchaudio's keywords over its defaults.  Everything outside what is served is a
    ValueError that says what is served."""
    defaults = MFCC_DEFAULTS if mfcc else FBANK_DEFAULTS
    unknown = sorted(set(kw) - set(defaults))
    if unknown:
        raise ValueError(f"{who}: unknown arguments {unknown} (torchaudio's keywords: {sorted(defaults)})")
    p = dict(defaults, **kw)
    sr = _real(who, "sample_frequency", sr)
    if not sr > 0:
        raise ValueError(f"{who}: sample_frequency must be positive (got {sr!r})")
    if not _flag(who, "round_to_power_of_two", p["round_to_power_of_two"]):
        raise ValueError(f"{who}: round_to_power_of_two=False is not served ({SERVED})")
    if _real(who, "vtln_warp", p["vtln_warp"]) != 1.0:
        raise ValueError(f"{who}: vtln_warp = {p['vtln_warp']!r} is not served ({SERVED})")
    fl, fs = _real(who, "frame_length", p["frame_length"]), _real(who, "frame_shift", p["frame_shift"])
    wl, hop, N = sizes(sr, fl, fs)
    if wl < 2 or N not in N_SERVED:
        raise ValueError(f"{who}: frame_length = {fl!r} ms at {sr!r} Hz is {wl} samples, padded to {N}: not served ({SERVED})")
    if hop < 1:
        raise ValueError(f"{who}: frame_shift = {fs!r} ms at {sr!r} Hz is below one sample ({SERVED})")
    M = _int(who, "num_mel_bins", p["num_mel_bins"])
    if not MEL_MIN <= M <= MEL_MAX:
        raise ValueError(f"{who}: num_mel_bins = {M} is not served ({SERVED})")
    wt = p["window_type"]
    if wt not in WINDOWS:
        raise ValueError(f"{who}: window_type = {wt!r} is not served ({SERVED})")
    low, high = _real(who, "low_freq", p["low_freq"]), _real(who, "high_freq", p["high_freq"])
    if high <= 0.0:
        high += 0.5 * sr
    if not (0.0 <= low < high <= 0.5 * sr):
        raise ValueError(f"{who}: need 0 <= low_freq < high_freq <= sr / 2 (got {low!r}, {high!r} at {sr!r} Hz)")
    pre = _real(who, "preemphasis_coefficient", p["preemphasis_coefficient"])
    if not 0.0 <= pre <= 1.0:
        raise ValueError(f"{who}: preemphasis_coefficient must be in [0, 1] (got {pre!r})")
    dither, ef = _real(who, "dither", p["dither"]), _real(who, "energy_floor", p["energy_floor"])
    md = _real(who, "min_duration", p["min_duration"])
    if dither < 0 or ef < 0 or md < 0:
        raise ValueError(f"{who}: dither, energy_floor and min_duration must be non-negative (got {dither!r}, {ef!r}, {md!r})")
    use_energy = _flag(who, "use_energy", p["use_energy"])
    nc, lifter = 0, 0.0
    if mfcc:
        nc = _int(who, "num_ceps", p["num_ceps"])
        if not 1 <= nc <= M:
            raise ValueError(f"{who}: num_ceps = {nc} is not served at num_mel_bins = {M} ({SERVED})")
        lifter = _real(who, "cepstral_lifter", p["cepstral_lifter"])
        if lifter < 0:
            raise ValueError(f"{who}: cepstral_lifter must be non-negative (got {lifter!r})")
    return Spec(mfcc=mfcc, sr=sr, wl=wl, hop=hop, N=N, M=M, low=low, high=high, window_type=wt,
                blackman_coeff=_real(who, "blackman_coeff", p["blackman_coeff"]), preemph=pre,
                remove_dc=_flag(who, "remove_dc_offset", p["remove_dc_offset"]), raw_energy=_flag(who, "raw_energy", p["raw_energy"]),
                use_power=True if mfcc else _flag(who, "use_power", p["use_power"]),
                use_log=True if mfcc else _flag(who, "use_log_fbank", p["use_log_fbank"]), use_energy=use_energy,
                htk_compat=_flag(who, "htk_compat", p["htk_compat"]), energy_floor=ef, dither=dither,
                snip_edges=_flag(who, "snip_edges", p["snip_edges"]), subtract_mean=_flag(who, "subtract_mean", p["subtract_mean"]),
                min_duration=md, num_ceps=nc, lifter=lifter, C=nc if mfcc else M + int(use_energy))


def frames_of(spec: Spec, L: int) -> int:
    """Frames of a clip of L samples: 0 below min_duration."""
    if L < spec.min_duration * spec.sr:
        return 0
    return num_frames(L, spec.wl, spec.hop, spec.snip_edges)


def check_layout(who: str, layout) -> str:
    if layout not in LAYOUTS:
        raise ValueError(f"{who}: layout must be 'ct' ([B, C, T]) or 'tc' ([B, T, C]) (got {layout!r})")
    return layout


def check_seed(who: str, seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64) (got {seed!r})")
    return int(seed)


# ------------------------------------------------------------------ tables (float64; *_f32: rounded once)
@lru_cache(maxsize=64)
def window(window_type: str, wl: int, blackman_coeff: float = 0.42) -> np.ndarray:
    """Kaldi's symmetric windows of wl samples."""
    n = np.arange(wl, dtype=np.float64)
    a = 2.0 * np.pi / (wl - 1)
    if window_type == "hanning":
        w = 0.5 - 0.5 * np.cos(a * n)
    elif window_type == "hamming":
        w = 0.54 - 0.46 * np.cos(a * n)
    elif window_type == "povey":
        w = (0.5 - 0.5 * np.cos(a * n)) ** 0.85
    elif window_type == "rectangular":
        w = np.ones(wl, dtype=np.float64)
    elif window_type == "blackman":
        w = blackman_coeff - 0.5 * np.cos(a * n) + (0.5 - blackman_coeff) * np.cos(2.0 * a * n)
    else:
        raise ValueError(f"window_type = {window_type!r} is not served ({SERVED})")
    w.setflags(write=False)
    return w


def mel_scale(f):
    """HTK: 1127 ln(1 + f / 700)."""
    return 1127.0 * np.log1p(np.asarray(f, dtype=np.float64) / 700.0)


@lru_cache(maxsize=64)
def mel_banks(M: int, N: int, sr: float, low: float, high: float) -> np.ndarray:
    """[M, N / 2]: triangles drawn in the mel domain, unit peak, no area normalisation; the Nyquist bin has no column."""
    ml, mh = float(mel_scale(low)), float(mel_scale(high))
    delta = (mh - ml) / (M + 1)
    mel = mel_scale(np.arange(N // 2, dtype=np.float64) * (sr / N))[None, :]
    left = ml + np.arange(M, dtype=np.float64)[:, None] * delta
    right = left + 2.0 * delta
    w = np.maximum(0.0, np.minimum((mel - left) / delta, (right - mel) / delta))
    w.setflags(write=False)
    return w


def mel_padded_f32(M: int, N: int, sr: float, low: float, high: float) -> np.ndarray:
    """[16 ceil(M / 16), N / 2] float32, rows past M zero: the A operand of the projection."""
    bp = np.zeros((-(-M // 16) * 16, N // 2), dtype=np.float32)
    bp[:M] = mel_banks(M, N, sr, low, high)
    return bp


def lifter_weights(num_ceps: int, Q: float) -> np.ndarray:
    i = np.arange(num_ceps, dtype=np.float64)
    return np.ones(num_ceps) if Q == 0 else 1.0 + 0.5 * Q * np.sin(np.pi * i / Q)


@lru_cache(maxsize=64)
def dct_lifter(num_ceps: int, M: int, Q: float) -> np.ndarray:
    """[num_ceps, M]: the orthonormal DCT-II rows times Kaldi's lifter 1 + 0.5 Q sin(pi i / Q) (Q = 0: none)."""
    k = np.arange(num_ceps, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    d = np.sqrt(2.0 / M) * np.cos(np.pi * k * (m + 0.5) / M)
    d[0] = np.sqrt(1.0 / M)
    d = d * lifter_weights(num_ceps, Q)[:, None]
    d.setflags(write=False)
    return d


def twiddle_f32(N: int) -> np.ndarray:
    """[N + N / 2, 2] float32: W_N^k (the real-input split), then W_(N/2)^k (the transform's passes)."""
    return np.concatenate([T.twiddles(N), T.twiddles(N // 2)])


def cep_columns(num_ceps: int, htk_compat: bool) -> np.ndarray:
    """Column of coefficient k in the result: htk_compat moves coefficient 0 to the end."""
    k = np.arange(num_ceps)
    return np.where(k == 0, num_ceps - 1, k - 1) if htk_compat else k
