"""Float64 restatement of librosa 0.10 `onset.onset_strength`, `util.peak_pick` and `onset.onset_detect` (librosa is not
a dependency: this is the parity contract of syg_onset_strength_f32 / syg_onset_peaks_f32), plus the clip generators the
onset tests share."""
from __future__ import annotations

import numpy as np
import scipy.ndimage
import scipy.signal

from oracle import cpu_ref as O


def log_mel(y, sr, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None, center=True):
    """power_to_db(melspectrogram(|STFT|^2), ref=1.0, amin=1e-10, top_db=80.0): Slaney mel, hann, zero-padded centre."""
    D = O.stft(y, n_fft=n_fft, hop_length=hop_length, window="hann", center=center, pad_mode="constant")
    B = O.mel_filterbank(sr, n_fft, n_mels, fmin, sr / 2.0 if fmax is None else fmax).astype(np.float64)
    return O.power_to_db(B @ (np.abs(D) ** 2), ref=1.0, amin=1e-10, top_db=80.0)


def onset_strength_from_db(S, n_fft=2048, hop_length=512, lag=1, max_size=1, center=True, detrend=False):
    """The part after the log-mel matrix S [M, T]."""
    S = np.asarray(S, dtype=np.float64)
    if not isinstance(lag, (int, np.integer)) or lag < 1:
        raise ValueError("lag must be a positive integer")
    if not isinstance(max_size, (int, np.integer)) or max_size < 1:
        raise ValueError("max_size must be a positive integer")
    T = S.shape[1]
    ref = S if max_size == 1 else scipy.ndimage.maximum_filter1d(S, max_size, axis=0)
    d = np.mean(np.maximum(0.0, S[:, lag:] - ref[:, :max(T - lag, 0)]), axis=0)     # (librosa: ref[..., :-lag])
    pad = lag + (n_fft // (2 * hop_length) if center else 0)
    env = np.concatenate([np.zeros(pad), d])
    if detrend:
        env = scipy.signal.lfilter([1.0, -1.0], [1.0, -0.99], env)
    return env[:T] if center else env


def onset_strength(y, sr, n_fft=2048, hop_length=512, n_mels=128, fmin=0.0, fmax=None, lag=1, max_size=1, center=True,
                   detrend=False):
    S = log_mel(y, sr, n_fft, hop_length, n_mels, fmin, fmax, center)
    return onset_strength_from_db(S, n_fft, hop_length, lag, max_size, center, detrend)


def _check_windows(pre_max, post_max, pre_avg, post_avg, delta, wait):
    for name, v in (("pre_max", pre_max), ("pre_avg", pre_avg), ("delta", delta), ("wait", wait)):
        if v < 0:
            raise ValueError(f"{name} must be non-negative")
    for name, v in (("post_max", post_max), ("post_avg", post_avg)):
        if v <= 0:
            raise ValueError(f"{name} must be positive")


def peak_terms(x, pre_max, post_max, pre_avg, post_avg):
    """(window maximum, window mean) of x with the explicit windows [max(0, n - pre), min(N, n + post))."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    mx = np.empty(N)
    av = np.empty(N)
    for n in range(N):
        mx[n] = x[max(0, n - pre_max):min(N, n + post_max)].max()
        av[n] = x[max(0, n - pre_avg):min(N, n + post_avg)].mean()
    return mx, av


def peak_candidates(x, pre_max, post_max, pre_avg, post_avg, delta):
    x = np.asarray(x, dtype=np.float64)
    mx, av = peak_terms(x, pre_max, post_max, pre_avg, post_avg)
    return (x == mx) & (x >= av + delta) & (x != 0)


def greedy_wait(cand, wait):
    out = []
    last = -np.inf
    for n in np.flatnonzero(cand):
        if n > last + wait:
            out.append(n)
            last = n
    return np.array(out, dtype=np.int64)


def peak_pick(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    pre_max, post_max, pre_avg, post_avg, wait = (int(v) for v in (pre_max, post_max, pre_avg, post_avg, wait))
    _check_windows(pre_max, post_max, pre_avg, post_avg, delta, wait)
    return greedy_wait(peak_candidates(x, pre_max, post_max, pre_avg, post_avg, delta), wait)


def peak_pick_scipy(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    """util.peak_pick as librosa 0.10.0 writes it: scipy.ndimage filters with a shifted origin, edge means recomputed."""
    x = np.asarray(x, dtype=np.float64)
    max_length = pre_max + post_max
    max_origin = int(np.ceil(0.5 * (pre_max - post_max)))
    mov_max = scipy.ndimage.maximum_filter1d(x, int(max_length), mode="constant", origin=max_origin, cval=x.min())
    avg_length = pre_avg + post_avg
    avg_origin = int(np.ceil(0.5 * (pre_avg - post_avg)))
    mov_avg = scipy.ndimage.uniform_filter1d(x, int(avg_length), mode="nearest", origin=avg_origin)
    n = 0
    while n - pre_avg < 0 and n < x.shape[0]:
        mov_avg[n] = np.mean(x[0:n + post_avg])
        n += 1
    n = x.shape[0] - post_avg
    n = n if n > 0 else 0
    while n < x.shape[0]:
        mov_avg[n] = np.mean(x[n - pre_avg:n + post_avg] if n - pre_avg >= 0 else x[0:n + post_avg])
        n += 1
    det = x * (x == mov_max)
    det = det * (det >= mov_avg + delta)
    return greedy_wait(det != 0, wait)


def default_windows(sr, hop_length):
    """onset_detect's defaults in frames; Python precedence makes each (c * sr) // hop_length, a float floor division."""
    return {"pre_max": int(0.03 * sr // hop_length), "post_max": int(0.00 * sr // hop_length + 1),
            "pre_avg": int(0.10 * sr // hop_length), "post_avg": int(0.10 * sr // hop_length + 1),
            "wait": int(0.03 * sr // hop_length), "delta": 0.07}


def normalize(env):
    env = np.asarray(env)
    tiny = np.finfo(env.dtype if np.issubdtype(env.dtype, np.floating) else np.float64).tiny
    x = env.astype(np.float64) - float(env.min())
    return x / (x.max() + tiny)


def local_minima(e):
    """i with e[i] <= e[i - 1] and e[i] < e[i + 1]; frame 0 is always in the set."""
    e = np.asarray(e, dtype=np.float64)
    m = 1 + np.flatnonzero((e[1:-1] <= e[:-2]) & (e[1:-1] < e[2:]))
    return np.unique(np.concatenate([[0], m])).astype(np.int64)


def backtrack(onsets, energy):
    minima = local_minima(energy)
    onsets = np.asarray(onsets, dtype=np.int64)
    return minima[np.searchsorted(minima, onsets, side="right") - 1] if len(onsets) else onsets


def onset_detect(y=None, sr=22050, onset_envelope=None, hop_length=512, backtrack_=False, energy=None, normalize_=True,
                 units="frames", **kwargs):
    if onset_envelope is None:
        if y is None:
            raise ValueError("y or onset_envelope must be provided")
        onset_envelope = onset_strength(y, sr, hop_length=hop_length)
    env = np.asarray(onset_envelope)
    if env.size == 0 or not env.any() or not np.all(np.isfinite(env)):
        onsets = np.array([], dtype=np.int64)
    else:
        x = normalize(env) if normalize_ else env.astype(np.float64)
        pk = default_windows(sr, hop_length)
        pk.update(kwargs)
        onsets = peak_pick(x, **pk)
        if backtrack_:
            onsets = backtrack(onsets, x if energy is None else energy)
    if units == "frames":
        return onsets
    if units == "samples":
        return onsets * hop_length
    if units == "time":
        return onsets * hop_length / float(sr)
    raise ValueError(f"Invalid unit type: {units}")


# ---------------------------------------------------------------------------- margins
def unsure_mean(x, pre_avg, post_avg, delta, margin, pre_max=1, post_max=1):
    """Frames whose mean test sits within `margin` of its threshold."""
    x = np.asarray(x, dtype=np.float64)
    _, av = peak_terms(x, pre_max, post_max, pre_avg, post_avg)
    return np.abs(x - (av + delta)) <= margin


def unsure_frames(x, pre_max, post_max, pre_avg, post_avg, delta, margin):
    """End-to-end rule.  A test is *close* when the mean test sits within `margin` of its threshold, or when x[n] is
    within `margin` of the largest OTHER value of its max window.  A close test can change the outcome only where the
    other test passes or is close itself, so a frame is unsure when one test is close and the other is not failed by
    more than `margin`.  (Taken alone, either closeness marks every run of equal values -- the zeros of the padding
    and of digital silence, which fail the mean test by delta -- and a fixture could never meet the cap.)"""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    _, av = peak_terms(x, pre_max, post_max, pre_avg, post_avg)
    mean_close = np.abs(x - (av + delta)) <= margin
    mean_open = x >= av + delta - margin
    max_close = np.zeros(N, dtype=bool)
    max_open = np.ones(N, dtype=bool)
    for n in range(N):
        a0, a1 = max(0, n - pre_max), min(N, n + post_max)
        others = np.delete(x[a0:a1], n - a0)
        if others.size:
            max_close[n] = abs(x[n] - others.max()) <= margin
            max_open[n] = x[n] >= others.max() - margin
    return (mean_close & max_open) | (max_close & mean_open)


# ---------------------------------------------------------------------------- clips
def burst_clip(sr, length, seed, floor=1e-3, n_bursts=None):
    """Decaying tone bursts at seeded positions over a noise floor (floor = 0: digital silence between them)."""
    rng = np.random.default_rng(seed)
    y = floor * rng.standard_normal(length)
    n_bursts = int(rng.integers(2, 6)) if n_bursts is None else n_bursts
    lo, hi = int(0.08 * length), int(0.92 * length)
    slots = np.linspace(lo, hi, n_bursts + 1)
    for i in range(n_bursts):
        pos = int(rng.uniform(slots[i], slots[i] + 0.5 * (slots[i + 1] - slots[i])))
        dur = min(int(sr * rng.uniform(0.04, 0.1)), length - pos)
        t = np.arange(dur) / sr
        f = rng.uniform(200.0, 0.2 * sr)
        y[pos:pos + dur] += rng.uniform(0.2, 0.8) * np.sin(2 * np.pi * f * t) * np.exp(-t * rng.uniform(20.0, 60.0))
    return y


def gpu_clips(sr, length, n=10, seed0=100):
    """The end-to-end fixture: n burst clips, every third over digital silence.  float32 values (what the device reads),
    returned as float64."""
    Y = np.stack([burst_clip(sr, length, seed0 + i, floor=0.0 if i % 3 == 2 else 1e-3) for i in range(n)])
    return Y.astype(np.float32).astype(np.float64)


def silence_clip(sr, seed=7):
    """Three noise passages separated by near-silence, for segment_by_silence."""
    rng = np.random.default_rng(seed)
    parts = [1e-5 * rng.standard_normal(int(0.30 * sr)), 0.3 * rng.standard_normal(int(0.50 * sr)),
             1e-5 * rng.standard_normal(int(0.40 * sr)), 0.2 * rng.standard_normal(int(0.35 * sr)),
             1e-5 * rng.standard_normal(int(0.25 * sr)), 0.4 * rng.standard_normal(int(0.45 * sr)),
             1e-5 * rng.standard_normal(int(0.20 * sr))]
    return np.concatenate(parts).astype(np.float32).astype(np.float64)


def rms_frames(y, frame_length, hop_length):
    """librosa.feature.rms(center=True, pad_mode='constant')."""
    F = O.frame_signal(y, frame_length, hop_length, True)
    return np.sqrt(np.mean(F * F, axis=1))


# ---------------------------------------------------------------------------- what the end-to-end tests share
TOL = 1e-5
E2E_CASES = [(22050, 512, 33075), (48000, 512, 48000), (16000, 256, 16000)]      # sr, hop, clip length


def e2e_reference(sr, hop, Y):
    """Per clip: (onset frames, unsure-frame mask at 10 * TOL) from the restatement alone."""
    out = []
    pk = default_windows(sr, hop)
    for y in Y:
        env = onset_strength(y, sr, hop_length=hop)
        on = onset_detect(onset_envelope=env, sr=sr, hop_length=hop)
        un = unsure_frames(normalize(env), pk["pre_max"], pk["post_max"], pk["pre_avg"], pk["post_avg"], pk["delta"],
                           10 * TOL) if env.any() else np.zeros(len(env), dtype=bool)
        out.append((on, un))
    return out


def within_cap(unsure_masks):
    """At most 1 % of all frames unsure, and at most one clip in ten with any."""
    frames = sum(len(u) for u in unsure_masks)
    bad = sum(int(u.sum()) for u in unsure_masks)
    clips = sum(bool(u.any()) for u in unsure_masks)
    return bad <= 0.01 * frames and clips <= 0.1 * len(unsure_masks), (bad, frames, clips, len(unsure_masks))


SILENCE_CASE = dict(sr=22050, frame_length=512, hop_length=128, threshold_db=-40.0)


def silence_unsure(rms, threshold_db):
    """Frames whose RMS is within 10 * TOL, relative, of the silence threshold."""
    rms = np.asarray(rms, dtype=np.float64)
    thr = rms.max() * 10.0 ** (threshold_db / 20.0)
    return np.abs(rms - thr) <= 10 * TOL * thr


# ---------------------------------------------------------------------------- what the parameter sweep adds
def flux_envelope(S, lag=1, max_size=1, pad=0, T_out=None, detrend=False):
    """The envelope as syg_onset_strength_f32 states it: `pad` zeros in front of the flux of the dB matrix S [M, T], detrended
    when asked, cut to T_out frames (default: uncut, pad + T - lag).  onset_strength_from_db is this with
    pad = lag + n_fft // (2 hop), T_out = T (centre) and with pad = lag, uncut (no centre)."""
    S = np.asarray(S, dtype=np.float64)
    d = onset_strength_from_db(S, lag=lag, max_size=max_size, center=False)[lag:]
    env = np.concatenate([np.zeros(pad), d])
    if detrend:
        env = scipy.signal.lfilter([1.0, -1.0], [1.0, -0.99], env)
    return env if T_out is None else env[:T_out]


def e2e_reference_with(sr, hop, Y, backtrack_=False, **peak):
    """e2e_reference with peak_pick arguments other than the defaults (and backtracking): per clip (onset frames, unsure
    mask at 10 * TOL).  Backtracking moves onsets that are already decided, so the unsure rule is the same."""
    out = []
    pk = default_windows(sr, hop)
    pk.update(peak)
    for y in Y:
        env = onset_strength(y, sr, hop_length=hop)
        on = onset_detect(onset_envelope=env, sr=sr, hop_length=hop, backtrack_=backtrack_, **peak)
        un = unsure_frames(normalize(env), pk["pre_max"], pk["post_max"], pk["pre_avg"], pk["post_avg"], pk["delta"],
                           10 * TOL) if env.any() else np.zeros(len(env), dtype=bool)
        out.append((on, un))
    return out


def peak_margin(pre_avg, post_avg):
    """The margin of the peaks-alone tests: (W + 4) 2^-24 for a mean window of W frames."""
    return (pre_avg + post_avg + 4) * 2.0 ** -24
