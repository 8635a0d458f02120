"""Float64 restatement of the reference's audio effects (sygnals/core/audio/effects: delay.py, tremolo.py, compression.py,
reverb.py, utility.py): the parity contract of the syg_fx_* entries and of syg_spectral_gate_f32.  Vectorised; the two
spectral effects call librosa in the reference (not a dependency) and rest on the restatement of tests/hpss_ref.py."""
from __future__ import annotations

import numpy as np
from scipy.signal import fftconvolve, lfilter

from tests import hpss_ref as H


def delay_samples(delay_time, sr):
    return int(delay_time * sr)


def delay_core(y, D, feedback, wet, dry):
    """w[n] = y[n] + feedback w[n - D]; out[n] = dry y[n] + wet w[n - D]; w = 0 before the clip (D >= 1)."""
    y = np.asarray(y, dtype=np.float64)
    L = len(y)
    w = np.zeros(L)
    if D * D <= L:                                 # few long chains: one first-order recursion per residue n mod D
        for r in range(D):
            w[r::D] = lfilter([1.0], [1.0, -feedback], y[r::D])
    else:                                          # many short chains: step by step, every residue at once
        w[:D] = y[:D]
        for s in range(D, L, D):
            e = min(s + D, L)
            w[s:e] = y[s:e] + feedback * w[s - D:e - D]
    wd = np.zeros(L)
    if D < L:
        wd[D:] = w[:L - D]
    return dry * y + wet * wd


def apply_delay(y, sr, delay_time=0.5, feedback=0.4, wet_level=0.5, dry_level=1.0):
    y = np.asarray(y, dtype=np.float64)
    D = delay_samples(delay_time, sr)
    if D <= 0:
        return (dry_level + wet_level) * y
    return delay_core(y, D, feedback, wet_level, dry_level)


def chorus_delay_samples(delay, depth, sr):
    """The delay that apply_chorus really applies: its read position is left of its interpolation grid, so np.interp
    returns the oldest sample of a buffer of this many samples and the LFO has no effect."""
    return int(np.ceil((delay + depth) * sr)) + 2


def lfo(sr, n, rate, shape, n0=0):
    """_generate_lfo for samples n0 .. n0 + n - 1, values in [0, 1]."""
    phase = 2 * np.pi * rate * (np.arange(n0, n0 + n) / sr)
    if shape == "sine":
        return (np.sin(phase) + 1.0) / 2.0
    if shape == "triangle":                        # scipy.signal.sawtooth(phase, 0.5)
        tm = np.mod(phase, 2 * np.pi)
        s = np.where(tm < np.pi, tm / (np.pi * 0.5) - 1.0, (np.pi * 1.5 - tm) / (np.pi * 0.5))
        return (s + 1.0) / 2.0
    if shape == "square":
        return (np.sin(phase) > 0).astype(np.float64)
    raise ValueError(shape)


def apply_tremolo(y, sr, rate=5.0, depth=0.5, shape="sine", n0=0):
    y = np.asarray(y, dtype=np.float64)
    return y * ((1.0 - depth) + lfo(sr, len(y), rate, shape, n0) * depth)


def compress(y, threshold=0.8, ratio=4.0):
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    out = y.copy()
    m = a > threshold
    out[m] = y[m] * ((threshold + (a[m] - threshold) / ratio) / a[m])
    return out


def basic_ir(sr, decay_time=0.5, seed=None):
    n = max(1, int(sr * decay_time * 1.5))
    if decay_time < 1e-6 or n <= 1:
        return np.array([1.0])
    noise = np.random.default_rng(seed).standard_normal(n)
    ir = noise * np.exp(-(-np.log(0.001) / (decay_time * sr + 1e-9)) * np.arange(n))
    return ir / np.max(np.abs(ir))


def apply_reverb(y, sr, decay_time=0.5, wet_level=0.3, dry_level=0.7, ir_seed=None):
    y = np.asarray(y, dtype=np.float64)
    ir = basic_ir(sr, decay_time, ir_seed)
    if len(ir) == 1:
        return (dry_level + wet_level) * y
    wet = fftconvolve(y, ir, mode="full")
    out = wet_level * wet
    out[:len(y)] += dry_level * y
    return out


def adjust_gain(y, gain_db):
    return np.asarray(y, dtype=np.float64) * 10.0 ** (gain_db / 20.0)


def midside(y, width=1.5):
    y = np.asarray(y, dtype=np.float64)
    mid, side = (y[0] + y[1]) / 2.0, (y[0] - y[1]) / 2.0 * width
    return np.stack([mid + side, mid - side])


def noise_profile(Dn):
    """Mean power per bin of the noise segment's STFT Dn [F, Tn]."""
    return np.mean(np.abs(Dn) ** 2, axis=1)


def gate(P, N, amount):
    """The gain sqrt(max(0, 1 - amount N / P)) on powers P [F, T] with the profile N [F]; 0 where P is 0."""
    P = np.asarray(P, dtype=np.float64)
    G = np.zeros_like(P)
    nz = P > 0
    G[nz] = np.sqrt(np.maximum(0.0, 1.0 - (amount * np.broadcast_to(N[:, None], P.shape)[nz]) / P[nz]))
    return G


def noise_reduction_spectral(y, sr, noise_profile_duration=0.5, reduction_amount=1.0):
    """n_fft 2048, hop 512.  The reference rebuilds the spectrum as sqrt(max(0, |D|^2 - a N)) exp(i angle D): the same
    numbers as the gain applied to D."""
    y = np.asarray(y, dtype=np.float64)
    ns = int(noise_profile_duration * sr)
    N = noise_profile(H.stft(y[:ns]))
    D = H.stft(y)
    mag = np.sqrt(np.maximum(0.0, np.abs(D) ** 2 - reduction_amount * N[:, None]))
    return H.istft(mag * np.exp(1j * np.angle(D)), len(y))


def transient_shaping_hpss(y, sr, percussive_scale=1.0, harmonic_margin=1.0, percussive_margin=1.0):
    yh, yp = H.hpss(y, 31, 2.0, (harmonic_margin, percussive_margin))
    return yh + yp * percussive_scale
