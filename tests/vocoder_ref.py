"""Float64 restatement of librosa 0.10 `phase_vocoder` / `effects.time_stretch` and of the reference's `add_noise`
(librosa is not a dependency: this is the parity contract of syg_phase_vocoder_f32 and syg_fx_add_noise_f32)."""
from __future__ import annotations

import numpy as np

from tests import hpss_ref as R

N_FFT = R.N_FFT
HOP = R.HOP
EPS64 = np.finfo(np.float64).eps


def phase_vocoder(D, rate, hop_length=HOP, n_fft=N_FFT):
    """librosa.phase_vocoder of D [n_fft / 2 + 1, T] complex -> [n_fft / 2 + 1, ceil(T / rate)], the angle form exactly
    as librosa writes it."""
    D = np.asarray(D, dtype=np.complex128)
    time_steps = np.arange(0, D.shape[-1], rate, dtype=np.float64)
    d_stretch = np.zeros((D.shape[0], len(time_steps)), dtype=np.complex128)
    phi_advance = hop_length * np.fft.rfftfreq(n_fft, d=1.0 / (2 * np.pi))     # fft_frequencies(sr=2 pi, n_fft)
    phase_acc = np.angle(D[:, 0])
    D = np.pad(D, [(0, 0), (0, 2)], mode="constant")
    for t, step in enumerate(time_steps):
        columns = D[:, int(step):int(step + 2)]
        alpha = np.mod(step, 1.0)
        mag = (1.0 - alpha) * np.abs(columns[:, 0]) + alpha * np.abs(columns[:, 1])
        d_stretch[:, t] = mag * (np.cos(phase_acc) + 1j * np.sin(phase_acc))   # util.phasor(phase_acc, mag=mag)
        dphase = np.angle(columns[:, 1]) - np.angle(columns[:, 0]) - phi_advance
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        phase_acc += phi_advance + dphase
    return d_stretch


def unit(z):
    """z / |z| = exp(i np.angle(z)); an all-zero element gives (copysign(1, re), 0): np.angle(-0 + 0j) is pi."""
    z = np.asarray(z, dtype=np.complex128)
    m = np.abs(z)
    zero = m == 0
    u = z / np.where(zero, 1.0, m)
    u[zero] = np.copysign(1.0, z.real[zero])
    return u


def phase_vocoder_product(D, rate):
    """The same transform as a product of unit phasors (what the device computes): modulo 2 pi the advance and the wrap
    of the angle form cancel, so p[t] = u(D[0]) prod_{j < t} u(D[c_j + 1]) conj(u(D[c_j]))."""
    D = np.asarray(D, dtype=np.complex128)
    time_steps = np.arange(0, D.shape[-1], rate, dtype=np.float64)
    out = np.zeros((D.shape[0], len(time_steps)), dtype=np.complex128)
    p = unit(D[:, 0])
    D = np.pad(D, [(0, 0), (0, 2)], mode="constant")
    for t, step in enumerate(time_steps):
        c = int(step)
        alpha = np.mod(step, 1.0)
        out[:, t] = ((1.0 - alpha) * np.abs(D[:, c]) + alpha * np.abs(D[:, c + 1])) * p
        p = p * unit(D[:, c + 1]) * np.conj(unit(D[:, c]))
    return out


def stretch_length(L, rate):
    """Output length of librosa.effects.time_stretch: Python's round, half to even."""
    return int(round(L / rate))


def time_stretch(y, rate):
    """librosa.effects.time_stretch(y, rate=rate) with its defaults (n_fft 2048, hop 512, hann, centred), float64."""
    y = np.asarray(y, dtype=np.float64)
    return R.istft(phase_vocoder(R.stft(y), rate), stretch_length(len(y), rate))


def add_noise_with(y, noise, snr_db):
    """The arithmetic of the reference's add_noise (noise.py:75-101) on a given noise array."""
    y = np.asarray(y, dtype=np.float64)
    noise = np.asarray(noise, dtype=np.float64)
    signal_power = np.mean(y ** 2)
    noise_power = np.mean(noise ** 2)
    if signal_power < EPS64 or noise_power < EPS64:
        return y
    snr_linear = 10.0 ** (snr_db / 10.0)
    return y + noise * np.sqrt((signal_power / snr_linear) / noise_power)


def add_noise(y, snr_db, seed=None):
    """The reference's add_noise for 'gaussian' / 'white' (and its placeholders): a seeded standard-normal draw."""
    y = np.asarray(y, dtype=np.float64)
    return add_noise_with(y, np.random.default_rng(seed).standard_normal(len(y)), snr_db)


# ------------------------------------------------------------------ signals of the conditioning table (README)
def tones_noise(L, seed=0):
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    y = sum(a * np.sin(2 * np.pi * f * n / 22050.0 + ph) for a, f, ph in ((0.4, 440.0, 0.3), (0.25, 1333.0, 1.1), (0.1, 5020.0, 2.0)))
    return y + 0.05 * rng.standard_normal(L)


def white(L, seed=1):
    return 0.3 * np.random.default_rng(seed).standard_normal(L)
