"""Float64 NumPy restatement of torchaudio.compliance.kaldi.fbank / mfcc (Kaldi's feature-window.cc and
mel-computations.cc): the contract of the device front end (csrc/kaldi_front.hip).  torchaudio and Kaldi are not
dependencies; parity with them is unpinned, and this restatement is pinned by construction (tests/test_kaldi_ref.py).

Sizes, frame counts and eps come from sygnals_amd/_kaldi.py, so that int() / floor of the same expression cannot disagree
between the two sides; windows, mel banks, DCT and lifter are restated here on their own.  Keyword names and defaults are
torchaudio's.  Results are [T, C] (Kaldi's layout)."""
import math

import numpy as np

from sygnals_amd import _kaldi as KD

EPS = KD.EPS


def reflect(s: int, L: int) -> int:
    """Kaldi's rule for an index outside [0, L): s <- -s - 1 or s <- 2 L - 1 - s, repeated until inside."""
    while s < 0 or s >= L:
        s = -s - 1 if s < 0 else 2 * L - 1 - s
    return s


def frames(x, wl, hop, snip_edges=True):
    """[T, wl] float64 frames of the clip x by Kaldi's framing rule."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    T = KD.num_frames(L, wl, hop, snip_edges)
    out = np.zeros((T, wl))
    for t in range(T):
        s0 = KD.frame_start(t, wl, hop, snip_edges)
        if 0 <= s0 and s0 + wl <= L:
            out[t] = x[s0:s0 + wl]
        else:
            out[t] = [x[reflect(s0 + i, L)] for i in range(wl)]
    return out


def window(window_type, wl, blackman_coeff=0.42):
    n = np.arange(wl, dtype=np.float64)
    a = 2.0 * math.pi / (wl - 1)
    hann = 0.5 - 0.5 * np.cos(a * n)
    if window_type == "hanning":
        return hann
    if window_type == "hamming":
        return 0.54 - 0.46 * np.cos(a * n)
    if window_type == "povey":
        return hann ** 0.85
    if window_type == "rectangular":
        return np.ones(wl)
    if window_type == "blackman":
        return blackman_coeff - 0.5 * np.cos(a * n) + (0.5 - blackman_coeff) * np.cos(2 * a * n)
    raise ValueError(window_type)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_banks(M, N, sr, low=20.0, high=0.0):
    """[M, N / 2]: the Nyquist bin carries no weight."""
    if high <= 0.0:
        high += 0.5 * sr
    ml, mh = float(mel(low)), float(mel(high))
    delta = (mh - ml) / (M + 1)
    mk = mel(np.arange(N // 2) * sr / N)
    w = np.zeros((M, N // 2))
    for m in range(M):
        left = ml + m * delta
        right = left + 2 * delta
        w[m] = np.maximum(0.0, np.minimum((mk - left) / delta, (right - mk) / delta))
    return w


def preemphasis(fr, c):
    """x[i] -= c x[i - 1] with x[-1] := x[0], on [T, wl]."""
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    return fr - c * prev


def log_energy(fr, energy_floor):
    e = np.log(np.maximum(np.sum(fr * fr, axis=1), EPS))
    return np.maximum(e, math.log(energy_floor)) if energy_floor > 0 else e


def windowed(x, sr, *, blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0,
             preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, snip_edges=True, window_type="povey",
             rng=None, **_):
    """([T, N] windowed, zero-padded frames, [T] log-energies)."""
    wl, hop, N = KD.sizes(sr, frame_length, frame_shift)
    fr = frames(x, wl, hop, snip_edges)
    if dither != 0.0:
        fr = fr + dither * (rng or np.random.default_rng(0)).standard_normal(fr.shape)
    if remove_dc_offset:
        fr = fr - fr.mean(axis=1, keepdims=True)
    e = log_energy(fr, energy_floor) if raw_energy else None
    fr = preemphasis(fr, preemphasis_coefficient)
    fr = fr * window(window_type, wl, blackman_coeff)[None, :]
    if not raw_energy:
        e = log_energy(fr, energy_floor)
    return np.pad(fr, ((0, 0), (0, N - wl))), e


def mel_energies(x, sr, *, num_mel_bins=23, low_freq=20.0, high_freq=0.0, use_power=True, **kw):
    """([T, M] mel energies before the logarithm, [T] log-energies)."""
    fr, e = windowed(x, sr, **kw)
    N = fr.shape[1]
    spec = np.abs(np.fft.rfft(fr, axis=1))[:, :N // 2]
    if use_power:
        spec = spec * spec
    return spec @ mel_banks(num_mel_bins, N, sr, low_freq, high_freq).T, e


def _empty(x, sr, frame_length, frame_shift, snip_edges, min_duration):
    wl, hop, _ = KD.sizes(sr, frame_length, frame_shift)
    L = np.asarray(x).shape[0]
    return L < min_duration * sr or KD.num_frames(L, wl, hop, snip_edges) == 0


def fbank(x, sample_frequency=16000.0, *, htk_compat=False, min_duration=0.0, num_mel_bins=23, subtract_mean=False,
          use_energy=False, use_log_fbank=True, round_to_power_of_two=True, vtln_warp=1.0, **kw):
    if not round_to_power_of_two or vtln_warp != 1.0:
        raise ValueError("round_to_power_of_two=False and vtln_warp != 1 are outside the contract")
    sr = sample_frequency
    C = num_mel_bins + int(use_energy)
    if _empty(x, sr, kw.get("frame_length", 25.0), kw.get("frame_shift", 10.0), kw.get("snip_edges", True), min_duration):
        return np.zeros((0, C))
    E, e = mel_energies(x, sr, num_mel_bins=num_mel_bins, **kw)
    f = np.log(np.maximum(E, EPS)) if use_log_fbank else E
    if use_energy:
        f = np.concatenate([f, e[:, None]], axis=1) if htk_compat else np.concatenate([e[:, None], f], axis=1)
    if subtract_mean:
        f = f - f.mean(axis=0, keepdims=True)
    return f


def dct_matrix(num_ceps, M):
    """[num_ceps, M]: the first rows of the orthonormal DCT-II."""
    d = np.zeros((num_ceps, M))
    for k in range(num_ceps):
        for m in range(M):
            d[k, m] = math.sqrt((1.0 if k == 0 else 2.0) / M) * math.cos(math.pi * k * (m + 0.5) / M)
    return d


def lifter(num_ceps, Q):
    return np.array([1.0 if Q == 0 else 1.0 + 0.5 * Q * math.sin(math.pi * i / Q) for i in range(num_ceps)])


def cepstra(logfb, num_ceps=13, cepstral_lifter=22.0):
    """[..., T, num_ceps] from the log filterbank [..., T, M]."""
    return (logfb @ dct_matrix(num_ceps, logfb.shape[-1]).T) * lifter(num_ceps, cepstral_lifter)


def finish_mfcc(c, e, use_energy=False, htk_compat=False, subtract_mean=False):
    c = np.array(c, dtype=np.float64)
    if use_energy:
        c[:, 0] = e
    if htk_compat:
        c = np.concatenate([c[:, 1:], c[:, :1]], axis=1)
    if subtract_mean:
        c = c - c.mean(axis=0, keepdims=True)
    return c


def mfcc(x, sample_frequency=16000.0, *, cepstral_lifter=22.0, num_ceps=13, htk_compat=False, min_duration=0.0, num_mel_bins=23,
         subtract_mean=False, use_energy=False, round_to_power_of_two=True, vtln_warp=1.0, **kw):
    if not round_to_power_of_two or vtln_warp != 1.0:
        raise ValueError("round_to_power_of_two=False and vtln_warp != 1 are outside the contract")
    sr = sample_frequency
    if _empty(x, sr, kw.get("frame_length", 25.0), kw.get("frame_shift", 10.0), kw.get("snip_edges", True), min_duration):
        return np.zeros((0, num_ceps))
    E, e = mel_energies(x, sr, num_mel_bins=num_mel_bins, use_power=True, **kw)
    c = cepstra(np.log(np.maximum(E, EPS)), num_ceps, cepstral_lifter)
    return finish_mfcc(c, e, use_energy, htk_compat, subtract_mean)
