"""Float64 restatement of librosa 0.10 `effects.hpss` and of the reference's harmonic_to_noise_ratio (librosa is not a
dependency: this is the parity contract of syg_hpss_masks_f32 / syg_istft2048_f32 / syg_hnr_rows_f32)."""
from __future__ import annotations

import numpy as np

N_FFT = 2048
HOP = 512
EPSILON = 1e-10


def hann(n=N_FFT):
    """Periodic Hann window (scipy.signal.get_window('hann', n, fftbins=True))."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def stft(y, n_fft=N_FFT, hop=HOP):
    """librosa.stft(center=True, pad_mode='constant', hann) -> D [n_fft / 2 + 1, T] complex128."""
    y = np.pad(np.asarray(y, dtype=np.float64), n_fft // 2, mode="constant")
    T = 1 + (len(y) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
    return np.fft.rfft(y[idx] * hann(n_fft)[None, :], axis=1).T


def reflect_index(i, n):
    """scipy.ndimage 'reflect' (half-sample symmetric, repeated): ... x1 x0 | x0 .. x(n-1) | x(n-1) x(n-2) ..."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def median_filter_axis(X, k, axis):
    """Median over windows [i - k//2, i - k//2 + k - 1] along `axis`, element of rank k//2, reflect folding."""
    X = np.moveaxis(np.asarray(X), axis, -1)
    n = X.shape[-1]
    idx = reflect_index(np.arange(n)[:, None] - k // 2 + np.arange(k)[None, :], n)   # [n, k]
    W = X[..., idx]                                                                   # [..., n, k]
    out = np.partition(W, k // 2, axis=-1)[..., k // 2]
    return np.moveaxis(out, -1, axis)


def softmask(X, X_ref, power=1.0, split_zeros=False, tiny=None):
    """librosa.util.softmask; `tiny` defaults to the finfo of X's dtype (float32 magnitudes: FLT_MIN)."""
    X = np.asarray(X)
    X_ref = np.asarray(X_ref)
    if power <= 0:
        raise ValueError("power must be strictly positive")
    if tiny is None:
        tiny = np.finfo(X.dtype if np.issubdtype(X.dtype, np.floating) else np.float32).tiny
    if not np.isfinite(power):
        return (X > X_ref).astype(np.float64)
    X = X.astype(np.float64)
    X_ref = X_ref.astype(np.float64)
    Z = np.maximum(X, X_ref)
    bad = Z < tiny
    Z[bad] = 1.0
    m = (X / Z) ** power
    r = (X_ref / Z) ** power
    good = ~bad
    m[good] /= m[good] + r[good]
    m[bad] = 0.5 if split_zeros else 0.0
    return m


def medians(S, kernel_size=31):
    kh, kp = (kernel_size, kernel_size) if np.isscalar(kernel_size) else kernel_size
    return median_filter_axis(S, kh, axis=1), median_filter_axis(S, kp, axis=0)


def masks(S, kernel_size=31, power=2.0, margin=1.0, tiny=None):
    """decompose.hpss(mask=True) on magnitudes S [F, T] -> (M_h, M_p, H, P)."""
    mh, mp = (margin, margin) if np.isscalar(margin) else margin
    if mh < 1 or mp < 1:
        raise ValueError("Margins must be >= 1.0")
    H, P = medians(S, kernel_size)
    split = mh == 1 and mp == 1
    return (softmask(H, P * mh, power, split, tiny), softmask(P, H * mp, power, split, tiny), H, P)


def istft(D, length, n_fft=N_FFT, hop=HOP):
    """librosa.istft(center=True, hann, length) of D [n_fft / 2 + 1, T]."""
    T = D.shape[1]
    n_frames = min(T, int(np.ceil((length + 2 * (n_fft // 2)) / hop)))
    w = hann(n_fft)
    fr = np.fft.irfft(D[:, :n_frames], n=n_fft, axis=0) * w[:, None]
    tot = n_fft + hop * (n_frames - 1)
    y = np.zeros(tot)
    wss = np.zeros(tot)
    for t in range(n_frames):
        y[t * hop:t * hop + n_fft] += fr[:, t]
        wss[t * hop:t * hop + n_fft] += w ** 2
    y = y[n_fft // 2:]
    wss = wss[n_fft // 2:]
    out = np.zeros(length)
    m = min(length, len(y))
    out[:m] = y[:m]
    ws = np.zeros(length)
    ws[:m] = wss[:m]
    nz = ws > np.finfo(np.float64).tiny
    out[nz] /= ws[nz]
    return out


def hpss(y, kernel_size=31, power=2.0, margin=1.0):
    """librosa.effects.hpss -> (y_harm, y_perc), float64."""
    y = np.asarray(y, dtype=np.float64)
    D = stft(y)
    Mh, Mp, _, _ = masks(np.abs(D), kernel_size, power, margin, tiny=np.finfo(np.float64).tiny)
    return istft(Mh * D, len(y)), istft(Mp * D, len(y))


def rms_power(y, frame_length, hop, center=True):
    """(librosa.feature.rms(constant padding))^2 per frame, as the reference squares it.  center=False frames the
    unpadded signal: 1 + (L - frame_length) // hop frames."""
    y = np.asarray(y, dtype=np.float64)
    if center:
        y = np.pad(y, frame_length // 2, mode="constant")
    T = 1 + (len(y) - frame_length) // hop
    idx = np.arange(frame_length)[None, :] + hop * np.arange(T)[:, None]
    return np.sqrt(np.mean(y[idx] ** 2, axis=1)) ** 2


def hnr_from_components(yh, yp, frame_length=2048, hop_length=None, center=True):
    hop = hop_length if hop_length is not None else frame_length // 4
    ph = rms_power(yh, frame_length, hop, center)
    pp = rms_power(yp, frame_length, hop, center)
    n = min(len(ph), len(pp))
    ph, pp = ph[:n], pp[:n]
    out = np.full(n, np.nan)
    both = (pp > EPSILON) & (ph > EPSILON)
    out[both] = 10 * np.log10(ph[both] / pp[both])
    out[(ph > EPSILON) & (pp <= EPSILON)] = 80.0
    out[(ph <= EPSILON) & (pp > EPSILON)] = -80.0
    return out, ph, pp


def harmonic_to_noise_ratio(y, frame_length=2048, hop_length=None, harmonic_margin=1.0, percussive_margin=1.0,
                            power=2.0):
    yh, yp = hpss(y, 31, power, (harmonic_margin, percussive_margin))
    return hnr_from_components(yh, yp, frame_length, hop_length)[0]


def sine(sr=22050, f=440.0, seconds=1.0, amp=0.7):
    """The reference test's sine fixture."""
    return amp * np.sin(2 * np.pi * f * np.arange(int(sr * seconds)) / sr)


def clicks(sr=22050, times=(0.2, 0.4, 0.6, 0.8), length=22050, click_duration=0.05, click_freq=1000.0):
    """librosa.clicks as the reference test's clicks fixture calls it: a click_freq tone decaying from 1 to 2^-10."""
    n = int(np.round(sr * click_duration))
    c = np.logspace(0, -10, num=n, base=2.0) * np.sin(2 * np.pi * click_freq / sr * np.arange(n))
    y = np.zeros(length)
    for s in (np.floor(np.asarray(times) * sr)).astype(int):
        m = min(n, length - s)
        y[s:s + m] += c[:m]
    return y
