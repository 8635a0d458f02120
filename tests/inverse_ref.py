"""Float64 restatement of librosa 0.10 `griffinlim` and of `feature.inverse.{mfcc_to_mel, mel_to_stft}` (librosa is not a
dependency: this is the parity contract of syg_gl_project_f32 / syg_inv_dense_f32 and of
ops.griffinlim).  Spectra are frame-major [T, 1025] here, as on the device; hpss_ref's stft / istft take [1025, T].

mel_to_stft is the minimum-norm least-squares inverse clipped at zero (torchaudio's InverseMelScale), NOT librosa's NNLS:
that problem is underdetermined (128 equations, 1025 unknowns) and its answer depends on the solver's path."""
from __future__ import annotations

import numpy as np

from . import hpss_ref as H
from . import rng_ref as RNG

NB = 1025
TINY = float(np.finfo(np.float32).tiny)          # librosa.util.tiny of complex64


def alpha_of(momentum):
    """momentum / (1 + momentum), rounded once to float32 as the host rounds it."""
    return float(np.float32(momentum / (1.0 + momentum)))


def project(R, P, S, alpha):
    """D = S A / (|A| + tiny), A = R - alpha P (A = R without P); np.abs of a complex number is a hypot."""
    A = np.asarray(R, dtype=np.complex128)
    if P is not None:
        A = A - alpha * np.asarray(P, dtype=np.complex128)
    return np.asarray(S, dtype=np.float64) * A / (np.abs(A) + TINY)


def sums(R, S):
    """(sum (|R| - S)^2, sum S^2) over one clip."""
    S = np.asarray(S, dtype=np.float64)
    return float(np.sum((np.abs(np.asarray(R, dtype=np.complex128)) - S) ** 2)), float(np.sum(S ** 2))


def random_spectrum(seed, row, T):
    """The initial R of init="random": normals 2 (t 1025 + f) and 2 (t 1025 + f) + 1 of (seed, row), rounded to float32."""
    z = RNG.normals(seed, row, T * NB * 2).astype(np.float32).astype(np.float64).reshape(T, NB, 2)
    return z[..., 0] + 1j * z[..., 1]


def stft(y):
    return H.stft(y).T


def istft(D, length):
    return H.istft(np.asarray(D).T, length)


def default_length(T):
    return H.HOP * (T - 1)


def griffinlim(S, n_iter=32, momentum=0.99, R0=None, length=None, stft32=False):
    """S [T, 1025] -> (y [length], trace [n_iter]).  R0: the spectrum whose phases start the run (None: phases of 1).
    stft32: every rebuilt spectrum is rounded to float32, the least a float32 implementation must do -- the run that
    measures how far float32 alone moves the result."""
    S = np.asarray(S, dtype=np.float64)
    T = S.shape[0]
    length = default_length(T) if length is None else int(length)
    alpha = alpha_of(momentum)
    R = np.ones((T, NB), dtype=np.complex128) if R0 is None else np.asarray(R0, dtype=np.complex128)
    D = project(R, None, S, alpha)
    prev = None
    trace = np.zeros(n_iter)
    for i in range(n_iter):
        R = stft(istft(D, length))
        if stft32:
            R = R.astype(np.complex64).astype(np.complex128)
        a, b = sums(R, S)
        trace[i] = np.sqrt(a / b) if b > 0 else np.nan
        D = project(R, prev, S, alpha)
        prev = R
    return istft(D, length), trace


def tones_noise(L, k=0, sr=22050):
    """Tones plus noise: the signals of the float32-against-float64 experiment the contract's figures come from."""
    rng = np.random.default_rng(100 + k)
    n = np.arange(L)
    y = 0.5 * np.sin(2 * np.pi * (220.0 * (k + 1)) * n / sr) + 0.3 * np.sin(2 * np.pi * 1975.3 * n / sr + 0.4 * k)
    return y + 0.05 * rng.standard_normal(L)


# ------------------------------------------------------------------ dense inversions
def db_to_power(x, ref=1.0):
    with np.errstate(over="ignore"):
        return ref * np.power(10.0, 0.1 * np.asarray(x, dtype=np.float64))


def inv_dense(X, W, pre_ref=None, post=None, power=2.0, ref=1.0):
    """out [T, F] = post(W [F, M] @ pre(X [M, T])), with the bound's scale sum_m |W| |pre(X)| beside it.
    post: None, "root" (max(., 0)^(1 / power)) or "db" (ref 10^(. / 10))."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    Xp = db_to_power(X, pre_ref) if pre_ref is not None else X
    with np.errstate(invalid="ignore", over="ignore"):
        v = (W @ Xp).T
        scale = (np.abs(W) @ np.abs(Xp)).T
    if post == "root":
        v = np.maximum(v, 0.0) ** (1.0 / power)
    elif post == "db":
        v = db_to_power(v, ref)
    return v, scale


def idct_matrix(n_mfcc, n_mels, dct_type=2, lifter=0):
    """W [n_mels, n_mfcc] of mfcc_to_mel: the transpose of the orthonormal DCT's first n_mfcc rows, which is
    scipy's idct(n=n_mels) of the zero-padded coefficients, with librosa's lifter divided out."""
    import scipy.fft
    D = scipy.fft.dct(np.eye(n_mels), axis=0, type=dct_type, norm="ortho")[:n_mfcc]
    W = D.T.copy()
    if lifter > 0:
        W /= (1.0 + (lifter / 2.0) * np.sin(np.pi * np.arange(1, n_mfcc + 1) / lifter))[None, :]
    return W


def mfcc_to_mel(mfcc, n_mels=128, dct_type=2, ref=1.0, lifter=0):
    """mfcc [K, T] -> mel power [n_mels, T]."""
    W = idct_matrix(np.asarray(mfcc).shape[0], n_mels, dct_type, lifter)
    return db_to_power(W @ np.asarray(mfcc, dtype=np.float64), ref)


def mel_pinv(basis):
    return np.linalg.pinv(np.asarray(basis, dtype=np.float64))


def mel_to_stft(mel, basis, power=2.0):
    """mel [M, T], basis [M, F] -> S [F, T] = max(pinv(basis) mel, 0)^(1 / power)."""
    return np.maximum(mel_pinv(basis) @ np.asarray(mel, dtype=np.float64), 0.0) ** (1.0 / power)
