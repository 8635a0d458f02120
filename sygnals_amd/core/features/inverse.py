"""Features back to audio on the device: Griffin-Lim (librosa 0.10 `griffinlim`) and the inversions of the mel and MFCC
maps (`librosa.feature.inverse`), over the kernels of csrc/griffinlim.hip and the inverse STFT.  The reference package has
no such functions, so there is nothing to mirror: the float64 restatement tests/inverse_ref.py is the contract.

Geometry is the inverse STFT's: n_fft 2048, hann, win_length 2048, hop 512, centred; anything else raises ValueError.
The single-clip functions take and return NumPy in librosa's orientation ([1025, T] magnitudes, [n_mels, T] mel power,
[n_mfcc, T] MFCC); the *_batch functions work on float32 device tensors in the device layouts (magnitudes frame-major
[B, T, 1025], mel and MFCC rows [B, M, T]) and stay on the device.

mel_to_stft is the minimum-norm least-squares inverse clipped at zero -- max(pinv(mel basis) mel, 0)^(1 / power),
torchaudio's InverseMelScale -- and NOT librosa's: librosa solves a non-negative least-squares problem by L-BFGS, which
with 128 equations and 1025 unknowns is underdetermined, so its answer depends on the solver's path."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import ops

__all__ = ["griffinlim", "griffinlim_batch", "mel_to_stft", "mel_to_stft_batch", "mel_to_audio", "mel_to_audio_batch",
           "mfcc_to_mel", "mfcc_to_mel_batch", "mfcc_to_audio", "mfcc_to_audio_batch"]

torch = ops.torch


def _rows(x, who: str, what: str, rows: Optional[int] = None):
    """One clip's feature matrix [rows, T] (librosa's orientation) as a float32 device tensor [1, rows, T]."""
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    if a.ndim != 2 or a.dtype.kind not in "fiu" or a.size == 0 or (rows is not None and a.shape[0] != rows):
        raise ValueError(f"{who}: {what} must be a real matrix [{rows if rows is not None else 'rows'}, T] "
                         f"(got shape {list(a.shape)}); the *_batch functions take batches")
    return lambda: torch.from_numpy(np.array(a[None], dtype=np.float32, order="C")).to(ops.require_gpu())


def _host(t) -> np.ndarray:
    return t[0].cpu().numpy()


def griffinlim_batch(S, n_iter: int = 32, momentum: float = 0.99, init="random", seed: int = 0, first_row: int = 0,
                     length: Optional[int] = None, angles=None, return_trace: bool = False, chunk: Optional[int] = None,
                     n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None, window="hann",
                     center: bool = True):
    """Clips [B, length] float32 on the device whose STFT magnitudes approach S [B, T, 1025] (ops.griffinlim)."""
    ops._gl_stft_args("griffinlim_batch", n_fft, hop_length, win_length, window, center)
    return ops.griffinlim(S, n_iter, momentum, init, seed, first_row, length, angles, return_trace, chunk)


def griffinlim(S, n_iter: int = 32, momentum: float = 0.99, init="random", seed: int = 0, length: Optional[int] = None,
               n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None, window="hann",
               center: bool = True) -> np.ndarray:
    """librosa.griffinlim of one magnitude spectrogram [1025, T]: float32 NumPy [length].  `seed` takes the place of
    librosa's random_state (the device's counter-based generator: the same seed gives the same clip)."""
    who = "griffinlim"
    ops._gl_stft_args(who, n_fft, hop_length, win_length, window, center)
    dev = _rows(S, who, "S", 1025)
    ops.gl_alpha(momentum)
    return _host(ops.griffinlim(dev().transpose(1, 2).contiguous(), n_iter, momentum, init, seed, 0, length))


def mel_to_stft_batch(mel, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, fmin: float = 0.0, fmax=None):
    """Mel power rows [B, n_mels, T] -> magnitudes [B, T, 1025] on the device (ops.mel_to_stft)."""
    return ops.mel_to_stft(mel, sr, n_fft, power, fmin, fmax)


def mel_to_stft(M, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, fmin: float = 0.0, fmax=None) -> np.ndarray:
    """One mel power spectrogram [n_mels, T] -> magnitudes [1025, T] (the clipped minimum-norm inverse: see above)."""
    ops._gl_stft_args("mel_to_stft", n_fft)
    return _host(ops.mel_to_stft(_rows(M, "mel_to_stft", "M")(), sr, n_fft, power, fmin, fmax)).T


def mel_to_audio_batch(mel, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, fmin: float = 0.0, fmax=None,
                       n_iter: int = 32, momentum: float = 0.99, seed: int = 0, first_row: int = 0,
                       length: Optional[int] = None):
    """Mel power rows [B, n_mels, T] -> clips [B, length] on the device (ops.mel_to_audio)."""
    return ops.mel_to_audio(mel, sr, n_fft, power, fmin, fmax, n_iter, momentum, seed, first_row, length)


def mel_to_audio(M, sr: float = 22050, n_fft: int = 2048, power: float = 2.0, fmin: float = 0.0, fmax=None, n_iter: int = 32,
                 momentum: float = 0.99, seed: int = 0, length: Optional[int] = None) -> np.ndarray:
    """One mel power spectrogram [n_mels, T] -> float32 NumPy [length]."""
    ops._gl_stft_args("mel_to_audio", n_fft)
    ops.gl_alpha(momentum)
    return _host(ops.mel_to_audio(_rows(M, "mel_to_audio", "M")(), sr, n_fft, power, fmin, fmax, n_iter, momentum, seed, 0, length))


def mfcc_to_mel_batch(mfcc, n_mels: int = 128, dct_type: int = 2, norm="ortho", ref: float = 1.0, lifter: float = 0):
    """MFCC rows [B, n_mfcc, T] -> mel power [B, n_mels, T] on the device (ops.mfcc_to_mel)."""
    return ops.mfcc_to_mel(mfcc, n_mels, dct_type, norm, ref, lifter)


def mfcc_to_mel(mfcc, n_mels: int = 128, dct_type: int = 2, norm="ortho", ref: float = 1.0, lifter: float = 0) -> np.ndarray:
    """librosa.feature.inverse.mfcc_to_mel of one MFCC matrix [n_mfcc, T] -> mel power [n_mels, T]."""
    dev = _rows(mfcc, "mfcc_to_mel", "mfcc")
    ops.idct_lifter_table(np.shape(mfcc)[0], n_mels, dct_type, norm, lifter)
    return _host(ops.mfcc_to_mel(dev(), n_mels, dct_type, norm, ref, lifter))


def mfcc_to_audio_batch(mfcc, n_mels: int = 128, dct_type: int = 2, norm="ortho", ref: float = 1.0, lifter: float = 0,
                        sr: float = 22050, fmin: float = 0.0, fmax=None, n_iter: int = 32, momentum: float = 0.99, seed: int = 0,
                        first_row: int = 0, length: Optional[int] = None):
    """MFCC rows [B, n_mfcc, T] -> clips [B, length] on the device (ops.mfcc_to_audio)."""
    return ops.mfcc_to_audio(mfcc, n_mels, dct_type, norm, ref, lifter, sr, fmin, fmax, n_iter, momentum, seed, first_row, length)


def mfcc_to_audio(mfcc, n_mels: int = 128, dct_type: int = 2, norm="ortho", ref: float = 1.0, lifter: float = 0,
                  sr: float = 22050, fmin: float = 0.0, fmax=None, n_iter: int = 32, momentum: float = 0.99, seed: int = 0,
                  length: Optional[int] = None) -> np.ndarray:
    """One MFCC matrix [n_mfcc, T] -> float32 NumPy [length]."""
    dev = _rows(mfcc, "mfcc_to_audio", "mfcc")
    ops.idct_lifter_table(np.shape(mfcc)[0], n_mels, dct_type, norm, lifter)
    ops.gl_alpha(momentum)
    return _host(ops.mfcc_to_audio(dev(), n_mels, dct_type, norm, ref, lifter, sr, fmin, fmax, n_iter, momentum, seed, 0, length))
