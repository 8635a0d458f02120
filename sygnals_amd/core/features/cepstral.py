"""Device-backed mirror of sygnals/core/features/cepstral.py (mfcc :20-120), and linear prediction (LPC), which that file's
feature table names as the next cepstral-family feature."""
from __future__ import annotations

import logging
from typing import Any, Dict, Optional

import numpy as np

from ... import _lpc, ops

logger = logging.getLogger(__name__)


def mfcc(y=None, sr: Optional[int] = None, S=None, n_mfcc: int = 13, dct_type: int = 2, norm: Optional[str] = "ortho",
         lifter: float = 0.0, **kwargs: Any) -> np.ndarray:
    """MFCCs [n_mfcc, T] float64 from a signal `y` or a log-power mel spectrogram `S`.

    With `y`, follows librosa.feature.mfcc(y=..): power_to_db(melspectrogram(y, sr, **kwargs))
    with ref=1.0 (the manager path uses ref=np.max instead, see manager.py:223).
    """
    if S is None and y is None:
        raise ValueError("Either audio time series 'y' or Mel spectrogram 'S' must be provided.")
    if S is None and sr is None:
        raise ValueError("Sampling rate 'sr' must be provided when calculating MFCCs from time series 'y'.")
    if S is not None and y is not None:
        logger.warning("Both 'y' and 'S' provided for MFCC calculation. Using pre-computed 'S'.")
    if lifter < 0:
        raise ValueError(f"MFCC lifter={lifter} must be a non-negative number")
    if S is not None:
        S = np.asarray(S)
        if S.ndim != 2:
            raise ValueError("S must be a 2D log-power mel spectrogram (n_mels x frames).")
        L = ops.to_device_f32(S[None])
        _, mf = ops.logmel_dct(L, n_mfcc, dct_type, norm, float(lifter), ref="db")   # DCT stage only
        return mf[0].cpu().numpy().astype(np.float64)
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio signal 'y' must be a 1D array.")
    n_fft = kwargs.get("n_fft", 2048)
    hop = kwargs.get("hop_length", 512)
    from .manager import mel_power_batch
    mel = mel_power_batch(ops.to_device_f32(y[None, :]), sr, n_fft, hop, kwargs.get("center", True),
                          kwargs.get("window", "hann"), kwargs.get("n_mels", 128), kwargs.get("fmin", 0.0),
                          kwargs.get("fmax"), kwargs.get("power", 2.0), win_length=kwargs.get("win_length"))
    _, mf = ops.logmel_dct(mel, n_mfcc, dct_type, norm, float(lifter), ref=1.0)
    return mf[0].cpu().numpy().astype(np.float64)


def _lpc_clips(y):
    """[B, L] on the device from a device tensor or a NumPy array; argument errors come first and need no device."""
    import torch
    if isinstance(y, torch.Tensor):
        if y.dim() != 2 or y.dtype != torch.float32:
            raise ValueError("y must be a float32 tensor [B, L] or a NumPy array [B, L]")
        return y
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError("y must be [B, L]")
    if y.size == 0:
        raise ValueError("y: empty input")
    return y


def lpc(y, order: int, method: str = "burg", window=None) -> np.ndarray:
    """Linear prediction coefficients a[0 .. order] (a[0] = 1) of a 1-D signal, float64: librosa.lpc(y, order=order) for
    method='burg' (Burg's recurrence, float64 on the device; no window unless one is given); method='autocorr' is the
    autocorrelation method (hann unless another window is given) with a Levinson-Durbin recursion.
    1 <= order <= min(64, len(y) - 2)."""
    _lpc.check_method(method)
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input signal 'y' must be a 1D array.")
    if y.size == 0:
        raise ValueError("y: empty input")
    _lpc.check_row(y.shape[0])
    _lpc.check_order(order, y.shape[0])
    a = ops.lpc_rows(ops.to_device_f32(y[None, :]), order, method, window)
    return a[0].cpu().numpy().astype(np.float64)


def lpc_batch(y, order: int, frame_length: int = 2048, hop_length: int = 512, center: bool = True, method: str = "burg",
              window=None, return_reflection: bool = False, return_error: bool = False):
    """LPC of every frame of the clips y [B, L] (a device tensor or a NumPy array) -> a [B, order + 1, T] float32 on the
    device, with the reflection coefficients [B, order, T] and the prediction error [B, T] when asked for
    (ops.lpc_frames)."""
    _lpc.check_method(method)
    N, hop = _lpc.check_frame(frame_length, hop_length)
    _lpc.check_order(order, N)
    y = _lpc_clips(y)
    if not hasattr(y, "is_cuda"):
        y = ops.to_device_f32(y)
    return ops.lpc_frames(y, order, N, hop, center, method, window, return_reflection, return_error)


def lpc_envelope_batch(a, err, n_fft: int = 2048, db: bool = False, amin: float = _lpc.AMIN):
    """The all-pole envelope err / |A|^2 of coefficients a [B, order + 1, T] and errors err [B, T] on the device ->
    [B, n_fft / 2 + 1, T] float32, in dB when db=True (ops.lpc_envelope)."""
    return ops.lpc_envelope(a, err, n_fft, db, amin)


CEPSTRAL_FEATURES: Dict[str, Any] = {"mfcc": mfcc, "lpc": lpc}


def mfcc_deltas_batch(y, sr, n_fft: int = 2048, hop_length: int = 512, n_mels: int = 128, n_mfcc: int = 13, deltas: int = 2,
                      width: int = 9, cmvn=None, variance: bool = True, mode: str = "interp", center: bool = True,
                      window="hann", fmin: float = 0.0, fmax=None, lifter: float = 0.0):
    """[B, L] clips -> [B, (deltas + 1) n_mfcc, T] on the device: ops.mfcc_batch followed by ops.feature_post (per-utterance
    CMVN `cmvn`: None, "global" or a sliding window; then delta and delta-delta of the statics).  With cmvn=None the static
    block equals mfcc_batch bit for bit."""
    yd = y if hasattr(y, "is_cuda") else ops.to_device_f32(np.atleast_2d(np.asarray(y, dtype=np.float32)))
    m = ops.mfcc_batch(yd, sr, n_fft=n_fft, hop=hop_length, n_mels=n_mels, n_mfcc=n_mfcc, center=center, window=window,
                       fmin=fmin, fmax=fmax, lifter=lifter)
    return ops.feature_post(m, cmvn=cmvn, variance=variance, deltas=deltas, width=width, mode=mode)
