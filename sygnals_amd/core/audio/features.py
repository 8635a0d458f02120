"""Device-backed mirror of sygnals/core/audio/features.py: zero_crossing_rate (:26-71) and rms_energy (:73-131).

The reference forwards both to librosa (`librosa.feature.zero_crossing_rate`: EDGE padding, threshold 1e-10,
first sample of a frame never counts; `librosa.feature.rms`: zero padding, or from a magnitude spectrogram with DC /
Nyquist halved).  Here one wave per frame computes them (`syg_frame_stats_f32`, `syg_rms_from_spec_f32`).
fundamental_frequency (:135-220; librosa 0.10 yin / pyin, parity unpinned: the float64 restatement of
tests/pitch_ref.py is the contract) runs the frame stage and the Viterbi decode on the device (`syg_pitch_frames_f32`,
`syg_pyin_viterbi_f32`); jitter (:319) and shimmer (:412) are host arithmetic on its f0 / voicing and on the device
rms_energy.  harmonic_to_noise_ratio (:225-316; librosa 0.10 effects.hpss, parity unpinned: the float64 restatement
of tests/hpss_ref.py is the contract) runs the STFT, the median-filter soft masks, both inverse STFTs and the per-frame
energy ratio on the device (`syg_stft2048_c2c_f32`, `syg_hpss_masks_f32`, `syg_istft2048_f32`, `syg_hnr_rows_f32`).
"""
from __future__ import annotations

import logging
import warnings
from typing import Any, Optional

import numpy as np

from ... import ops

logger = logging.getLogger(__name__)

_ROW_RMS, _ROW_ZCR = 7, 8


def zero_crossing_rate(y, frame_length: int = 2048, hop_length: int = 512, center: bool = True, **kwargs: Any):
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio data must be a 1D array.")
    if kwargs:
        raise TypeError(f"zero_crossing_rate: unsupported librosa arguments on the device backend: {sorted(kwargs)}")
    logger.debug(f"Calculating Zero Crossing Rate: frame={frame_length}, hop={hop_length}, center={center}")
    st = ops.frame_stats(ops.to_device_f32(y[None, :]), frame_length, hop_length, center, mask=1 << _ROW_ZCR)
    return st[0, _ROW_ZCR].cpu().numpy().astype(np.float64)


def rms_energy(y=None, *, S=None, frame_length: int = 2048, hop_length: int = 512, center: bool = True,
               pad_mode: str = "constant", **kwargs: Any):
    if S is None and y is None:
        raise ValueError("Either audio time series 'y' or magnitude spectrogram 'S' must be provided.")
    if y is not None and np.asarray(y).ndim != 1:
        raise ValueError("Input audio data 'y' must be a 1D array.")
    if S is not None and np.asarray(S).ndim != 2:
        raise ValueError("Input spectrogram 'S' must be a 2D array.")
    if kwargs:
        raise TypeError(f"rms_energy: unsupported librosa arguments on the device backend: {sorted(kwargs)}")
    logger.debug(f"Calculating RMS Energy: frame={frame_length}, hop={hop_length}, center={center}")
    if S is not None:                       # librosa ignores y when S is given
        Sm = np.asarray(S)                   # (the kernel squares the values: |S|^2 needs no abs on the host)
        if Sm.shape[0] != frame_length // 2 + 1:
            raise ValueError(f"Since S.shape[-2] is {Sm.shape[0]}, frame_length is expected to be "
                             f"{2 * Sm.shape[0] - 2} or {2 * Sm.shape[0] - 1}; found {frame_length}")
        out = ops.rms_from_spec(ops.to_device_f32(np.ascontiguousarray(Sm.T)), frame_length)
        return out.cpu().numpy().astype(np.float64)
    if pad_mode != "constant":
        raise ValueError("rms_energy: only pad_mode='constant' is offloaded")
    st = ops.frame_stats(ops.to_device_f32(np.asarray(y)[None, :]), frame_length, hop_length, center, mask=1 << _ROW_RMS)
    return st[0, _ROW_RMS].cpu().numpy().astype(np.float64)


_EPSILON = 1e-10


def _pitch_defaults(fmin, fmax, hop_length):
    from ... import _pitch as P
    return (P.C2 if fmin is None else float(fmin)), (P.C7 if fmax is None else float(fmax)), hop_length


def fundamental_frequency_batch(y, sr: int, fmin: Optional[float] = None, fmax: Optional[float] = None,
                                method: str = "pyin", hop_length: Optional[int] = None, frame_length: int = 2048,
                                win_length: Optional[int] = None, center: bool = True):
    """Batched fundamental_frequency of clips y [B, L] (a float32 device tensor or an array): device tensors
    (times [T] float64 on the host, f0 [B, T] with NaN unvoiced, voiced_flag [B, T] float32 0 / 1, voiced_probs [B, T])."""
    fmin, fmax, hop = _pitch_defaults(fmin, fmax, hop_length)
    y = y if hasattr(y, "is_cuda") else ops.to_device_f32(np.atleast_2d(np.asarray(y)))
    if y.dim() != 2:
        raise ValueError("Input audio batch must be a 2D array [B, L].")
    if method == "pyin":
        f0, vf, vp = ops.pitch_pyin(y, sr, fmin, fmax, frame_length, win_length, hop, center)
        vf = vf.float()
    elif method == "yin":
        f0 = ops.pitch_yin(y, sr, fmin, fmax, frame_length, win_length, hop, center)
        vf = _finite01(f0)
        vp = vf
    else:
        raise ValueError(f"Unsupported pitch estimation method: {method}. Choose 'pyin' or 'yin'.")
    hop_calc = hop if hop is not None else 512
    times = np.arange(f0.shape[1], dtype=np.float64) * hop_calc / sr
    return times, f0, vf, vp


def _finite01(t):
    return t.isfinite().float()


def fundamental_frequency(y, sr: int, fmin: Optional[float] = None, fmax: Optional[float] = None,
                          method: str = "pyin", hop_length: Optional[int] = None, **kwargs: Any):
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio data must be a 1D array.")
    logger.debug(f"Estimating Fundamental Frequency (Pitch) using {method}: fmin={fmin}, fmax={fmax}, hop={hop_length}")
    allowed = {"frame_length", "win_length", "center"}
    if set(kwargs) - allowed:
        raise TypeError(f"fundamental_frequency: unsupported librosa arguments on the device backend: "
                        f"{sorted(set(kwargs) - allowed)}")
    if method not in ("pyin", "yin"):
        raise ValueError(f"Unsupported pitch estimation method: {method}. Choose 'pyin' or 'yin'.")
    times, f0, vf, vp = fundamental_frequency_batch(y[None, :], sr, fmin, fmax, method, hop_length, **kwargs)
    return (times, f0[0].cpu().numpy().astype(np.float64), vf[0].cpu().numpy().astype(np.float64),
            vp[0].cpu().numpy().astype(np.float64))


def jitter(y, sr: int, f0=None, voiced_flag=None, method: str = "local_abs", f0_min: float = 75.0,
           f0_max: float = 600.0, hop_length: Optional[int] = None):
    warnings.warn("Jitter feature is an approximation based on frame-level F0 period differences.", UserWarning,
                  stacklevel=2)
    logger.warning("Jitter feature is an approximation based on frame-level F0 period differences.")
    if method != "local_abs":
        raise NotImplementedError(f"Jitter method '{method}' not implemented. Only 'local_abs' is available.")
    if f0 is None or voiced_flag is None:
        logger.warning("F0 or voiced_flag not provided. Calculating F0 internally using pyin.")
        hop_calc = hop_length if hop_length is not None else 512
        try:
            _, f0, voiced_flag, _ = fundamental_frequency(y, sr, fmin=f0_min, fmax=f0_max, method="pyin",
                                                          hop_length=hop_calc)
        except Exception as e:
            logger.error(f"Internal F0 calculation failed for Jitter: {e}")
            n = 1 + len(y) // hop_calc if hop_calc > 0 else 0
            return np.full(n, np.nan, dtype=np.float64)
    f0 = np.asarray(f0, dtype=np.float64)
    voiced_flag = np.asarray(voiced_flag, dtype=np.float64)
    if len(f0) != len(voiced_flag):
        raise ValueError("Length of f0 and voiced_flag must match.")
    n = len(f0)
    out = np.full(n, np.nan, dtype=np.float64)
    periods = np.full(n, np.nan, dtype=np.float64)
    ok = (voiced_flag > 0.5) & np.isfinite(f0) & (f0 >= f0_min) & (f0 <= f0_max)
    periods[ok] = 1.0 / f0[ok]
    diffs = np.abs(np.diff(periods))
    out[1:] = diffs
    out[1:][~np.isfinite(diffs)] = np.nan
    if n:
        out[0] = np.nan
    out[voiced_flag <= 0.5] = np.nan
    return out


def shimmer(y, sr: int, voiced_flag=None, method: str = "local_rms_rel", frame_length: int = 2048,
            hop_length: Optional[int] = None, center: bool = True):
    warnings.warn("Shimmer feature is an approximation based on frame-level relative RMS differences.", UserWarning,
                  stacklevel=2)
    logger.warning("Shimmer feature is an approximation based on frame-level relative RMS differences.")
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio 'y' must be 1D for shimmer calculation.")
    if method != "local_rms_rel":
        raise NotImplementedError(f"Shimmer method '{method}' not implemented. Only 'local_rms_rel' is available.")
    hop_calc = hop_length if hop_length is not None else frame_length // 4
    if hop_calc <= 0:
        raise ValueError("Hop length must be positive.")
    try:
        rms = rms_energy(y=y, frame_length=frame_length, hop_length=hop_calc, center=center)
    except Exception as e:
        logger.error(f"Internal RMS calculation failed for Shimmer: {e}")
        return np.full(1 + len(y) // hop_calc, np.nan, dtype=np.float64)
    if voiced_flag is None:
        logger.warning("voiced_flag not provided for Shimmer. Calculating F0 internally using pyin.")
        try:
            _, _, voiced_flag, _ = fundamental_frequency(y, sr, fmin=75.0, fmax=600.0, method="pyin", hop_length=hop_calc)
        except Exception as e:
            logger.error(f"Internal F0/voicing calculation failed for Shimmer: {e}")
            return np.full(len(rms), np.nan, dtype=np.float64)
    voiced_flag = np.asarray(voiced_flag, dtype=np.float64)
    n = min(len(rms), len(voiced_flag))
    if n == 0:
        return np.array([], dtype=np.float64)
    rms = rms[:n]
    vf = voiced_flag[:n]
    out = np.full(n, np.nan, dtype=np.float64)
    both = (vf[1:] > 0.5) & (vf[:-1] > 0.5)
    s = rms[1:] + rms[:-1]
    val = np.where(s > _EPSILON, 2.0 * np.abs(rms[1:] - rms[:-1]) / np.where(s > _EPSILON, s, 1.0), 0.0)
    out[1:][both] = val[both]
    return out


_HPSS_KWARGS = {"power", "n_fft", "win_length", "window", "center"}


def _hpss_kwargs(kwargs):
    if set(kwargs) - _HPSS_KWARGS:
        raise TypeError(f"harmonic_to_noise_ratio: unsupported librosa arguments on the device backend: "
                        f"{sorted(set(kwargs) - _HPSS_KWARGS)}")
    hk = dict(kwargs)
    # the STFT settings the device path supports are checked here, outside the reference's NaN path
    ops._hpss_stft_args(hk.get("n_fft", 2048), None, hk.get("win_length"), hk.get("window", "hann"),
                        hk.get("center", True))
    return hk


def harmonic_to_noise_ratio_batch(y, sr: int, frame_length: int = 2048, hop_length: Optional[int] = None,
                                  harmonic_margin=1.0, percussive_margin=1.0, **kwargs: Any):
    """Batched harmonic_to_noise_ratio of clips y [B, L] (a float32 device tensor or an array) -> float32 [B, T]
    device tensor with the reference's NaN / +-80 rules.  Errors raise (no NaN path)."""
    hk = _hpss_kwargs(kwargs)
    if hasattr(y, "is_cuda"):                # a torch tensor: moved to the device as float32 unless it is already
        y = y if (y.is_cuda and y.dtype == ops.torch.float32) else ops.to_device_f32(y)
    else:
        y = ops.to_device_f32(np.atleast_2d(np.asarray(y)))
    if y.dim() != 2:
        raise ValueError("Input audio batch must be a 2D array [B, L].")
    hop_calc = hop_length if hop_length is not None else frame_length // 4
    yh, yp = ops.hpss(y, kernel_size=31, power=hk.get("power", 2.0), margin=(harmonic_margin, percussive_margin),
                      win_length=hk.get("win_length"), window=hk.get("window", "hann"), center=hk.get("center", True),
                      n_fft=hk.get("n_fft", 2048))
    return ops.hnr_rows(yh, yp, frame_length, hop_calc, center=True)


def harmonic_to_noise_ratio(y, sr: int, frame_length: int = 2048, hop_length: Optional[int] = None,
                            harmonic_margin=1.0, percussive_margin=1.0, **kwargs: Any):
    warnings.warn("harmonic_to_noise_ratio feature is an approximation based on HPSS energy ratio.", UserWarning,
                  stacklevel=2)
    logger.warning("harmonic_to_noise_ratio feature is an approximation based on HPSS energy ratio.")
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio 'y' must be 1D for HPSS-based HNR.")
    _hpss_kwargs(kwargs)
    ops.require_gpu()
    hop_length_calc = hop_length if hop_length is not None else frame_length // 4
    try:
        out = harmonic_to_noise_ratio_batch(y[None, :], sr, frame_length, hop_length, harmonic_margin,
                                            percussive_margin, **kwargs)
        hnr_db = out[0].cpu().numpy().astype(np.float64)
        logger.debug(f"Calculated approximate HNR for {len(hnr_db)} frames.")
        return hnr_db
    except Exception as e:
        logger.error(f"Error calculating approximate HNR using HPSS: {e}")
        num_frames = 1 + len(y) // hop_length_calc if hop_length_calc > 0 else 0
        return np.full(num_frames, np.nan, dtype=np.float64)
