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
detect_onsets (:555-619; librosa 0.10 onset_detect, parity unpinned: the float64 restatement of tests/onset_ref.py is the
contract) takes the mel power from the mel front end of the frame length and runs the spectral flux, the normalisation,
peak_pick and the backtracking on the device (`syg_onset_strength_f32`, `syg_onset_peaks_f32`); get_basic_audio_metrics
(:508-551) takes its two clip totals from `syg_clip_metrics_f32`.
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
                                win_length: Optional[int] = None, center: bool = True, threshold: Optional[float] = None):
    """Batched fundamental_frequency of clips y [B, L] (a float32 device tensor or an array): device tensors
    (times [T] float64 on the host, f0 [B, T] with NaN unvoiced, voiced_flag [B, T] float32 0 / 1, voiced_probs [B, T]).
    method 'cepstrum' (not in the reference; tests/cepstrum_ref.py is its contract) takes the peak of the real cepstrum of
    every hann frame between the quefrencies sr / fmax and sr / fmin; a frame is voiced when the peak reaches `threshold`
    (default 0.13), and voiced_probs equals voiced_flag.  Any frame length is served (2048 by the fused kernel)."""
    fmin, fmax, hop = _pitch_defaults(fmin, fmax, hop_length)
    if method not in ("pyin", "yin", "cepstrum"):
        raise ValueError(f"Unsupported pitch estimation method: {method}. Choose 'pyin', 'yin' or 'cepstrum'.")
    if threshold is not None and method != "cepstrum":
        raise TypeError("fundamental_frequency: threshold belongs to method='cepstrum'")
    if method == "cepstrum":
        from ... import _cepstrum as CP
        if win_length is not None:
            raise TypeError("fundamental_frequency: method='cepstrum' windows the whole frame (no win_length)")
        CP.quefrency_range(sr, fmin, fmax, int(frame_length))         # refused before a copy
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
        f0, voiced, _ = ops.pitch_cepstrum(y, sr, fmin, fmax, frame_length, hop if hop is not None else 512, center,
                                           threshold=CP.THRESHOLD if threshold is None else float(threshold))
        vf = voiced.float()
        vp = vf
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
    allowed = {"frame_length", "win_length", "center", "threshold"}
    if set(kwargs) - allowed:
        raise TypeError(f"fundamental_frequency: unsupported librosa arguments on the device backend: "
                        f"{sorted(set(kwargs) - allowed)}")
    if method not in ("pyin", "yin", "cepstrum"):
        raise ValueError(f"Unsupported pitch estimation method: {method}. Choose 'pyin', 'yin' or 'cepstrum'.")
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


# ------------------------------------------------------------------ global metrics, onsets
def get_basic_audio_metrics(y, sr: int):
    logger.debug("Calculating basic global audio metrics.")
    try:
        y = np.asarray(y)
        if y.ndim > 1:
            logger.warning("Input signal is multi-channel. Converting to mono for global RMS/peak calculation.")
            # the shorter axis is taken for the channels
            y_mono = (np.mean(y, axis=0) if y.shape[0] < y.shape[1] else np.mean(y, axis=1)).astype(np.float64)
        else:
            y_mono = y
        duration_seconds = y.shape[-1] / float(sr)         # librosa.get_duration(y=y): samples along the last axis
        rms_global = peak_amplitude = 0.0
        if y_mono.size > 0:
            ss, pk = ops.clip_metrics(ops.to_device_f32(y_mono[None, :]))[0].cpu().numpy().astype(np.float64)
            rms_global = np.sqrt(ss / y_mono.size)
            peak_amplitude = pk
        return {"duration_seconds": float(duration_seconds), "rms_global": float(rms_global),
                "peak_amplitude": float(peak_amplitude)}
    except Exception as e:
        logger.error(f"Error calculating basic audio metrics: {e}")
        raise


_PEAK_KWARGS = ("pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait")


def _peak_defaults(sr, hop_length, kwargs):
    """onset_detect's peak_pick defaults, in frames: each is (c * sr) // hop_length, a float floor division."""
    pk = {"pre_max": 0.03 * sr // hop_length, "post_max": 0.00 * sr // hop_length + 1,
          "pre_avg": 0.10 * sr // hop_length, "post_avg": 0.10 * sr // hop_length + 1,
          "wait": 0.03 * sr // hop_length, "delta": 0.07}
    pk.update({k: kwargs[k] for k in _PEAK_KWARGS if k in kwargs})
    for k in _PEAK_KWARGS:
        if pk[k] < 0:
            raise ValueError(f"{k} must be non-negative")
    for k in ("post_max", "post_avg"):
        if pk[k] <= 0:
            raise ValueError(f"{k} must be positive")
    for k in _PEAK_KWARGS:
        if k != "delta":
            if int(pk[k]) != pk[k]:
                raise ValueError(f"{k}={pk[k]} must be an integer number of frames")
            pk[k] = int(pk[k])
    return pk


def _as_clips(y):
    if hasattr(y, "is_cuda"):
        y = y if (y.is_cuda and y.dtype == ops.torch.float32) else ops.to_device_f32(y)
    else:
        y = ops.to_device_f32(np.atleast_2d(np.asarray(y)))
    if y.dim() != 2:
        raise ValueError("Input audio batch must be a 2D array [B, L].")
    return y


def onset_strength_batch(y, sr: int, n_fft: int = 2048, hop_length: int = 512, n_mels: int = 128, fmin: float = 0.0,
                         fmax: Optional[float] = None, lag: int = 1, max_size: int = 1, center: bool = True,
                         detrend: bool = False, feature=None, aggregate=None):
    """librosa.onset.onset_strength of clips y [B, L] (a float32 device tensor or an array) -> float32 [B, T] device
    tensor.  The log-mel matrix comes from whichever mel front end serves n_fft (`syg_onset_strength_f32` after it)."""
    if feature is not None or aggregate is not None:
        raise TypeError("onset_strength_batch: feature= / aggregate= callables are not offloaded on the device backend")
    from ..features import manager as M               # inside the function: the manager imports this package's users
    y = _as_clips(y)
    mel = M.mel_power_batch(y, sr, n_fft, hop_length, center, "hann", n_mels, fmin, fmax)
    if not isinstance(lag, (int, np.integer)) or lag < 1:
        raise ValueError("lag must be a positive integer")
    if not isinstance(max_size, (int, np.integer)) or max_size < 1:
        raise ValueError("max_size must be a positive integer")
    pad = lag + (n_fft // (2 * hop_length) if center else 0)
    Tn = mel.shape[2]
    if Tn <= lag:
        # no frame has a frame `lag` before it: the flux is empty and librosa returns its padding alone (the C entry
        # refuses lag >= T, so the mirror answers before the call)
        return ops.torch.zeros((mel.shape[0], Tn if center else pad), dtype=ops.torch.float32, device=mel.device)
    T_out = Tn if center else None
    return ops.onset_strength(mel, lag, max_size, pad, T_out, detrend=detrend)


def detect_onsets_batch(y, sr: int, hop_length: int = 512, backtrack: bool = False, energy=None,
                        normalize: bool = True, **kwargs: Any):
    """Batched detect_onsets of clips y [B, L] -> (frames [B, T] int32: each clip's onset frames in ascending order,
    -1 beyond them; count [B] int32), device tensors (`syg_onset_peaks_f32` on onset_strength_batch)."""
    if set(kwargs) - set(_PEAK_KWARGS):
        raise TypeError(f"detect_onsets: unsupported librosa arguments on the device backend: "
                        f"{sorted(set(kwargs) - set(_PEAK_KWARGS))}")
    pk = _peak_defaults(sr, hop_length, kwargs)
    env = onset_strength_batch(y, sr, hop_length=hop_length)
    if energy is not None and not hasattr(energy, "is_cuda"):
        energy = ops.to_device_f32(np.atleast_2d(np.asarray(energy)))
    return ops.onset_peaks(env, normalize=normalize, backtrack=backtrack, energy=energy, **pk)


def detect_onsets(y=None, *, sr: Optional[int] = None, onset_envelope=None, hop_length: int = 512,
                  units: str = "frames", **kwargs: Any):
    if y is None and onset_envelope is None:
        raise ValueError("Either audio time series 'y' or 'onset_envelope' must be provided.")
    if y is not None and sr is None:
        raise ValueError("Sampling rate 'sr' must be provided when using time series 'y'.")
    if units in ["samples", "time"] and sr is None:
        raise ValueError(f"Sampling rate 'sr' is required when units='{units}'.")
    logger.debug(f"Detecting onsets: units={units}, hop_length={hop_length}, kwargs={kwargs}")
    allowed = set(_PEAK_KWARGS) | {"backtrack", "energy", "normalize"}
    if set(kwargs) - allowed:
        raise TypeError(f"detect_onsets: unsupported librosa arguments on the device backend: "
                        f"{sorted(set(kwargs) - allowed)}")
    try:
        if sr is None:                   # an envelope without a rate: librosa's window defaults multiply sr
            raise TypeError("unsupported operand type(s) for *: 'float' and 'NoneType'")
        if units not in ("frames", "samples", "time"):
            raise ValueError(f"Invalid unit type: {units}")
        backtrack = bool(kwargs.get("backtrack", False))
        normalize = bool(kwargs.get("normalize", True))
        energy = kwargs.get("energy")
        peak = {k: kwargs[k] for k in _PEAK_KWARGS if k in kwargs}
        if onset_envelope is None:
            y = np.asarray(y)
            if y.ndim != 1:
                raise ValueError("Input audio data must be a 1D array.")
            if energy is not None:
                energy = np.asarray(energy)[None, :]
            frames, count = detect_onsets_batch(y[None, :], sr, hop_length, backtrack, energy, normalize, **peak)
        else:
            env = np.asarray(onset_envelope)
            if env.ndim != 1:
                raise ValueError("onset_envelope must be a 1D array.")
            pk = _peak_defaults(sr, hop_length, peak)
            if env.size == 0:
                frames = count = None
            else:
                if energy is not None:
                    energy = ops.to_device_f32(np.asarray(energy)[None, :])
                frames, count = ops.onset_peaks(ops.to_device_f32(env[None, :]), normalize=normalize,
                                                backtrack=backtrack, energy=energy, **pk)
        onsets = np.array([], dtype=np.int64) if frames is None else \
            frames[0, :int(count[0].item())].cpu().numpy().astype(np.int64)
        if units == "frames":
            return onsets
        samples = onsets * int(hop_length)
        if units == "samples":
            return samples.astype(np.int64, copy=False)
        return (samples / float(sr)).astype(np.float64, copy=False)
    except Exception as e:
        logger.error(f"Error detecting onsets: {e}")
        raise
