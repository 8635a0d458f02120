"""Device-backed mirror of sygnals/core/audio/effects/utility.py: adjust_gain (:22-55, `syg_fx_mix_f32`),
noise_reduction_spectral (:59-131: `syg_stft2048_c2c_f32` of the clip and of its noise segment, `syg_spectral_gate_f32`,
`syg_istft2048_f32` with the gain as its mask), transient_shaping_hpss (:136-183: ops.hpss, then the two WAVEFORMS mixed
by `syg_fx_mix_f32`) and stereo_widening_midside (:188-253, `syg_fx_midside_f32`).  The two spectral effects call librosa
in the reference; librosa is not a dependency and the float64 restatement of tests/effects_ref.py is their contract."""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np

from .... import ops
from ._common import host, row

logger = logging.getLogger(__name__)


# ------------------------------------------------------------------ gain
def adjust_gain_batch(y, gain_db: float):
    """Rows y [B, L] (float32 device tensor) -> [B, L] scaled by 10^(gain_db / 20)."""
    return ops.fx_mix(y, None, 10.0 ** (gain_db / 20.0))


def adjust_gain(y, gain_db: float) -> np.ndarray:
    if not isinstance(y, np.ndarray):
        raise ValueError("Input audio data must be a NumPy array.")
    logger.info(f"Adjusting gain by {gain_db:.2f} dB.")
    if y.size == 0:
        return y.astype(np.float64)
    rows = y.reshape(-1, y.shape[-1]) if y.ndim > 1 else y[None, :]
    out = adjust_gain_batch(ops.to_device_f32(rows), gain_db)
    return out.cpu().numpy().astype(np.float64).reshape(y.shape)


# ------------------------------------------------------------------ spectral noise reduction
def _gate_args(n_samples, sr, noise_profile_duration, reduction_amount, n_fft, hop_length):
    if noise_profile_duration <= 0 or noise_profile_duration * sr > n_samples:
        raise ValueError("Invalid noise_profile_duration.")
    if reduction_amount < 0:
        raise ValueError("reduction_amount must be non-negative.")
    hop = hop_length if hop_length is not None else n_fft // 4
    if n_fft != 2048 or hop != 512:
        raise ValueError(f"noise_reduction_spectral: only n_fft=2048 with hop_length 512 is offloaded (got n_fft={n_fft}, "
                         f"hop_length={hop})")
    noise_samples = int(noise_profile_duration * sr)
    if noise_samples < 1:
        raise ValueError(f"noise_reduction_spectral: the noise profile holds no sample (noise_profile_duration="
                         f"{noise_profile_duration} at sr={sr})")
    return noise_samples


def noise_reduction_spectral_batch(y, sr: int, noise_profile_duration: float = 0.5, reduction_amount: float = 1.0,
                                   n_fft: int = 2048, hop_length: Optional[int] = None):
    """Clips y [B, L] (float32 device tensor) -> [B, L]; every clip's first int(noise_profile_duration sr) samples are
    its noise profile (a strided view, no copy)."""
    if y.dim() != 2:
        raise ValueError("Input audio batch must be a 2D array [B, L].")
    ns = _gate_args(y.shape[1], sr, noise_profile_duration, reduction_amount, n_fft, hop_length)
    D = ops.stft2048_c2c(y, 512, True, "hann", 2048)
    Dn = ops.stft2048_c2c(y[:, :ns], 512, True, "hann", 2048)
    G = ops.spectral_gate(D, Dn, reduction_amount)
    return ops.istft2048(D, 512, y.shape[1], True, "hann", 2048, mask=G)


def noise_reduction_spectral(y, sr: int, noise_profile_duration: float = 0.5, reduction_amount: float = 1.0,
                             n_fft: int = 2048, hop_length: Optional[int] = None) -> np.ndarray:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio 'y' must be 1D for spectral noise reduction.")
    _gate_args(len(y), sr, noise_profile_duration, reduction_amount, n_fft, hop_length)
    logger.info(f"Applying spectral noise reduction: profile_dur={noise_profile_duration}s, reduction={reduction_amount}")
    return host(noise_reduction_spectral_batch(row(y), sr, noise_profile_duration, reduction_amount, n_fft, hop_length))


# ------------------------------------------------------------------ transient shaping
def transient_shaping_hpss_batch(y, sr: int, percussive_scale: float = 1.0, harmonic_margin=1.0, percussive_margin=1.0):
    """Clips y [B, L] (float32 device tensor) -> [B, L]: y_harm + percussive_scale y_perc."""
    if y.dim() != 2:
        raise ValueError("Input audio batch must be a 2D array [B, L].")
    yh, yp = ops.hpss(y, margin=(harmonic_margin, percussive_margin))
    return ops.fx_mix(yh, yp, 1.0, percussive_scale)


def transient_shaping_hpss(y, sr: int, percussive_scale: float = 1.0, harmonic_margin=1.0, percussive_margin=1.0
                           ) -> np.ndarray:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("Input audio 'y' must be 1D for HPSS transient shaping.")
    logger.info(f"Applying transient shaping (HPSS): percussive_scale={percussive_scale}")
    return host(transient_shaping_hpss_batch(row(y), sr, percussive_scale, harmonic_margin, percussive_margin))


# ------------------------------------------------------------------ mid / side
def stereo_widening_midside_batch(y, width_factor: float = 1.5):
    """Stereo clips y [B, 2, L] (float32 device tensor) -> [B, 2, L]."""
    if width_factor < 0:
        raise ValueError("width_factor must be non-negative.")
    return ops.fx_midside(y, width_factor)


def stereo_widening_midside(y, width_factor: float = 1.5) -> np.ndarray:
    if not isinstance(y, np.ndarray) or y.ndim != 2 or y.shape[0] != 2:
        raise ValueError("Input audio 'y' must be a 2-channel NumPy array with shape (2, n_samples) for stereo widening.")
    if width_factor < 0:
        raise ValueError("width_factor must be non-negative.")
    logger.info(f"Applying Mid/Side stereo widening: width_factor={width_factor}")
    if y.shape[1] == 0:
        return y.astype(np.float64)
    out = stereo_widening_midside_batch(ops.to_device_f32(y[None]), width_factor)
    return out[0].cpu().numpy().astype(np.float64)
