"""Device-backed mirror of sygnals/core/audio/effects/reverb.py: apply_reverb (:85-166).  The impulse response of
_generate_basic_ir (:16-83) is a seeded host computation in float64 (the same seed gives the reference's IR); the
convolution is the device's real-input FFT convolution (dsp.convolve_batch) and the dry / wet mix over the longer output
`syg_fx_mix_f32`."""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np

from .... import ops
from ...dsp import convolve_batch
from ._common import host, one_d, row

logger = logging.getLogger(__name__)

_TINY = 1e-9


def _generate_basic_ir(sr: int, decay_time: float = 0.5, seed: Optional[int] = None) -> np.ndarray:
    """Seeded white noise under an envelope that reaches -60 dB at decay_time, peak 1, int(1.5 sr decay_time) samples;
    [1.0] when that is one sample or fewer, decay_time < 1e-6, or the noise is all but zero."""
    if decay_time < 0:
        raise ValueError("decay_time must be non-negative.")
    n = max(1, int(sr * decay_time * 1.5))
    if decay_time < 1e-6 or n <= 1:
        return np.array([1.0], dtype=np.float64)
    noise = np.random.default_rng(seed).standard_normal(n).astype(np.float64)
    slope = -np.log(0.001) / (decay_time * sr + _TINY)
    ir = noise * np.exp(-slope * np.arange(n))
    peak = np.max(np.abs(ir))
    if not peak > _TINY:
        logger.warning("Generated IR is near zero, returning Dirac delta.")
        return np.array([1.0], dtype=np.float64)
    return ir / peak


def _check(wet_level, dry_level):
    if not 0.0 <= wet_level <= 1.0:
        raise ValueError("wet_level must be between 0.0 and 1.0.")
    if not 0.0 <= dry_level <= 1.0:
        raise ValueError("dry_level must be between 0.0 and 1.0.")


def apply_reverb_batch(y, sr: int, decay_time: float = 0.5, wet_level: float = 0.3, dry_level: float = 0.7,
                       ir_seed: Optional[int] = None):
    """Clips y [B, L] (float32 device tensor) -> [B, L + len(ir) - 1]; one impulse response for the batch."""
    _check(wet_level, dry_level)
    ir = _generate_basic_ir(sr, decay_time, seed=ir_seed)
    if len(ir) == 1 and np.isclose(ir[0], 1.0):
        return ops.fx_mix(y, None, dry_level + wet_level)
    wet = convolve_batch(y, ops.to_device_f32(ir[None, :]), "full")
    return ops.fx_mix(y, wet, dry_level, wet_level)


def apply_reverb(y, sr: int, decay_time: float = 0.5, wet_level: float = 0.3, dry_level: float = 0.7,
                 ir_seed: Optional[int] = None) -> np.ndarray:
    y = one_d(y)
    _check(wet_level, dry_level)
    logger.info(f"Applying reverb: decay={decay_time}s, wet={wet_level}, dry={dry_level}")
    if y.size == 0:
        raise ValueError("apply_reverb: empty input")
    return host(apply_reverb_batch(row(y), sr, decay_time, wet_level, dry_level, ir_seed))
