"""Device-backed mirror of sygnals/core/audio/effects/delay.py: apply_delay (:15-111) on `syg_fx_delay_f32`."""
from __future__ import annotations

import logging

import numpy as np

from .... import ops
from ._common import host, one_d, row

logger = logging.getLogger(__name__)


def _check(delay_time, feedback, wet_level, dry_level):
    if delay_time < 0:
        raise ValueError("delay_time must be non-negative.")
    if not 0.0 <= feedback < 1.0:
        raise ValueError("feedback gain must be between 0.0 and < 1.0.")
    if not 0.0 <= wet_level <= 1.0:
        raise ValueError("wet_level must be between 0.0 and 1.0.")
    if not 0.0 <= dry_level <= 1.0:
        raise ValueError("dry_level must be between 0.0 and 1.0.")


def apply_delay_batch(y, sr: int, delay_time: float = 0.5, feedback: float = 0.4, wet_level: float = 0.5,
                      dry_level: float = 1.0):
    """Clips y [B, L] (float32 device tensor) -> [B, L]; one parameter set for the batch."""
    _check(delay_time, feedback, wet_level, dry_level)
    delay_samples = int(delay_time * sr)
    if delay_samples <= 0:                      # the wet signal is the input itself
        logger.warning("Delay time is zero or negative. Returning dry signal scaled by (dry + wet).")
        return ops.fx_mix(y, None, dry_level + wet_level)
    return ops.fx_delay(y, delay_samples, feedback, wet_level, dry_level)


def apply_delay(y, sr: int, delay_time: float = 0.5, feedback: float = 0.4, wet_level: float = 0.5,
                dry_level: float = 1.0) -> np.ndarray:
    y = one_d(y)
    _check(delay_time, feedback, wet_level, dry_level)
    logger.info(f"Applying delay: time={delay_time}s, feedback={feedback}, wet={wet_level}, dry={dry_level}")
    if y.size == 0:
        return np.zeros(0, dtype=np.float64)
    return host(apply_delay_batch(row(y), sr, delay_time, feedback, wet_level, dry_level))
