"""Device-backed mirror of sygnals/core/audio/effects/tremolo.py: apply_tremolo (:55-111) on `syg_fx_tremolo_f32`, the
LFO of _generate_lfo (:16-52) formed in float64 on the device."""
from __future__ import annotations

import logging

import numpy as np

from .... import ops
from ._common import host, one_d, row

logger = logging.getLogger(__name__)


def _check(rate, depth, shape):
    if not 0.0 <= depth <= 1.0:
        raise ValueError("Tremolo depth must be between 0.0 and 1.0.")
    if rate <= 0:
        raise ValueError("Tremolo rate must be positive.")
    if shape not in ["sine", "triangle", "square"]:
        raise ValueError("LFO shape must be 'sine', 'triangle', or 'square'.")


def apply_tremolo_batch(y, sr: int, rate: float = 5.0, depth: float = 0.5, shape: str = "sine"):
    """Clips y [B, L] (float32 device tensor) -> [B, L]; every clip starts at phase 0."""
    _check(rate, depth, shape)
    return ops.fx_tremolo(y, sr, rate, depth, shape)


def apply_tremolo(y, sr: int, rate: float = 5.0, depth: float = 0.5, shape: str = "sine") -> np.ndarray:
    y = one_d(y)
    _check(rate, depth, shape)
    logger.info(f"Applying Tremolo: rate={rate} Hz, depth={depth}, shape={shape}")
    if y.size == 0:
        return np.zeros(0, dtype=np.float64)
    return host(apply_tremolo_batch(row(y), sr, rate, depth, shape))
