"""Device-backed mirror of sygnals/core/audio/effects/time_stretch.py: time_stretch (:15-48), librosa's phase vocoder
between `syg_stft2048_c2c_f32` and `syg_istft2048_f32` (`syg_phase_vocoder_f32`)."""
from __future__ import annotations

import logging

import numpy as np

from .... import ops
from ._common import host, one_d, row

logger = logging.getLogger(__name__)


def time_stretch_batch(y, rate: float):
    """Clips y [B, L] (float32 device tensor) -> [B, round(L / rate)]; one rate for the batch."""
    if rate <= 0:
        raise ValueError("Time stretch rate must be positive.")
    return ops.time_stretch(y, rate)


def time_stretch(y, rate: float) -> np.ndarray:
    y = one_d(y)
    if rate <= 0:
        raise ValueError("Time stretch rate must be positive.")
    logger.debug(f"Applying time stretch: rate={rate}")
    if y.size == 0 or int(round(y.size / rate)) == 0:
        return np.zeros(0, dtype=np.float64)
    return host(time_stretch_batch(row(y), rate))
