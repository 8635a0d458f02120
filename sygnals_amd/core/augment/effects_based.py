"""Device-backed mirror of sygnals/core/augment/effects_based.py: time_stretch (:60-99), the same computation as
core/audio/effects/time_stretch.py.  pitch_shift (:16-58) is not mirrored (see the package docstring)."""
from __future__ import annotations

import logging

import numpy as np

from ..audio.effects.time_stretch import time_stretch as _time_stretch
from ..audio.effects.time_stretch import time_stretch_batch  # noqa: F401  (the batch form is the same function)

logger = logging.getLogger(__name__)


def time_stretch(y, rate: float) -> np.ndarray:
    logger.info(f"Applying time stretch augmentation: rate={rate}")
    return _time_stretch(y, rate)
