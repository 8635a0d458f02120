"""Device-backed mirror of sygnals/core/augment/noise.py: add_noise (:19-101) on `syg_fx_add_noise_f32`.  The noise is
the reference's seeded host draw, uploaded as float32; a caller of the batch form may pass device noise instead."""
from __future__ import annotations

import logging
import warnings
from typing import Optional

import numpy as np

from ... import ops
from ..audio.effects._common import host, one_d, row

logger = logging.getLogger(__name__)


def _check_type(noise_type: str, stacklevel: int) -> None:
    """The reference's noise types: 'pink' and 'brown' are its placeholders (white noise and a warning)."""
    if noise_type in ("gaussian", "white"):
        return
    if noise_type in ("pink", "brown"):
        text = f"{noise_type.capitalize()} noise generation is currently a placeholder (using white noise)."
        warnings.warn(text, UserWarning, stacklevel=stacklevel)
        logger.warning(text)
        return
    raise ValueError(f"Invalid noise_type: '{noise_type}'. Choose 'gaussian', 'white', 'pink', or 'brown'.")


def draw(shape, seed: Optional[int]) -> np.ndarray:
    """np.random.default_rng(seed).standard_normal(shape): row 0 of a batch is the single clip's draw."""
    return np.random.default_rng(seed).standard_normal(shape)


def add_noise_batch(y, snr_db, noise_type: str = "gaussian", seed: Optional[int] = None, noise=None):
    """Clips y [B, L] (float32 device tensor) -> [B, L]; snr_db a number or one per row.  noise: a float32 device tensor
    [B, L] to mix in; None draws it on the host from `seed` as the reference does."""
    _check_type(noise_type, 3)
    if noise is None:
        noise = ops.to_device_f32(draw(tuple(y.shape), seed), y.device)
    return ops.fx_add_noise(y, noise, snr_db)


def add_noise(y, snr_db: float, noise_type: str = "gaussian", seed: Optional[int] = None) -> np.ndarray:
    y = one_d(y, "Input audio data must be a 1D array for noise addition.")
    logger.info(f"Applying noise augmentation: type={noise_type}, SNR={snr_db:.2f} dB.")
    _check_type(noise_type, 3)
    if y.size == 0:
        return np.zeros(0, dtype=np.float64)
    return host(ops.fx_add_noise(row(y), ops.to_device_f32(draw((1, y.size), seed)), float(snr_db)))
