"""Device-backed mirror of sygnals/core/audio/effects/compression.py: simple_dynamic_range_compression (:14-64) on
`syg_fx_compress_f32`."""
from __future__ import annotations

import logging

import numpy as np

from .... import ops
from ._common import host, one_d, row

logger = logging.getLogger(__name__)


def _check(threshold, ratio):
    if not 0.0 <= threshold <= 1.0:
        raise ValueError("Threshold must be between 0.0 and 1.0.")
    if ratio < 1.0:
        raise ValueError("Compression ratio must be >= 1.0.")


def simple_dynamic_range_compression_batch(y, threshold: float = 0.8, ratio: float = 4.0):
    """Clips y [B, L] (float32 device tensor) -> [B, L]."""
    _check(threshold, ratio)
    return ops.fx_compress(y, threshold, ratio)


def simple_dynamic_range_compression(y, threshold: float = 0.8, ratio: float = 4.0) -> np.ndarray:
    y = one_d(y)
    _check(threshold, ratio)
    logger.debug(f"Applying simple compression: threshold={threshold}, ratio={ratio}")
    if y.size == 0:
        return np.zeros(0, dtype=np.float64)
    return host(simple_dynamic_range_compression_batch(row(y), threshold, ratio))
