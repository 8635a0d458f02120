"""What the effect mirrors share: the 1-D check of the reference and the trip to the device and back."""
from __future__ import annotations

import numpy as np

from .... import ops


def one_d(y, message: str = "Input audio data must be a 1D array.") -> np.ndarray:
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(message)
    return y


def row(y: np.ndarray):
    """1-D host array -> [1, L] float32 device tensor."""
    return ops.to_device_f32(y[None, :])


def host(t) -> np.ndarray:
    """Row 0 of a device tensor -> float64 host array."""
    return t[0].cpu().numpy().astype(np.float64)
