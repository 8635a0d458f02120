"""Parametric and graphic equalizers: cascades of biquads run by one causal `ops.sosfilt` call.

The signatures are those of sygnals/core/audio/effects/equalizer.py (apply_graphic_eq :176-246, apply_parametric_eq
:248-320); the filters are this project's own definition, because the reference has none to mirror: its peaking stage
returns None by design and its shelves come out of an iirdesign call that raises inside a try block, so both functions
return their input.  What their docstrings promise is delivered here with the standard audio forms:

  peak, low_shelf, high_shelf   Audio EQ Cookbook (R. Bristow-Johnson) biquads; the shelves take the cookbook's Q
                                (default 1 / sqrt(2): the steepest shelf without overshoot)
  notch                         scipy.signal.iirnotch(freq, q, fs)

The EQ is causal (scipy.signal.sosfilt from rest).  A zero-phase EQ is not offered: filtering forward and backward
squares the magnitude response, i.e. doubles every gain in dB.  Stages whose |gain_db| is below 0.1 dB are skipped, as
the reference skips them; with no stage left the input is returned as a copy without a launch.
"""
from __future__ import annotations

import logging
import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
from scipy.signal import iirnotch

from .... import ops
from ._common import host, one_d, row

logger = logging.getLogger(__name__)

EQ_TYPES = ("peak", "low_shelf", "high_shelf", "notch")
MIN_GAIN_DB = 0.1          # stages below it are skipped (equalizer.py:64, :113)
SHELF_Q = 1.0 / math.sqrt(2.0)


def design_eq_sos(filter_type: str, fs: float, freq: float, gain_db: float = 0.0, q: Optional[float] = None):
    """One EQ stage as a biquad [1, 6] (float64, a0 = 1), or None for a peak / shelf whose |gain_db| is below 0.1 dB.

    filter_type: 'peak', 'low_shelf', 'high_shelf' (gain_db at the centre / the shelf's own end, gain_db / 2 at a shelf's
    freq) or 'notch' (gain_db ignored).  q: quality factor; None is 1.0 for peak and notch, 1 / sqrt(2) for the shelves."""
    if filter_type not in EQ_TYPES:
        raise ValueError(f"Unknown EQ filter type {filter_type!r}; served: 'peak', 'low_shelf', 'high_shelf', 'notch'.")
    nyquist = fs / 2.0
    if not 0 < freq < nyquist:
        raise ValueError(f"EQ frequency ({freq} Hz) must be between 0 and Nyquist ({nyquist} Hz).")
    if q is None:
        q = SHELF_Q if filter_type.endswith("shelf") else 1.0
    if not q > 0:
        raise ValueError("Q factor must be positive for peak/notch filters.")
    if filter_type == "notch":
        b, a = iirnotch(freq, q, fs)
        return np.concatenate([b, a])[None, :].astype(np.float64)
    if abs(gain_db) < MIN_GAIN_DB:
        return None
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * freq / fs
    cw, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    if filter_type == "peak":
        b = [1.0 + alpha * A, -2.0 * cw, 1.0 - alpha * A]
        a = [1.0 + alpha / A, -2.0 * cw, 1.0 - alpha / A]
    else:
        r = 2.0 * math.sqrt(A) * alpha
        sg = 1.0 if filter_type == "low_shelf" else -1.0          # the high shelf is the low shelf with cos -> -cos
        b = [A * ((A + 1.0) - sg * (A - 1.0) * cw + r), sg * 2.0 * A * ((A - 1.0) - sg * (A + 1.0) * cw),
             A * ((A + 1.0) - sg * (A - 1.0) * cw - r)]
        a = [(A + 1.0) + sg * (A - 1.0) * cw + r, -sg * 2.0 * ((A - 1.0) + sg * (A + 1.0) * cw),
             (A + 1.0) + sg * (A - 1.0) * cw - r]
    return (np.array([b + a], dtype=np.float64) / a[0])


def parametric_eq_sos(sr: float, params: List[Dict[str, Any]]) -> np.ndarray:
    """The stages of apply_parametric_eq stacked in order: [n, 6], n = 0 when every stage is skipped."""
    if not isinstance(params, list) or not all(isinstance(item, dict) for item in params):
        raise ValueError("params must be a list of dictionaries defining filter stages.")
    stages = []
    for i, st in enumerate(params):
        if "type" not in st or "freq" not in st:
            raise ValueError(f"EQ stage {i} missing required 'type' or 'freq' parameter.")
        sos = design_eq_sos(str(st["type"]).lower(), sr, st["freq"], st.get("gain_db", 0.0), st.get("q"))
        if sos is not None:
            stages.append(sos)
    return np.concatenate(stages) if stages else np.zeros((0, 6))


def graphic_eq_sos(sr: float, band_gains: List[Tuple[float, float]], q_factor: float = 1.414) -> np.ndarray:
    """One peaking stage per (center_frequency_hz, gain_db) band, in order: [n, 6]."""
    if not isinstance(band_gains, list) or not all(isinstance(item, tuple) and len(item) == 2 for item in band_gains):
        raise ValueError("band_gains must be a list of (center_frequency_hz, gain_db) tuples.")
    if q_factor <= 0:
        raise ValueError("q_factor must be positive.")
    stages = [design_eq_sos("peak", sr, f, g, q_factor) for f, g in band_gains if abs(g) >= MIN_GAIN_DB]
    return np.concatenate(stages) if stages else np.zeros((0, 6))


def _run(y, sos):
    if sos.shape[0] > 32:
        raise ValueError(f"The equalizer has {sos.shape[0]} stages; one call serves at most 32.")
    return ops.sosfilt(y, sos) if sos.shape[0] else y.clone()


def apply_parametric_eq_batch(y, sr: int, params: List[Dict[str, Any]]):
    """Clips y [B, L] (float32 device tensor) -> [B, L], one stage list for the batch."""
    return _run(y, parametric_eq_sos(sr, params))


def apply_graphic_eq_batch(y, sr: int, band_gains: List[Tuple[float, float]], q_factor: float = 1.414):
    """Clips y [B, L] (float32 device tensor) -> [B, L], one band list for the batch."""
    return _run(y, graphic_eq_sos(sr, band_gains, q_factor))


def _apply(y: np.ndarray, sos: np.ndarray) -> np.ndarray:
    if y.size == 0 or sos.shape[0] == 0:
        return y.astype(np.float64)            # (a copy)
    return host(_run(row(y), sos))


def apply_parametric_eq(y, sr: int, params: List[Dict[str, Any]]) -> np.ndarray:
    y = one_d(y)
    sos = parametric_eq_sos(sr, params)
    logger.info(f"Applying Parametric EQ: {len(params)} stages.")
    return _apply(y, sos)


def apply_graphic_eq(y, sr: int, band_gains: List[Tuple[float, float]], q_factor: float = 1.414) -> np.ndarray:
    y = one_d(y)
    sos = graphic_eq_sos(sr, band_gains, q_factor)
    logger.info(f"Applying Graphic EQ: {len(band_gains)} bands, Q={q_factor:.2f}")
    return _apply(y, sos)
