"""IIR (SOS) and FIR design (host, float64), zero-phase and causal application (device).

Mirror of sygnals/core/filters.py: design_butterworth_sos :22-83 (validation strings are
pinned by the reference's tests/test_filters.py:73-87), apply_sos_filter :85-115 and the
four convenience filters :119-211.  The design stays on the host in float64 (24
coefficients); filtering runs in sosfilt.hip for single signals and [B, L] batches.

Beyond the reference (its specification, section 3.5, lists them; its code has only the above): the other IIR families
(design_iir_sos = scipy.signal.iirfilter), causal filtering with state in and out (scipy.signal.sosfilt semantics,
sosfilt_causal.hip) and windowed FIR design and application (scipy.signal.firwin / lfilter).
"""
from __future__ import annotations

import logging
from typing import Tuple, Union

import numpy as np
from scipy.signal import bessel, butter, firwin, iirfilter

from .. import _tables as T
from .. import ops

logger = logging.getLogger(__name__)


def design_butterworth_sos(cutoff: Union[float, Tuple[float, float]], fs: float, order: int, filter_type: str):
    nyquist = 0.5 * fs
    if isinstance(cutoff, (int, float)):
        if not 0 < cutoff < nyquist:
            raise ValueError(f"Cutoff frequency ({cutoff} Hz) must be strictly between 0 and Nyquist ({nyquist} Hz).")
        wn = cutoff / nyquist
    elif isinstance(cutoff, tuple) and len(cutoff) == 2:
        low, high = cutoff
        if not (0 < low < nyquist and 0 < high < nyquist):
            raise ValueError(f"Both low ({low} Hz) and high ({high} Hz) cutoff frequencies must be strictly "
                             f"between 0 and Nyquist ({nyquist} Hz).")
        if low >= high:
            raise ValueError(f"Low cutoff ({low} Hz) must be less than high cutoff ({high} Hz).")
        wn = (low / nyquist, high / nyquist)
    else:
        raise TypeError("cutoff must be a float (for low/high pass) or a tuple of two floats (for band pass/stop).")
    logger.debug("Designing %s-order Butterworth %s filter, cutoff %s Hz, fs %s Hz", order, filter_type, cutoff, fs)
    return butter(order, wn, btype=filter_type, analog=False, output="sos").astype(np.float64, copy=False)


IIR_FAMILIES = ("butter", "cheby1", "cheby2", "ellip", "bessel")
BESSEL_NORMS = ("phase", "delay", "mag")


def _normalised_cutoff(cutoff, fs):
    """cutoff (Hz) -> scipy's Wn, behind design_butterworth_sos's checks and messages."""
    nyquist = 0.5 * fs
    if isinstance(cutoff, (int, float)):
        if not 0 < cutoff < nyquist:
            raise ValueError(f"Cutoff frequency ({cutoff} Hz) must be strictly between 0 and Nyquist ({nyquist} Hz).")
        return cutoff / nyquist
    if isinstance(cutoff, tuple) and len(cutoff) == 2:
        low, high = cutoff
        if not (0 < low < nyquist and 0 < high < nyquist):
            raise ValueError(f"Both low ({low} Hz) and high ({high} Hz) cutoff frequencies must be strictly "
                             f"between 0 and Nyquist ({nyquist} Hz).")
        if low >= high:
            raise ValueError(f"Low cutoff ({low} Hz) must be less than high cutoff ({high} Hz).")
        return (low / nyquist, high / nyquist)
    raise TypeError("cutoff must be a float (for low/high pass) or a tuple of two floats (for band pass/stop).")


def design_iir_sos(cutoff: Union[float, Tuple[float, float]], fs: float, order: int, filter_type: str, family: str = "butter",
                   rp=None, rs=None, norm: str = "phase"):
    """scipy.signal.iirfilter(order, Wn, rp, rs, btype, ftype=family, output='sos') behind design_butterworth_sos's cutoff
    checks.  family: 'butter', 'cheby1' (needs rp, dB of pass-band ripple), 'cheby2' (needs rs, dB of stop-band
    attenuation), 'ellip' (needs both), 'bessel' (norm: 'phase', 'delay' or 'mag')."""
    served = ("served: 'butter', 'cheby1' (with rp > 0), 'cheby2' (with rs > 0), 'ellip' (with rp > 0 and rs > 0), "
              "'bessel' (norm 'phase', 'delay' or 'mag')")
    if family not in IIR_FAMILIES:
        raise ValueError(f"Unknown filter family {family!r}; {served}.")
    need_rp, need_rs = family in ("cheby1", "ellip"), family in ("cheby2", "ellip")
    for name, val, need in (("rp", rp, need_rp), ("rs", rs, need_rs)):
        if need and (val is None or not np.isfinite(val) or val <= 0):
            raise ValueError(f"Family {family!r} needs {name} > 0 dB (got {val}); {served}.")
    if family == "bessel" and norm not in BESSEL_NORMS:
        raise ValueError(f"Unknown Bessel norm {norm!r}; {served}.")
    wn = _normalised_cutoff(cutoff, fs)
    logger.debug("Designing %s-order %s %s filter, cutoff %s Hz, fs %s Hz", order, family, filter_type, cutoff, fs)
    if family == "bessel":                      # (iirfilter's own 'bessel' is the phase norm; the others go through bessel())
        sos = bessel(order, wn, btype=filter_type, analog=False, output="sos", norm=norm)
    else:
        sos = iirfilter(order, wn, rp=rp if need_rp else None, rs=rs if need_rs else None, btype=filter_type, analog=False,
                        ftype=family, output="sos")
    return sos.astype(np.float64, copy=False)


def design_fir(numtaps: int, cutoff, fs: float, window="hamming", pass_zero=True) -> np.ndarray:
    """scipy.signal.firwin(numtaps, cutoff, window=window, pass_zero=pass_zero, fs=fs): windowed-sinc FIR taps (float64)."""
    return firwin(numtaps, cutoff, window=window, pass_zero=pass_zero, fs=fs).astype(np.float64, copy=False)


def _steady_state(sos: np.ndarray) -> np.ndarray:
    """Per-section DF2T state for a unit step input (what scipy.signal.sosfilt_zi returns)."""
    zi = np.zeros((sos.shape[0], 2))
    gain = 1.0
    for s, (b0, b1, b2, a0, a1, a2) in enumerate(sos):
        b0, b1, b2, a1, a2 = b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0
        # z0 = b1 - a1*y + z1, z1 = b2 - a2*y with y = b0 + z0 at steady state for x = 1
        y = (b0 + b1 + b2) / (1.0 + a1 + a2)
        z1 = b2 - a2 * y
        z0 = b1 - a1 * y + z1
        zi[s] = gain * np.array([z0, z1])
        gain *= y
    return zi


def sosfilt_zi(sos) -> np.ndarray:
    """scipy.signal.sosfilt_zi(sos): the [n_sections, 2] states of the cascade's step response at rest.  Scaled by a row's
    first sample it starts a causal filter without a transient for a row that begins at a constant level."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("Input sos must be a 2D array with shape (n_sections, 6).")
    return _steady_state(sos)


def apply_sos_filter_causal_batch(sos, data, zi=None, return_state: bool = False):
    """[B, L] float32 device tensor (or array) -> causally filtered device tensor, scipy.signal.sosfilt semantics.
    zi: [B, n_sections, 2] float64 states (device tensor or array; one [n_sections, 2] array serves every row), None for
    rest.  return_state=True also returns zf [B, n_sections, 2] float64 on the device: the next block's zi."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("Input sos must be a 2D array with shape (n_sections, 6).")
    x = data if hasattr(data, "is_cuda") else ops.to_device_f32(np.asarray(data))
    if x.dim() != 2:
        raise ValueError("Batched input must have shape [B, L].")
    if zi is not None and not hasattr(zi, "is_cuda"):
        z = np.asarray(zi, dtype=np.float64)
        if z.ndim == 2:
            z = np.broadcast_to(z[None], (x.shape[0],) + z.shape)
        import torch
        zi = torch.from_numpy(np.ascontiguousarray(z)).to(x.device)
    return ops.sosfilt(x, sos, zi=zi, return_state=return_state)


def apply_sos_filter_causal(sos, data):
    """1-D float64 in and out: scipy.signal.sosfilt(sos, data) from rest."""
    data = np.asarray(data)
    sos = np.asarray(sos, dtype=np.float64)
    if data.ndim != 1:
        raise ValueError("Input data for filtering must be a 1D array.")
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("Input sos must be a 2D array with shape (n_sections, 6).")
    logger.debug("Applying SOS filter (causal) with %d sections.", sos.shape[0])
    y = apply_sos_filter_causal_batch(sos, data[None, :].astype(np.float32))
    return y[0].cpu().numpy().astype(np.float64)


def apply_fir_filter_batch(taps, data):
    """[B, L] float32 device tensor (or array) -> scipy.signal.lfilter(taps, 1, x) per row: the first L samples of the
    full convolution (convolve_batch), from rest."""
    from .dsp import convolve_batch
    x = data if hasattr(data, "is_cuda") else ops.to_device_f32(np.asarray(data))
    if x.dim() != 2:
        raise ValueError("Batched input must have shape [B, L].")
    t = np.asarray(taps, dtype=np.float64)
    if t.ndim != 1 or t.size == 0:
        raise ValueError("taps must be a non-empty 1D array.")
    k = ops.to_device_f32(t.astype(np.float32), x.device)
    return convolve_batch(x, k, "full")[:, :x.shape[1]].contiguous()


def apply_sos_filter_batch(sos, data):
    """[B, L] float32 device tensor (or array) -> filtered device tensor, sosfiltfilt semantics."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("Input sos must be a 2D array with shape (n_sections, 6).")
    x = data if hasattr(data, "is_cuda") else ops.to_device_f32(np.asarray(data))
    if x.dim() != 2:
        raise ValueError("Batched input must have shape [B, L].")
    return ops.sosfiltfilt(x, sos, _steady_state(sos), T.butter_padlen(sos))


def apply_sos_filter(sos, data):
    data = np.asarray(data)
    sos = np.asarray(sos, dtype=np.float64)
    if data.ndim != 1:
        raise ValueError("Input data for filtering must be a 1D array.")
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("Input sos must be a 2D array with shape (n_sections, 6).")
    logger.debug("Applying SOS filter (zero-phase) with %d sections.", sos.shape[0])
    y = apply_sos_filter_batch(sos, data[None, :].astype(np.float32))
    return y[0].cpu().numpy().astype(np.float64)


def low_pass_filter(data, cutoff: float, fs: float, order: int = 5):
    return apply_sos_filter(design_butterworth_sos(cutoff, fs, order, "lowpass"), data)


def high_pass_filter(data, cutoff: float, fs: float, order: int = 5):
    return apply_sos_filter(design_butterworth_sos(cutoff, fs, order, "highpass"), data)


def band_pass_filter(data, low_cutoff: float, high_cutoff: float, fs: float, order: int = 5):
    return apply_sos_filter(design_butterworth_sos((low_cutoff, high_cutoff), fs, order, "bandpass"), data)


def band_stop_filter(data, low_cutoff: float, high_cutoff: float, fs: float, order: int = 5):
    return apply_sos_filter(design_butterworth_sos((low_cutoff, high_cutoff), fs, order, "bandstop"), data)
