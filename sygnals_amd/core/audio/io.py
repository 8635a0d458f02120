"""Device-backed mirror of sygnals/core/audio/io.py: load_audio :38-102 (decode, mix down, cut, resample on load).

The reference loads through librosa with res_type='kaiser_best', which is resampy's tabulated filter; that method cannot
be pinned here and is not served.  The resampler here is the `scipy` method of the reference's spec,
scipy.signal.resample_poly, run on the device (core.dsp.resample; res_type='poly').  Decoding goes through
sygnals_amd.io.read_audio: WAV only.  The save_audio function of that module has no mirror."""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

from ... import io as sio
from ..dsp import resample_batch

logger = logging.getLogger(__name__)


def load_audio(file_path, sr: Optional[int] = None, mono: bool = True, offset: float = 0.0,
               duration: Optional[float] = None, res_type: str = "poly") -> Tuple[np.ndarray, int]:
    """(float64 samples, rate): shape (n,) if mono or the file has one channel, else (channels, n).  offset / duration are
    seconds at the file's native rate, cut before resampling; sr other than the native rate resamples on the device."""
    file_path = Path(file_path)
    if not file_path.exists():
        raise FileNotFoundError(f"Audio input file not found: {file_path}")
    if not file_path.is_file():
        raise ValueError(f"Input path is not a file: {file_path}")
    if res_type != "poly":
        raise ValueError(f"res_type={res_type!r} is not served: the reference's 'kaiser_best' (and 'kaiser_fast') is resampy's "
                         "tabulated filter, which this backend does not reproduce; the device resampler is "
                         "scipy.signal.resample_poly (res_type='poly')")
    if offset < 0 or (duration is not None and duration < 0):
        raise ValueError("offset and duration must not be negative")
    data, native = sio.read_audio(file_path)
    if mono and data.ndim == 2:
        data = data.mean(axis=0)
    start = int(offset * native)
    stop = None if duration is None else start + int(duration * native)
    data = data[..., start:stop]
    if sr is None or sr == native:
        return np.ascontiguousarray(data, dtype=np.float64), native
    if data.shape[-1] == 0:
        return np.ascontiguousarray(data, dtype=np.float64), int(sr)
    from ... import ops
    rows = ops.to_device_f32(np.atleast_2d(data))
    out = resample_batch(rows, native, sr).cpu().numpy().astype(np.float64)
    return (out[0] if data.ndim == 1 else out), int(sr)
