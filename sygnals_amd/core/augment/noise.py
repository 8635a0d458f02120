"""Device-backed mirror of sygnals/core/augment/noise.py: add_noise (:19-101) on `syg_fx_add_noise_f32`.  The noise is
the reference's seeded host draw, uploaded as float32; a caller of the batch form may pass device noise instead.

The `*_device*` functions draw the noise on the device instead (ops.randn: Philox4x32-10, a value depends on the seed, the
row and the sample index alone), where 'pink' and 'brown' are real power-law noise (ops.colored_noise) and no placeholder.
They are this package's own: another generator gives other samples than the reference's NumPy draw at the same seed."""
from __future__ import annotations

import logging
import warnings
from typing import Optional

import numpy as np

from ... import _rng, ops
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


# ------------------------------------------------------------------ noise drawn on the device
COLOR_EXPONENTS = {"gaussian": 0.0, "white": 0.0, "pink": 1.0, "brown": 2.0}
# Rows past this length are mixed from stored noise (ops.randn + ops.fx_add_noise) rather than by the generating kernel;
# shorter ones are generated in registers (ops.fx_add_noise_gen).  None: the generating kernel at every length.
# tools/noise_bench.py measures both (profiles/noise_bench.json); DESIGN.md 4.19 has the figures behind the rule.
GEN_MIX_MAX_L = None


def _exponent(noise_type: str, exponent) -> float:
    """The spectral exponent of a noise type (the reference's message for an unknown one), or the caller's own in [0, 2]."""
    if noise_type not in COLOR_EXPONENTS:
        raise ValueError(f"Invalid noise_type: '{noise_type}'. Choose 'gaussian', 'white', 'pink', or 'brown'.")
    if exponent is None:
        return COLOR_EXPONENTS[noise_type]
    exponent = float(exponent)
    if not 0.0 <= exponent <= 2.0:
        raise ValueError(f"exponent must be in [0, 2] (got {exponent})")
    return exponent


def generate_noise_batch(B: int, L: int, noise_type: str = "gaussian", seed: Optional[int] = None, exponent=None,
                         first_row: int = 0, device=None):
    """Noise [B, L] as a float32 device tensor, drawn on the device: standard normals for 'gaussian' / 'white', power-law
    noise of arbitrary unit for 'pink' (1 / f), 'brown' (1 / f^2) or a caller's `exponent` in [0, 2].  Row r is row
    first_row + r of `seed` whatever the batch; seed=None draws a fresh 64-bit seed.  A coloured row of one sample is zero."""
    import torch
    alpha = _exponent(noise_type, exponent)
    seed = _rng.check_seed(seed)
    with torch.cuda.device(device if device is not None else ops.require_gpu()):
        return ops.randn(B, L, seed, first_row) if alpha == 0.0 else ops.colored_noise(B, L, seed, alpha, first_row)


def _snr_rows(snr_db, B: int, seed: int, first_row: int):
    """A pair (lo, hi) draws one ratio per row: lo + (hi - lo) (w0 + 0.5) 2^-32, w0 the first word of the row's own
    counter (0, 0, row, stream 1) -- taken on the host.  Everything else passes through to the mix."""
    if isinstance(snr_db, tuple):
        if len(snr_db) != 2:
            raise ValueError("snr_db as a tuple must be a pair (lo, hi)")
        return _rng.uniform_rows(seed, first_row, B, snr_db[0], snr_db[1])
    return snr_db


def add_noise_device_batch(y, snr_db, noise_type: str = "gaussian", seed: Optional[int] = None, exponent=None,
                           first_row: int = 0, return_seed: bool = False):
    """Clips y [B, L] (float32 device tensor) -> [B, L] with noise drawn on the device.  snr_db: a number, one per row, a
    float64 device tensor [B], or a pair (lo, hi) from which every row draws its own ratio in [lo, hi) (the random-SNR
    augmentation of a training loop).  Row r uses row first_row + r of `seed`: a batch equals its clips.  seed=None draws a
    fresh 64-bit seed; return_seed=True returns (result, the seed used).  White noise is generated inside the mix and never
    stored; coloured noise is generated, then mixed.  A silent clip, and a coloured clip of one sample, is copied."""
    alpha = _exponent(noise_type, exponent)
    seed = _rng.check_seed(seed)
    B, L = y.shape
    first_row = _rng.check_rows(first_row, B)
    snr = _snr_rows(snr_db, B, seed, first_row)
    if alpha != 0.0:
        out = ops.fx_add_noise(y, ops.colored_noise(B, L, seed, alpha, first_row), snr)
    elif GEN_MIX_MAX_L is None or L <= GEN_MIX_MAX_L:
        out = ops.fx_add_noise_gen(y, snr, seed, first_row)
    else:
        out = ops.fx_add_noise(y, ops.randn(B, L, seed, first_row), snr)
    return (out, seed) if return_seed else out


def add_noise_device(y, snr_db: float, noise_type: str = "gaussian", seed: Optional[int] = None, exponent=None) -> np.ndarray:
    """add_noise with the noise drawn on the device: 1-D NumPy in, float64 out.  'pink' and 'brown' are real here (or a
    caller's `exponent` in [0, 2]) and raise no warning."""
    y = one_d(y, "Input audio data must be a 1D array for noise addition.")
    logger.info(f"Applying noise augmentation (device generator): type={noise_type}, SNR={snr_db:.2f} dB.")
    _exponent(noise_type, exponent)
    if y.size == 0:
        return np.zeros(0, dtype=np.float64)
    return host(add_noise_device_batch(row(y), float(snr_db), noise_type, seed, exponent=exponent))
