"""SpecAugment (Park et al. 2019) on the device, over csrc/spec_augment.hip: a time warp, then frequency and time masks,
drawn fresh per clip from the package's Philox generator.  The reference's `augment` group works on waveforms only, so
this is the package's own definition (sygnals_amd/_specaug.py states the draws; tests/specaug_ref.py is the contract).

The `*_batch` functions take [B, K, T] float32 device tensors, frames fastest (what mfcc_batch, feature_post and the mel
front ends leave on the device), and stay there; spec_augment takes one NumPy [K, T] array and returns NumPy.  Clip b
draws from row first_row + b of `seed` alone, so a batch equals its clips and a call can be replayed from its seed."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import _rng, _specaug, ops


def spec_augment_batch(x, freq_masks: int = 2, freq_width: int = 27, time_masks: int = 2, time_width: int = 100,
                       time_ratio: float = 1.0, time_warp: int = 0, mask_value=0.0, mode: str = "linear",
                       seed: Optional[int] = None, first_row: int = 0, lengths=None, out=None, return_seed: bool = False,
                       return_params: bool = False):
    """x [B, K, T] (float32 device tensor) -> [B, K, T]: per clip a warp of up to `time_warp` frames about a drawn centre
    (two linear resizes; none if T_b <= 2 time_warp), then the union of `freq_masks` masks of up to `freq_width` rows and
    `time_masks` masks of up to min(time_width, floor(time_ratio T_b)) frames, written with `mask_value` (a finite float or
    "mean", the clip's mean over its valid frames).  lengths [B]: valid frames T_b per clip; later frames are copied.
    seed=None draws a fresh 64-bit seed.  `out` may be x itself when time_warp = 0 (only masked cells are written).
    Returns the result, then the seed (return_seed) and the draws as integer arrays (return_params:
    sygnals_amd._specaug.params), in that order."""
    who = "spec_augment_batch"
    _specaug.check_mode(mode, who)
    ops._f32(x, f"{who}: x", 3, axes="[B, K, T]")
    B, K, T = (int(n) for n in x.shape)
    _specaug.check_shape(B, K, T, who)
    _specaug.check_args(K, T, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, who)
    _specaug.check_mask_value(mask_value, who)
    seed = _rng.check_seed(seed)
    first_row = _rng.check_rows(first_row, B)
    if lengths is not None:
        lengths = ops._spec_lengths(lengths, B, T, who)
    y = ops.spec_augment(x, seed, first_row, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, mask_value,
                         lengths=lengths, out=out)
    res = (y,)
    if return_seed:
        res += (seed,)
    if return_params:
        res += (_specaug.params(seed, first_row, B, K, T, lengths, freq_masks, freq_width, time_masks, time_width, time_ratio,
                                time_warp),)
    return res if len(res) > 1 else y


def spec_augment(S, freq_masks: int = 2, freq_width: int = 27, time_masks: int = 2, time_width: int = 100, time_ratio: float = 1.0,
                 time_warp: int = 0, mask_value=0.0, mode: str = "linear", seed: Optional[int] = None, first_row: int = 0,
                 return_seed: bool = False, return_params: bool = False):
    """One NumPy [K, T] array -> float32 NumPy [K, T]: clip 0 of spec_augment_batch on S[None], bit for bit."""
    a = np.asarray(S)
    if a.ndim != 2:
        raise ValueError(f"spec_augment: S must be [K, T] (got {a.ndim} dimensions)")
    if a.size == 0:
        raise ValueError(f"spec_augment: empty input (shape {list(a.shape)})")
    _specaug.check_mode(mode, "spec_augment")
    _specaug.check_args(a.shape[0], a.shape[1], freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp)
    _specaug.check_mask_value(mask_value)
    x = ops.to_device_f32(np.ascontiguousarray(a, dtype=np.float32)).reshape(1, a.shape[0], a.shape[1])
    res = spec_augment_batch(x, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, mask_value, mode, seed,
                             first_row, return_seed=return_seed, return_params=return_params)
    if isinstance(res, tuple):
        return (res[0][0].cpu().numpy(),) + res[1:]
    return res[0].cpu().numpy()


def freq_mask_batch(x, freq_masks: int = 2, freq_width: int = 27, mask_value=0.0, seed: Optional[int] = None, first_row: int = 0,
                    lengths=None, out=None, return_seed: bool = False, return_params: bool = False):
    """The frequency masks of spec_augment_batch alone: the same draws as the full call's, bit for bit."""
    return spec_augment_batch(x, freq_masks, freq_width, 0, 0, 1.0, 0, mask_value, "linear", seed, first_row, lengths, out,
                              return_seed, return_params)


def time_mask_batch(x, time_masks: int = 2, time_width: int = 100, time_ratio: float = 1.0, mask_value=0.0,
                    seed: Optional[int] = None, first_row: int = 0, lengths=None, out=None, return_seed: bool = False,
                    return_params: bool = False):
    """The time masks of spec_augment_batch alone: the same draws as the full call's, bit for bit."""
    return spec_augment_batch(x, 0, 0, time_masks, time_width, time_ratio, 0, mask_value, "linear", seed, first_row, lengths, out,
                              return_seed, return_params)


def time_warp_batch(x, time_warp: int = 5, mode: str = "linear", seed: Optional[int] = None, first_row: int = 0, lengths=None,
                    out=None, return_seed: bool = False, return_params: bool = False):
    """The time warp of spec_augment_batch alone (ESPnet's time_warp with a drawn centre): the same draws as the full call's."""
    return spec_augment_batch(x, 0, 0, 0, 0, 1.0, time_warp, 0.0, mode, seed, first_row, lengths, out, return_seed,
                              return_params)
