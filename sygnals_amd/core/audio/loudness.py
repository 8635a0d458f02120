"""Loudness metering (ITU-R BS.1770-4 / EBU R128) and loudness normalisation on the device, over the kernels of
csrc/loudness.hip.  The reference package has no loudness functions, so there is nothing to mirror: the float64 restatement
tests/loudness_ref.py, pinned to the standards' known answers, is the contract.

The *_batch functions take clips [B, L] (mono) or [B, C, L] (a float32 device tensor is taken as it is, anything else is
uploaded) and stay on the device.  integrated_loudness, loudness_metrics and normalize_loudness take one clip [L] or
[C, L]: NumPy in, NumPy / floats out.  sr is an integer rate from 8000 to 384000 Hz.  True peak is the largest
|resample_poly(y, up, 1)| with the package's default filter (up = 4 below 96 kHz, 2 below 192 kHz, else 1), not Annex 2's
48-tap table.  What is not served raises ValueError."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import _loudness as LD
from ... import ops

__all__ = ["integrated_loudness", "integrated_loudness_batch", "momentary_loudness_batch", "short_term_loudness_batch",
           "loudness_range_batch", "true_peak_batch", "loudness_metrics", "normalize_loudness", "normalize_loudness_batch"]

torch = ops.torch


def _clips(y, sr, who: str, channel_weights=None):
    """[B, L] or [B, C, L] float32 on the device, after the checks that need none: the shape, the rate, the weights."""
    a = y if hasattr(y, "is_cuda") else np.asarray(y)
    if len(a.shape) not in (2, 3) or (not hasattr(y, "is_cuda") and a.dtype.kind not in "fiu"):
        raise ValueError(f"{who}: clips must be real, [B, L] (mono) or [B, C, L] (got shape {list(a.shape)}, dtype {a.dtype})")
    if min(a.shape) == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    LD.check_fs(sr, who)
    LD.channel_weights(a.shape[1] if len(a.shape) == 3 else 1, channel_weights)
    if hasattr(y, "is_cuda"):
        return y if (y.is_cuda and y.dtype == torch.float32) else y.to(device=ops.require_gpu(), dtype=torch.float32)
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(ops.require_gpu())     # (a copy: a may be read-only)


def _one(y, who: str) -> np.ndarray:
    """One clip [L] or [C, L] as a host array [1, C, L] (the caller reshapes a result to y's own shape)."""
    a = y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)
    if a.ndim not in (1, 2) or a.dtype.kind not in "fiu":
        raise ValueError(f"{who}: y must be one real clip [L] or [C, L] (got shape {list(a.shape)}); the *_batch functions take [B, C, L]")
    if a.size == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    return a.reshape(1, -1, a.shape[-1])


def _blocks(y, sr, channel_weights, who):
    x = _clips(y, sr, who, channel_weights)
    return ops.loudness_blocks(ops.loudness_segments(x, sr), sr, channel_weights)


def integrated_loudness_batch(y, sr: int, channel_weights=None):
    """Integrated loudness of every clip: float64 [B] LUFS on the device, -inf where no block passes the gates."""
    return ops.integrated_loudness(_clips(y, sr, "integrated_loudness_batch", channel_weights), sr, channel_weights)


def momentary_loudness_batch(y, sr: int, channel_weights=None):
    """Momentary loudness (400 ms blocks every 100 ms): float32 [B, n_m] LUFS on the device."""
    return _blocks(y, sr, channel_weights, "momentary_loudness_batch")[0]


def short_term_loudness_batch(y, sr: int, channel_weights=None):
    """Short-term loudness (3 s blocks every 100 ms): float32 [B, n_s] LUFS on the device."""
    return _blocks(y, sr, channel_weights, "short_term_loudness_batch")[1]


def loudness_range_batch(y, sr: int, channel_weights=None):
    """Loudness range (EBU Tech 3342): float32 [B] LU on the device, 0 where fewer than two short-term values pass."""
    _, S, _, thr = _blocks(y, sr, channel_weights, "loudness_range_batch")
    return ops.loudness_range(S, thr)


def true_peak_batch(y, sr: int, db: bool = False):
    """True peak of every clip over its channels: float32 [B] on the device, linear or (db=True) dBTP."""
    tp = ops.true_peak(_clips(y, sr, "true_peak_batch"), sr)
    return 20.0 * torch.log10(tp) if db else tp


def normalize_loudness_batch(y, sr: int, target_lufs: float = -23.0, peak_limit_dbtp: Optional[float] = None,
                             channel_weights=None, return_gain: bool = False):
    """Clips scaled to target_lufs (ops.normalize_loudness): float32 on the device in y's shape; with peak_limit_dbtp the
    gain is lowered so that the true peak stays under it; silent or too-short clips are copied.  return_gain adds the
    gains and the measured loudness, float64 [B] each.  Nothing between measuring and scaling waits on the host."""
    return ops.normalize_loudness(_clips(y, sr, "normalize_loudness_batch", channel_weights), sr, target_lufs, peak_limit_dbtp,
                                  channel_weights, return_gain)


def integrated_loudness(y, sr: int, channel_weights=None) -> float:
    """Integrated loudness in LUFS of one clip [L] or [C, L]."""
    return float(integrated_loudness_batch(_one(y, "integrated_loudness"), sr, channel_weights)[0].item())


def loudness_metrics(y, sr: int, channel_weights=None) -> dict:
    """I (LUFS), LRA (LU), TP_dbtp, M_max and S_max (LUFS) of one clip [L] or [C, L]; -inf where there is nothing to read."""
    x = _clips(_one(y, "loudness_metrics"), sr, "loudness_metrics", channel_weights)
    M, S, I, thr = ops.loudness_blocks(ops.loudness_segments(x, sr), sr, channel_weights)
    lra = ops.loudness_range(S, thr)
    tp = true_peak_batch(x, sr, db=True)
    top = lambda t: float(t.max().item()) if t.numel() else float("-inf")      # noqa: E731
    return {"I": float(I[0].item()), "LRA": float(lra[0].item()), "TP_dbtp": float(tp[0].item()), "M_max": top(M), "S_max": top(S)}


def normalize_loudness(y, sr: int, target_lufs: float = -23.0, peak_limit_dbtp: Optional[float] = None, channel_weights=None
                       ) -> np.ndarray:
    """One clip [L] or [C, L] scaled to target_lufs: float64 NumPy in y's shape (computed in float32 on the device)."""
    a = _one(y, "normalize_loudness")
    out = normalize_loudness_batch(a, sr, target_lufs, peak_limit_dbtp, channel_weights)
    return out[0].cpu().numpy().astype(np.float64).reshape(tuple(y.shape) if hasattr(y, "shape") else np.shape(y))
