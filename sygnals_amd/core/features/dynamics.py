"""Feature dynamics on the device: deltas (librosa.feature.delta), per-utterance CMVN and context stacking
(librosa.feature.stack_memory), over the kernels of csrc/dynamics.hip.  The NumPy functions mirror the host libraries'
signatures (NumPy in, float64 out); the *_batch functions take [B, K, T] device tensors or arrays and stay on the device."""
from __future__ import annotations

import numpy as np

from ... import _dynamics as DY
from ... import ops


def _dev3(data, who: str):
    """[B, K, T] float32 on the device (a tensor is taken as it is; an array is uploaded)."""
    if hasattr(data, "is_cuda"):
        return data
    a = np.asarray(data, dtype=np.float32)
    if a.ndim != 3:
        raise ValueError(f"{who}: data must be [B, K, T] (got {a.ndim} dimensions)")
    if a.size == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    return ops.to_device_f32(a.reshape(a.shape[0], -1)).reshape(a.shape)


def _rows(data, who: str):
    """A [..., T] array as [1, R, T] (any leading axes), and the shape to give back."""
    a = np.asarray(data)
    if a.ndim < 1 or a.size == 0:
        raise ValueError(f"{who}: empty input (shape {list(a.shape)})")
    return np.ascontiguousarray(a, dtype=np.float32).reshape(1, -1, a.shape[-1]), a.shape


def delta(data, width: int = 9, order: int = 1, axis: int = -1, mode: str = "interp", **kwargs) -> np.ndarray:
    """librosa.feature.delta: the order-th Savitzky-Golay derivative of `data` along `axis` (width odd and >= 3).
    kwargs: cval for mode="constant"."""
    cval = float(kwargs.pop("cval", 0.0))
    if kwargs:
        raise ValueError(f"delta: unknown arguments {sorted(kwargs)} (served: cval)")
    a = np.moveaxis(np.asarray(data), axis, -1)
    x, shape = _rows(a, "delta")
    w, o = DY.check_width_order(width, order)
    DY.check_mode(mode)
    DY.check_interp(w, x.shape[-1], mode)
    y = ops.delta(_dev3(x, "delta"), w, o, mode=mode, cval=cval).cpu().numpy().astype(np.float64).reshape(shape)
    return np.moveaxis(y, -1, axis)


def cmvn(data, window=None, variance: bool = True) -> np.ndarray:
    """Per-row mean / variance normalisation of a [K, T] array along T: all frames (window=None) or Kaldi's centred sliding
    window of `window` frames."""
    x, shape = _rows(data, "cmvn")
    return ops.cmvn(_dev3(x, "cmvn"), window, variance).cpu().numpy().astype(np.float64).reshape(shape)


def stack_memory(data, n_steps: int = 2, delay: int = 1) -> np.ndarray:
    """librosa.feature.stack_memory with zero padding on a [K, T] (or [T]) array: [n_steps K, T]."""
    a = np.asarray(data)
    a2 = a[None, :] if a.ndim == 1 else a
    if a2.ndim != 2:
        raise ValueError("stack_memory: data must be [K, T] or [T]")
    if a2.size == 0:
        raise ValueError(f"stack_memory: empty input (shape {list(a.shape)})")
    x = np.ascontiguousarray(a2, dtype=np.float32)[None]
    return ops.stack_memory(_dev3(x, "stack_memory"), n_steps, delay).cpu().numpy().astype(np.float64)[0]


def _frames(x) -> int:
    return int(x.shape[-1]) if hasattr(x, "shape") else int(np.asarray(x).shape[-1])


def delta_batch(x, width: int = 9, order: int = 1, mode: str = "interp", cval: float = 0.0, out=None, form=None):
    """ops.delta on [B, K, T] (a device tensor, or an array that is uploaded); the arguments are checked first."""
    w, _ = DY.check_width_order(width, order)
    DY.check_mode(mode)
    DY.check_interp(w, _frames(x), mode)
    return ops.delta(_dev3(x, "delta_batch"), width, order, mode=mode, cval=cval, out=out, form=form)


def cmvn_batch(x, window=None, variance: bool = True, out=None, form=None):
    """ops.cmvn on [B, K, T]."""
    DY.check_window(window)
    return ops.cmvn(_dev3(x, "cmvn_batch"), window, variance, out=out, form=form)


def stack_memory_batch(x, n_steps: int = 2, delay: int = 1, out=None):
    """ops.stack_memory on [B, K, T]."""
    DY.check_stack(n_steps, delay)
    return ops.stack_memory(_dev3(x, "stack_memory_batch"), n_steps, delay, out=out)


def feature_post_batch(x, cmvn=None, variance: bool = True, deltas: int = 2, width: int = 9, mode: str = "interp", out=None,
                       form=None):
    """ops.feature_post on [B, K, T]: [statics | delta | delta-delta] after the optional CMVN (None, "global" or a window)."""
    if isinstance(deltas, bool) or deltas not in (0, 1, 2):
        raise ValueError(f"feature_post: deltas must be 0, 1 or 2 (got {deltas!r})")
    if cmvn not in (None, "global"):
        if isinstance(cmvn, str):
            raise ValueError(f"feature_post: cmvn must be None, 'global' or a sliding window >= 1 (got {cmvn!r})")
        DY.check_window(cmvn, "feature_post")
    if deltas:
        w, _ = DY.check_width_order(width, deltas, "feature_post")
        DY.check_mode(mode, "feature_post")
        DY.check_interp(w, _frames(x), mode, "feature_post")
    return ops.feature_post(_dev3(x, "feature_post_batch"), cmvn=cmvn, variance=variance, deltas=deltas, width=width, mode=mode,
                            out=out, form=form)
