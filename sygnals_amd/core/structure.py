"""Structure analysis on the device: the rest of `librosa.segment` over the kernels of csrc/structure.hip.  The
reference package has no such functions, so there is nothing to mirror: the float64 restatement
tests/structure_ref.py, pinned to NumPy, SciPy and scikit-learn, is the contract.

The functions with librosa's names take and return NumPy arrays in librosa's orientation (features data [d, t],
axis=-1); the `*_batch` forms work on float32 device tensors (matrices [B, T, T'], frame-major features [B, T, D]) and
stay on the device.  Sparse matrices and `clusterer=` callables raise ValueError, and so does `sync` with the median."""
from __future__ import annotations

import functools
from typing import Optional

import numpy as np

from .. import _structure as ST
from .. import ops

__all__ = ["recurrence_to_lag", "recurrence_to_lag_batch", "lag_to_recurrence", "lag_to_recurrence_batch", "timelag_filter",
           "timelag_filter_batch", "path_enhance", "path_enhance_batch", "agglomerative", "agglomerative_batch", "subsegment",
           "subsegment_batch", "sync", "sync_batch", "structure_segments"]

torch = ops.torch


def _matrix(who, a, name, square=False):
    """One dense real matrix -> float32 host tensor [1, rows, cols]."""
    if hasattr(a, "tocsr") or hasattr(a, "todense"):
        raise ValueError(f"{who}: sparse matrices are not served; pass a dense array")
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    if a.ndim != 2 or a.dtype.kind not in "fiub" or a.size == 0:
        raise ValueError(f"{who}: {name} must be a real matrix (got shape {list(a.shape)}); {who}_batch takes batches")
    if square and a.shape[0] != a.shape[1]:
        raise ValueError(f"{who}: {name} must be square (got shape {list(a.shape)})")
    return torch.from_numpy(np.array(a[None], dtype=np.float32, order="C"))


def _features(who, data, axis):
    """data with time along `axis` -> float32 host tensor [1, t, d] (librosa flattens the other axes in Fortran order)."""
    a = data.detach().cpu().numpy() if hasattr(data, "detach") else np.asarray(data)
    if a.dtype.kind not in "fiu" or a.size == 0 or a.ndim > 8:
        raise ValueError(f"{who}: data must be a real array with time along axis={axis} (got shape {list(a.shape)})")
    a = np.atleast_2d(a)
    try:
        a = np.swapaxes(a, axis, 0)
    except (np.exceptions.AxisError if hasattr(np, "exceptions") else np.AxisError) as e:
        raise ValueError(f"{who}: axis={axis!r} is not an axis of data {list(a.shape)}") from e
    a = a.reshape((a.shape[0], -1), order="F")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: data must be finite")
    return torch.from_numpy(np.array(a[None], dtype=np.float32, order="C"))


def _host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ shear
recurrence_to_lag_batch = ops.recurrence_to_lag
lag_to_recurrence_batch = ops.lag_to_recurrence


def recurrence_to_lag(rec, pad: bool = True, axis: int = -1):
    """librosa.segment.recurrence_to_lag(rec [t, t], pad, axis) -> [2 t, t] (pad) or [t, t] float32; axis=0: [t, 2 t]."""
    who = "recurrence_to_lag"
    R = _matrix(who, rec, "rec", square=True)
    ops._struct_axis(who, axis)
    return _host(ops.recurrence_to_lag(R.to(ops.require_gpu()), pad=pad, axis=axis)[0])


def lag_to_recurrence(lag, axis: int = -1):
    """librosa.segment.lag_to_recurrence(lag, axis) -> [t, t] float32; lag is [t, t] or padded to 2 t."""
    who = "lag_to_recurrence"
    L = _matrix(who, lag, "lag")
    ax = ops._struct_axis(who, axis)
    n, t = (L.shape[1], L.shape[2]) if ax == 1 else (L.shape[2], L.shape[1])
    if n not in (t, 2 * t):
        raise ValueError(f"{who}: lag must be [t, t] or padded along axis={axis} to 2 t (got {list(L.shape[1:])})")
    return _host(ops.lag_to_recurrence(L.to(ops.require_gpu()), axis=axis)[0])


def _median_window(function, args, kwargs, axis):
    """w if the call is scipy.ndimage.median_filter with size (1, w) along time (axis 0: (w, 1)) and nothing else that
    changes the filter; else None."""
    try:
        from scipy.ndimage import median_filter
    except ImportError:
        return None
    if function is not median_filter or len(args) != 1 or set(kwargs) - {"size", "mode", "cval"}:
        return None
    size = kwargs.get("size")
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        return None
    w, one = (size[1], size[0]) if axis != 0 else (size[0], size[1])
    cap = ops.structure_constants()["median_w_max"]
    if one != 1 or isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 1 or w % 2 == 0 or w > cap:
        return None
    return int(w) if kwargs.get("mode", "reflect") in ST.BOUNDARY_MODES else None


def timelag_filter_batch(function, pad: bool = True, index: int = 0, axis: int = -1):
    """librosa.segment.timelag_filter for device tensors: the wrapped function receives its `index`-th argument [B, t, t]
    sheared into time-lag form on the device and its result is sheared back.  scipy.ndimage.median_filter with
    size=(1, w) (axis 0: (w, 1)), w odd, takes the fused kernel instead (ops.diag_median): no lag matrix is made."""
    ops._struct_axis("timelag_filter", axis)

    @functools.wraps(function)
    def wrapper(*args, **kwargs):
        args = list(args)
        w = _median_window(function, args, kwargs, axis) if index == 0 else None
        if w is not None:
            return ops.diag_median(args[0], w, mode=kwargs.get("mode", "reflect"), cval=kwargs.get("cval", 0.0), pad=pad, axis=axis)
        args[index] = ops.recurrence_to_lag(args[index], pad=pad, axis=axis)
        result = function(*args, **kwargs)
        if not isinstance(result, torch.Tensor):
            raise ValueError("timelag_filter_batch: the wrapped function must return a device tensor")
        return ops.lag_to_recurrence(result.to(torch.float32), axis=axis)
    return wrapper


def timelag_filter(function, pad: bool = True, index: int = 0, axis: int = -1):
    """librosa.segment.timelag_filter(function, pad, index): a wrapper that applies `function` in time-lag space.  The
    shears run on the device; `function` receives and returns NumPy arrays.  scipy.ndimage.median_filter with
    size=(1, w), w odd and up to 63, is run by the fused device kernel."""
    ops._struct_axis("timelag_filter", axis)

    @functools.wraps(function)
    def wrapper(*args, **kwargs):
        who = "timelag_filter"
        args = list(args)
        R = _matrix(who, args[index], "the matrix", square=True)
        dev = ops.require_gpu()
        w = _median_window(function, args, kwargs, axis) if index == 0 else None
        if w is not None:
            return _host(ops.diag_median(R.to(dev), w, mode=kwargs.get("mode", "reflect"), cval=kwargs.get("cval", 0.0), pad=pad,
                                         axis=axis)[0])
        args[index] = _host(ops.recurrence_to_lag(R.to(dev), pad=pad, axis=axis)[0])
        result = _matrix(who, function(*args, **kwargs), "the function's result")
        return _host(ops.lag_to_recurrence(result.to(dev), axis=axis)[0])
    return wrapper


# ------------------------------------------------------------------ path enhancement
def _path_kwargs(who, kwargs):
    extra = set(kwargs) - {"mode", "cval"}
    if extra:
        raise ValueError(f"{who}: the convolution arguments served are mode and cval (got {sorted(extra)})")
    return kwargs.get("mode", "reflect"), kwargs.get("cval", 0.0)


def path_enhance_batch(R, n: int, window="hann", max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7,
                       zero_mean: bool = False, clip: bool = True, **kwargs):
    """R [B, T, T'] float32 on the device -> [B, T, T'] (ops.path_enhance)."""
    mode, cval = _path_kwargs("path_enhance", kwargs)
    return ops.path_enhance(R, n, window, max_ratio, min_ratio, n_filters, zero_mean, clip, mode, cval)


def path_enhance(R, n: int, window="hann", max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7,
                 zero_mean: bool = False, clip: bool = True, **kwargs):
    """librosa.segment.path_enhance(R, n, window, max_ratio, min_ratio, n_filters, zero_mean, clip, **kwargs) -> float32
    NumPy of R's shape; mode and cval in kwargs are scipy.ndimage.convolve's."""
    who = "path_enhance"
    mode, cval = _path_kwargs(who, kwargs)
    Rm = _matrix(who, R, "R")
    ST.boundary_code(who, mode)
    ST.path_filters(n, window, max_ratio, min_ratio, n_filters, zero_mean)
    return _host(ops.path_enhance(Rm.to(ops.require_gpu()), n, window, max_ratio, min_ratio, n_filters, zero_mean, clip, mode, cval)[0])


# ------------------------------------------------------------------ segmentation
def _no_clusterer(who, clusterer):
    if clusterer is not None:
        raise ValueError(f"{who}: clusterer= callables are not served; the device runs the default, Ward linkage over the chain")


def agglomerative_batch(X, k, offset=None, length=None):
    """X [B, T, D] float32 on the device -> (bounds [n_spans, max k] int32, count [n_spans]) (ops.agglomerative)."""
    return ops.agglomerative(X, k, offset, length)


def agglomerative(data, k: int, clusterer=None, axis: int = -1):
    """librosa.segment.agglomerative(data [d, t], k, axis) -> the k boundary frames (the first is 0)."""
    who = "agglomerative"
    _no_clusterer(who, clusterer)
    X = _features(who, data, axis)
    k = ops._sim_int(who, "k", k, 1)
    if k > X.shape[1]:
        raise ValueError(f"{who}: k = {k} segments need at least k frames (data has {X.shape[1]})")
    cap = ops.structure_constants()["agg_t_max"]
    if X.shape[1] > cap:
        raise ValueError(f"{who}: {X.shape[1]} frames are above the served {cap} frames")
    bounds, _ = ops.agglomerative(X.to(ops.require_gpu()), k)
    return _host(bounds[0]).astype(np.int64)


def subsegment_batch(X, frames, n_segments: int = 4):
    """X [B, T, D] float32 on the device -> (bounds [B, n] int32, count [B]) (ops.subsegment)."""
    return ops.subsegment(X, frames, n_segments)


def subsegment(data, frames, n_segments: int = 4, clusterer=None, axis: int = -1):
    """librosa.segment.subsegment(data [d, t], frames, n_segments, axis) -> the boundary frames of the sub-segments."""
    who = "subsegment"
    _no_clusterer(who, clusterer)
    X = _features(who, data, axis)
    ops._sim_int(who, "n_segments", n_segments, 1)
    ST.fix_frames(ops._struct_ints(who, "frames", frames), X.shape[1])
    bounds, _ = ops.subsegment(X.to(ops.require_gpu()), frames, n_segments)
    return _host(bounds[0]).astype(np.int64)


def sync_batch(X, edges, aggregate: str = "mean"):
    """X [B, T, D] float32 on the device, edges [n_seg + 1] or [B, n_seg + 1] -> [B, n_seg, D] (ops.segment_sync)."""
    return ops.segment_sync(X, edges, aggregate)


_AGGREGATES = {np.mean: "mean", np.max: "max", np.min: "min", np.amax: "max", np.amin: "min", np.median: "median"}


def sync(data, idx, aggregate="mean", pad: bool = True, axis: int = -1):
    """librosa.util.sync(data, idx, aggregate, pad, axis) for aggregate 'mean' / np.mean, 'max' / np.max or 'min' / np.min
    and idx a list of boundary frames -> float32 NumPy with the segments along `axis`."""
    who = "sync"
    name = _AGGREGATES.get(aggregate, aggregate) if callable(aggregate) else aggregate
    if name == "median":
        raise ValueError(f"{who}: aggregate='median' is not served; served: 'mean', 'max', 'min'")
    ops._sim_name(who, "aggregate", name, ST.SYNC_AGGREGATES)
    a = data.detach().cpu().numpy() if hasattr(data, "detach") else np.asarray(data)
    if a.ndim < 1 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"{who}: data must be a real array (got shape {list(a.shape)})")
    moved = np.moveaxis(a, axis, 0)                              # [t, ...]
    Tn = moved.shape[0]
    edges = ST.fix_frames(ops._struct_ints(who, "idx", idx), Tn, pad=pad)
    if edges.size < 2:
        raise ValueError(f"{who}: idx leaves no segment")
    X = torch.from_numpy(np.array(moved.reshape(1, Tn, -1), dtype=np.float32, order="C"))
    out = _host(ops.segment_sync(X.to(ops.require_gpu()), edges, name)[0])
    return np.moveaxis(out.reshape((edges.size - 1,) + moved.shape[1:]), 0, axis)


# ------------------------------------------------------------------ the chain behind `dsp structure`
def structure_segments(y, sr: float, k: int, feature: str = "mfcc", enhance: Optional[int] = None, median: Optional[int] = None):
    """One clip -> the start frames of k segments: MFCC or STFT chroma (n_fft 2048, hop 512), their symmetric affinity
    recurrence matrix, optionally path_enhance over `enhance` frames and the diagonal median over `median` frames, then
    the Ward clustering of neighbouring frames, each frame described by its row of that matrix.  Everything after the
    load stays on the device."""
    who = "structure_segments"
    a = np.asarray(y.detach().cpu().numpy() if hasattr(y, "detach") else y)
    if a.ndim != 1 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"{who}: y must be one real clip [L] (got shape {list(a.shape)})")
    if feature not in ("mfcc", "chroma"):
        raise ValueError(f"{who}: feature={feature!r} is not served; served: 'mfcc', 'chroma'")
    k = ops._sim_int(who, "k", k, 1)
    Tn = 1 + a.size // 512
    cap = ops.structure_constants()["agg_t_max"]
    if k > Tn or Tn > cap:
        raise ValueError(f"{who}: the clip has {Tn} frames; served are k <= frames <= {cap}")
    if enhance is not None:
        ST.path_filters(enhance)
    yd = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)[None]).to(ops.require_gpu())
    if feature == "mfcc":
        F = ops.mfcc_batch(yd, float(sr))
    else:
        from .features.tonal import chroma_stft_batch
        F = chroma_stft_batch(yd, float(sr))
    X = F.transpose(1, 2).contiguous()
    R = ops.recurrence_matrix(X, mode="affinity", sym=True) if X.shape[1] > 1 else torch.ones((1, 1, 1), device=X.device)
    if enhance is not None:
        R = ops.path_enhance(R, enhance)
    if median is not None:
        R = ops.diag_median(R, median)
    bounds, _ = ops.agglomerative(R, k)
    return _host(bounds[0]).astype(np.int64)
