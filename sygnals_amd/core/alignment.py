"""Time-series alignment on the device: dynamic time warping (the reference's specification lists it, docs/dev_spec_v1.0.0.md
section 3.7, and its users know it as librosa.sequence.dtw, whose signature and return convention `dtw` keeps).

Served: the four metrics euclidean, sqeuclidean, cityblock, cosine or a caller's cost matrix C; the default step set
[[1,1],[0,1],[1,0]] with any finite weights_add / weights_mul; subseq; backtrack=False; return_steps.  Refused with a
ValueError: another step set, global_constraints, another metric or a callable, a non-finite C, a step matrix above
MAX_STEP_CELLS.  Parity is unpinned (librosa is not a dependency): the contract is the float64 restatement
tests/dtw_ref.py.  The accumulated cost is float64 on the device and depends on nothing but the float32 cost matrix.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops

METRICS = tuple(ops.DTW_METRICS)
DEFAULT_STEPS = ((1, 1), (0, 1), (1, 0))
# cells of one call's step matrix (one byte each; D, when asked for, is eight more): above it the caller wants distances
MAX_STEP_CELLS = 1 << 31

_SERVED = ("served: metric in " + ", ".join(METRICS) + " or a cost matrix C; the default step_sizes_sigma [[1,1],[0,1],[1,0]] with "
           "finite weights_add / weights_mul; subseq; backtrack; return_steps")


def _check_metric(metric):
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"dtw: metric {metric!r} is not served ({_SERVED})")


def _check_weights(weights_add, weights_mul):
    out = []
    for v, name in ((weights_mul, "weights_mul"), (weights_add, "weights_add")):
        if v is None:
            out.append(None)
            continue
        a = np.asarray(v, dtype=np.float64).reshape(-1)
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError(f"dtw: {name} must hold three finite values, one per step ({_SERVED})")
        out.append(a)
    return out


def _check_cells(B, N, M):
    if B * N * M > MAX_STEP_CELLS:
        raise ValueError(f"dtw: the step matrix of {B} x {N} x {M} cells is above the cap of {MAX_STEP_CELLS} cells; "
                         "dtw_distance_batch returns the costs without it")


def _seq(v, name) -> torch.Tensor:
    """(K, N) or (N,) NumPy array / tensor -> [1, K, N] float32 tensor, still where it was"""
    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
    if t.dim() == 1:
        t = t[None, :]
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"dtw: {name} must be a (K, N) or (N,) sequence, got shape {tuple(t.shape)}")
    return t.to(dtype=torch.float32)[None]


def dtw(X=None, Y=None, *, C=None, metric="euclidean", step_sizes_sigma=None, weights_add=None, weights_mul=None,
        subseq=False, backtrack=True, global_constraints=False, band_rad=0.25, return_steps=False):
    """librosa.sequence.dtw (0.10): D (N, M) float64 ndarray; wp (L, 2) int array from the end of the path to its start,
    when backtrack; steps (N, M) int array, when return_steps.  X, Y: (K, N) / (K, M) or (N,) / (M,) NumPy arrays or
    device tensors; or C, a precomputed (N, M) cost matrix."""
    if (C is None) == (X is None and Y is None) or (C is None and (X is None or Y is None)):
        raise ValueError("dtw: give either X and Y or a cost matrix C, not both and not neither")
    if step_sizes_sigma is not None:
        s = np.asarray(step_sizes_sigma)
        if s.shape != (3, 2) or tuple(map(tuple, s.tolist())) != DEFAULT_STEPS:
            raise ValueError(f"dtw: step_sizes_sigma {s.tolist()} is not served ({_SERVED})")
    if global_constraints:
        raise ValueError("dtw: global_constraints is not served: librosa's Sakoe-Chiba band rule (band_rad) cannot be pinned "
                         f"without librosa ({_SERVED})")
    wm, wa = _check_weights(weights_add, weights_mul)
    if C is not None:
        Ch = C.detach().cpu().numpy() if isinstance(C, torch.Tensor) else np.asarray(C)
        if Ch.ndim != 2 or Ch.size == 0:
            raise ValueError(f"dtw: C must be an (N, M) cost matrix, got shape {Ch.shape}")
        if not np.isfinite(Ch).all():
            raise ValueError("dtw: C must be finite (no NaN, no infinity)")
        _check_cells(1, *Ch.shape)
        Cd = (C if isinstance(C, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(Ch, dtype=np.float32)))
        Cd = Cd.to(device=ops.require_gpu(), dtype=torch.float32)[None]
    else:
        _check_metric(metric)
        Xd, Yd = _seq(X, "X"), _seq(Y, "Y")
        if Xd.shape[1] != Yd.shape[1]:
            raise ValueError(f"dtw: X and Y must have the same number of features, got {Xd.shape[1]} and {Yd.shape[1]}")
        _check_cells(1, Xd.shape[2], Yd.shape[2])
        dev = ops.require_gpu()
        Cd = ops.dtw_cost(Xd.to(dev), Yd.to(dev), metric)
    r = ops.dtw(Cd, weights_mul=wm, weights_add=wa, subseq=bool(subseq), want_D=True, want_steps=bool(return_steps),
                want_path=bool(backtrack))
    out = [r["D"][0].cpu().numpy()]
    if backtrack:
        n = int(r["path_len"][0].item())
        out.append(r["path"][0, :n].cpu().numpy().astype(np.int64))
    if return_steps:
        out.append(r["steps"][0].cpu().numpy().astype(np.int32))
    return out[0] if len(out) == 1 else tuple(out)


def _batch_cost(X, Y, C, metric, x_len, y_len):
    if (C is None) == (X is None and Y is None) or (C is None and (X is None or Y is None)):
        raise ValueError("dtw_batch: give either X and Y or a cost tensor C, not both and not neither")
    if C is not None:
        if not isinstance(C, torch.Tensor) or C.dim() != 3:
            raise ValueError("dtw_batch: C must be a [B, N, M] device tensor")
        return C.to(dtype=torch.float32)
    _check_metric(metric)
    return ops.dtw_cost(X, Y, metric, x_len, y_len)


def dtw_batch(X=None, Y=None, *, C=None, metric="euclidean", x_len=None, y_len=None, subseq=False, weights_add=None,
              weights_mul=None, return_D=False):
    """DTW of every pair of X [B, K, N] and Y [B, K, M] (float32 device tensors; x_len / y_len [B]: ragged batches), or
    of a cost tensor C [B, N, M] -> (cost [B] float64, path [B, N + M - 1, 2] int32 end first with (-1, -1) past
    path_len [B] int32), plus D [B, N, M] float64 when return_D; everything stays on the device."""
    wm, wa = _check_weights(weights_add, weights_mul)
    Cd = _batch_cost(X, Y, C, metric, x_len, y_len)
    _check_cells(*Cd.shape)
    r = ops.dtw(Cd, x_len, y_len, wm, wa, bool(subseq), want_D=bool(return_D), want_path=True)
    return (r["cost"], r["path"], r["path_len"]) + ((r["D"],) if return_D else ())


def dtw_distance_batch(X=None, Y=None, *, C=None, metric="euclidean", x_len=None, y_len=None, subseq=False,
                       weights_add=None, weights_mul=None) -> torch.Tensor:
    """The DTW cost of every pair -> [B] float64 on the device, through the distance-only path: neither the accumulated
    cost matrix nor the step codes are written."""
    wm, wa = _check_weights(weights_add, weights_mul)
    Cd = _batch_cost(X, Y, C, metric, x_len, y_len)
    return ops.dtw(Cd, x_len, y_len, wm, wa, bool(subseq), want_path=False)["cost"]
