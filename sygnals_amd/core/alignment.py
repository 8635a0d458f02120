"""Time-series alignment on the device: dynamic time warping (the reference's specification lists it, docs/dev_spec_v1.0.0.md
section 3.7, and its users know it as librosa.sequence.dtw, whose signature and return convention `dtw` keeps).

Served: the four metrics euclidean, sqeuclidean, cityblock, cosine or a caller's cost matrix C; the default step set
[[1,1],[0,1],[1,0]] with any finite weights_add / weights_mul; subseq; backtrack=False; return_steps.  Refused with a
ValueError: another step set, global_constraints, another metric or a callable, a non-finite C, a step matrix above
MAX_STEP_CELLS.  Parity is unpinned (librosa is not a dependency): the contract is the float64 restatement
tests/dtw_ref.py.  The accumulated cost is float64 on the device and depends on nothing but the float32 cost matrix.

Below DTW: generalised cross-correlation and delay estimation (gcc_batch, estimate_delay_batch, estimate_delay).
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


# ------------------------------------------------------------------ generalised cross-correlation and delay estimation
# (the reference's specification lists cross-correlation, docs/dev_spec_v1.0.0.md 3.5, and multi-channel handling, 3.7).
# Served: real float32 rows, y with one row (a reference channel) or one per row of x, the weightings "none" (plain
# cross-correlation: scipy.signal.correlate(x, y, "full") at scipy.signal.correlation_lags) and "phat" (phase transform).
# Refused with a ValueError: another weighting (SCOT, Roth, ML), complex or empty input, a max_lag above
# min(Lx, Ly) - 1.  The contract is the float64 restatement tests/xspec_ref.py.
GCC_WEIGHTINGS = tuple(ops.GCC_WEIGHTINGS)
_GCC_SERVED = ("served: real float32 rows x [B, Lx] and y [1 or B, Ly], weighting in " + ", ".join(GCC_WEIGHTINGS)
               + ", 0 <= max_lag <= min(Lx, Ly) - 1")


def _gcc_args(x, y, max_lag, weighting, who):
    if not isinstance(weighting, str) or weighting not in GCC_WEIGHTINGS:
        raise ValueError(f"{who}: weighting {weighting!r} is not served ({_GCC_SERVED})")
    for t, name in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a [rows, samples] device tensor ({_GCC_SERVED})")
        if t.is_complex():
            raise ValueError(f"{who}: complex input is not served ({_GCC_SERVED})")
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: {name} is empty, shape {tuple(t.shape)} ({_GCC_SERVED})")
    if y.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"{who}: y must have one row or one row per row of x ({x.shape[0]}), got {y.shape[0]} ({_GCC_SERVED})")
    top = min(x.shape[1], y.shape[1]) - 1
    if max_lag is None:
        max_lag = top
    if isinstance(max_lag, bool) or int(max_lag) != max_lag or not (0 <= max_lag <= top):
        raise ValueError(f"{who}: max_lag={max_lag} is outside 0 ... min(Lx, Ly) - 1 = {top} ({_GCC_SERVED})")
    return int(max_lag)


def gcc_batch(x, y, max_lag: Optional[int] = None, weighting: str = "none"):
    """Generalised cross-correlation of the rows of x [B, Lx] with y [1 or B, Ly] (float32 device tensors) ->
    (lags int64 ndarray [2 max_lag + 1], r device tensor [B, 2 max_lag + 1]); r at lag t is
    irfft(W X conj(Y), n)[t mod n], n = conv_fft_len(Lx + Ly - 1).  If x[n] = y[n - d] the peak is at lag +d."""
    max_lag = _gcc_args(x, y, max_lag, weighting, "gcc_batch")
    r = ops.gcc(x.to(dtype=torch.float32), y.to(dtype=torch.float32), max_lag, weighting)
    return np.arange(-max_lag, max_lag + 1, dtype=np.int64), r


def estimate_delay_batch(x, y, fs: float = 1.0, max_lag: Optional[int] = None, weighting: str = "phat"):
    """The delay of every row of x against y -> (delay_seconds float64 [B], lag int64 [B], peak float64 [B]), device
    tensors: the first maximum of gcc_batch's r over the lags, refined by the parabola through its neighbours where it is
    interior and the parabola opens downwards (the cepstral picker's rule, float64)."""
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"estimate_delay_batch: fs must be positive and finite, got {fs}")
    max_lag = _gcc_args(x, y, max_lag, weighting, "estimate_delay_batch")
    r = ops.gcc(x.to(dtype=torch.float32), y.to(dtype=torch.float32), max_lag, weighting)
    return ops.peak_pick(r, -max_lag, float(fs))


def estimate_delay(x, y, fs: float = 1.0, max_lag: Optional[int] = None, weighting: str = "phat"):
    """1-D NumPy x, y -> (delay_seconds, lag, peak) as Python numbers: x lags y by `delay_seconds`."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim != 1 or y.ndim != 1:
        raise ValueError("Input data must be a 1D array.")
    if np.iscomplexobj(x) or np.iscomplexobj(y):
        raise ValueError(f"estimate_delay: complex input is not served ({_GCC_SERVED})")
    if x.size == 0 or y.size == 0:
        raise ValueError(f"estimate_delay: empty input ({_GCC_SERVED})")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError(f"estimate_delay: fs must be positive and finite, got {fs}")
    xt, yt = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))[None] for v in (x, y))
    max_lag = _gcc_args(xt, yt, max_lag, weighting, "estimate_delay")
    dev = ops.require_gpu()
    d, lag, pk = ops.peak_pick(ops.gcc(xt.to(dev), yt.to(dev), max_lag, weighting), -max_lag, float(fs))
    return float(d[0].item()), int(lag[0].item()), float(pk[0].item())
