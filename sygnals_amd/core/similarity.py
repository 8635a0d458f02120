"""Self-similarity on the device: `librosa.segment.recurrence_matrix` and `cross_similarity` over the kernels of
csrc/similarity.hip.  The reference package has no such functions, so there is nothing to mirror: the float64
restatement tests/similarity_ref.py, pinned to scikit-learn's brute NearestNeighbors and scipy's cdist, is the contract.

`recurrence_matrix` and `cross_similarity` take one feature matrix in librosa's orientation, data [d, t], and return a
dense float32 NumPy matrix; like librosa's, R[i, j] is non-zero when frame i is a nearest neighbour of frame j (the
transpose of the device layout, where row i holds the neighbours of frame i).  The `*_batch` forms work on float32 device
tensors in the device layout, X [B, T, D] -> [B, T, T'], row i the links of frame i, and stay on the device.  Served:
metric "euclidean", "sqeuclidean" or "cosine", 1 to 256 neighbours; the k-NN search never writes the distance matrix.
Sparse outputs, "cityblock" and every other metric raise ValueError."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import ops

__all__ = ["recurrence_matrix", "recurrence_matrix_batch", "cross_similarity", "cross_similarity_batch"]

torch = ops.torch


def _features(who, data, name="data"):
    """data [d, t] -> float32 host tensor [1, t, d]."""
    a = data.detach().cpu().numpy() if hasattr(data, "detach") else np.asarray(data)
    if a.ndim != 2 or a.dtype.kind not in "fiu" or a.size == 0:
        raise ValueError(f"{who}: {name} must be a real matrix [d, t] (got shape {list(a.shape)}); {who}_batch takes batches")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{who}: {name} must be finite")
    return torch.from_numpy(np.array(a.T[None], dtype=np.float32, order="C"))


def recurrence_matrix_batch(X, *, k: Optional[int] = None, width: int = 1, metric: str = "euclidean", sym: bool = False,
                            mode: str = "connectivity", bandwidth=None, self: bool = False, x_len=None):
    """X [B, T, D] float32 on the device -> [B, T, T] float32 (ops.recurrence_matrix): row i holds the links of frame i."""
    return ops.recurrence_matrix(X, None, k=k, width=width, metric=metric, sym=sym, mode=mode, bandwidth=bandwidth, self=self,
                                 x_len=x_len)


def cross_similarity_batch(X, Y, *, k: Optional[int] = None, metric: str = "euclidean", mode: str = "connectivity",
                           bandwidth=None, x_len=None, y_len=None):
    """X [B, T, D], Y [B, T', D] (or [1, T', D]) float32 on the device -> [B, T, T'] float32: row i holds the k frames of Y
    nearest to frame i of X."""
    if Y is None:
        raise ValueError("cross_similarity_batch: Y must be a float32 tensor [B, T', D]")
    return ops.recurrence_matrix(X, Y, k=k, metric=metric, mode=mode, bandwidth=bandwidth, x_len=x_len, y_len=y_len)


def recurrence_matrix(data, k: Optional[int] = None, width: int = 1, metric: str = "euclidean", sym: bool = False,
                      mode: str = "connectivity", bandwidth=None, self: bool = False, sparse: bool = False):
    """librosa.segment.recurrence_matrix(data [d, t], k, width, metric, sym, sparse=False, mode, bandwidth, self) ->
    [t, t] float32 NumPy, R[i, j] non-zero when frame i is one of the k nearest neighbours of frame j."""
    who = "recurrence_matrix"
    if sparse:
        raise ValueError(f"{who}: sparse outputs are not served; the matrix is dense")
    X = _features(who, data)
    ops._sim_metric(who, metric)
    ops._sim_name(who, "mode", mode, ops.SIM_MODES)
    ops._sim_int(who, "width", width, 1, 1 << 30)
    if k is not None:
        ops._sim_int(who, "k", k, 1, ops.K_MAX)
    dev = ops.require_gpu()
    out = recurrence_matrix_batch(X.to(dev), k=k, width=width, metric=metric, sym=sym, mode=mode, bandwidth=bandwidth, self=self)
    return out[0].T.contiguous().cpu().numpy()


def cross_similarity(data, data_ref, k: Optional[int] = None, metric: str = "euclidean", mode: str = "connectivity",
                     bandwidth=None, sparse: bool = False):
    """librosa.segment.cross_similarity(data [d, n], data_ref [d, n_ref]) -> [n_ref, n] float32 NumPy, non-zero at (i, j)
    when frame i of data_ref is one of the k frames of data_ref nearest to frame j of data."""
    who = "cross_similarity"
    if sparse:
        raise ValueError(f"{who}: sparse outputs are not served; the matrix is dense")
    X, Y = _features(who, data), _features(who, data_ref, "data_ref")
    if X.shape[2] != Y.shape[2]:
        raise ValueError(f"{who}: data and data_ref must have the same number of features (got {X.shape[2]} and {Y.shape[2]})")
    ops._sim_metric(who, metric)
    ops._sim_name(who, "mode", mode, ops.SIM_MODES)
    if k is not None:
        ops._sim_int(who, "k", k, 1, ops.K_MAX)
    dev = ops.require_gpu()
    out = cross_similarity_batch(X.to(dev), Y.to(dev), k=k, metric=metric, mode=mode, bandwidth=bandwidth)
    return out[0].T.contiguous().cpu().numpy()
