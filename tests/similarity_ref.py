"""Float64 restatement of the self-similarity functions (the contract of csrc/similarity.hip): k nearest frames,
recurrence matrix, nn_filter, the REPET-SIM masks and the separation built on them.  Frame-major like the device code:
X [T, D] are the query frames of ONE clip, Y [T', D] the frames searched.  The lists are pinned to scikit-learn's brute
NearestNeighbors and the distances to scipy's cdist in tests/test_similarity_ref.py; librosa is not a dependency.

Definitions
  candidates   of row i: every j < y_len with Y given; the j with |i - j| >= width for self-similarity
  sqeuclidean  sum (x - y)^2;  euclidean its root;  cosine 1 - x.y / max(|x| |y|, FLT_MIN) (a zero frame is at distance 1
               from everything: scipy gives NaN there)
  list         the min(k, candidates) nearest candidates, ordered by distance, then by index
"""
from __future__ import annotations

import numpy as np

from tests import hpss_ref as HR

K_MAX = 256
METRICS = ("euclidean", "sqeuclidean", "cosine")
FLT_MIN = float(np.finfo(np.float32).tiny)


def default_k(T, width=1):
    """librosa's rule: 2 ceil(sqrt(T - 2 width + 1)), at least 1, at most K_MAX."""
    return int(min(K_MAX, max(1, 2 * int(np.ceil(np.sqrt(max(1, T - 2 * width + 1)))))))


def distances(X, Y, metric):
    """[T, T'] float64, in difference form (no cancellation)."""
    if metric not in METRICS:
        raise ValueError(f"metric={metric!r} is not served; served: {', '.join(METRICS)}")
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if metric == "cosine":
        nx = np.sqrt(np.sum(X * X, axis=1))
        ny = np.sqrt(np.sum(Y * Y, axis=1))
        return 1.0 - (X @ Y.T) / np.maximum(nx[:, None] * ny[None, :], FLT_MIN)
    d2 = np.zeros((X.shape[0], Y.shape[0]))
    for lo in range(0, X.shape[0], 64):                                  # [64, T', D] at a time
        e = X[lo:lo + 64, None, :] - Y[None, :, :]
        d2[lo:lo + 64] = np.sum(e * e, axis=2)
    return np.sqrt(d2) if metric == "euclidean" else d2


def candidate_mask(T, Ty, width, self_sim, x_len=None, y_len=None):
    """[T, T'] bool: j is a candidate of row i."""
    x_len = T if x_len is None else int(x_len)
    y_len = (x_len if self_sim else Ty) if y_len is None else int(y_len)
    i = np.arange(T)[:, None]
    j = np.arange(Ty)[None, :]
    ok = (i < x_len) & (j < y_len)
    if self_sim:
        ok &= np.abs(i - j) >= width
    return ok


def lists_from(Dm, ok, k):
    """(idx [T, k] int32, dist [T, k] float64, count [T] int32) of a distance matrix and its candidate mask: -1 / +inf
    past the count."""
    T = Dm.shape[0]
    idx = np.full((T, k), -1, dtype=np.int32)
    dist = np.full((T, k), np.inf)
    count = np.zeros(T, dtype=np.int32)
    for i in range(T):
        js = np.nonzero(ok[i])[0]
        order = js[np.lexsort((js, Dm[i, js]))][:k]
        c = len(order)
        idx[i, :c] = order
        dist[i, :c] = Dm[i, order]
        count[i] = c
    return idx, dist, count


def knn(X, Y=None, k=None, width=1, metric="euclidean", x_len=None, y_len=None):
    """The lists of one clip."""
    X = np.asarray(X)
    self_sim = Y is None
    if width < 1 or (not self_sim and width != 1):
        raise ValueError("width must be >= 1, and 1 with Y")
    Ys = X if self_sim else np.asarray(Y)
    T, Ty = X.shape[0], Ys.shape[0]
    k = default_k(T, width) if k is None else int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError(f"k must be in [1, {K_MAX}]")
    return lists_from(distances(X, Ys, metric), candidate_mask(T, Ty, width, self_sim, x_len, y_len), k)


def boundary_gaps(X, Y=None, k=None, width=1, metric="euclidean", x_len=None, y_len=None):
    """(gap [T], scale): the float64 distance from the k-th to the (k + 1)-th candidate of each row (+inf where the row
    keeps every candidate) and the clip's largest kept distance, the scale of the gates."""
    X = np.asarray(X)
    self_sim = Y is None
    Ys = X if self_sim else np.asarray(Y)
    T, Ty = X.shape[0], Ys.shape[0]
    k = default_k(T, width) if k is None else int(k)
    Dm = distances(X, Ys, metric)
    ok = candidate_mask(T, Ty, width, self_sim, x_len, y_len)
    gap = np.full(T, np.inf)
    scale = 0.0
    for i in range(T):
        d = np.sort(Dm[i, ok[i]])
        if len(d) > k:
            gap[i] = d[k] - d[k - 1]
        if len(d):
            scale = max(scale, float(d[:k][-1]))
    return gap, scale


def mutual(idx, count):
    """keep [T, k] bool: entry (i, e) has i in the list of idx[i, e] as well."""
    T, k = idx.shape
    keep = np.zeros((T, k), dtype=bool)
    for i in range(T):
        for e in range(count[i]):
            j = idx[i, e]
            keep[i, e] = i in idx[j, :count[j]]
    return keep


def bandwidth_of(dist, count, keep=None):
    """numpy's median, over the rows that kept a link, of the row's largest kept distance (float64).  1.0 for a clip
    without a link; 0 raises ValueError."""
    mx = []
    for i in range(dist.shape[0]):
        d = [float(dist[i, e]) for e in range(count[i]) if keep is None or keep[i, e]]
        if d:
            mx.append(max(d))
    bw = float(np.median(np.asarray(mx, dtype=np.float64))) if mx else 1.0
    if bw == 0:
        raise ValueError("the default bandwidth is 0")
    return bw


def dense(idx, dist, count, n_cols=None, mode="connectivity", sym=False, bandwidth=None, self=False):
    """(R [T, n_cols] float64, bandwidth or None) from the lists."""
    if mode not in ("connectivity", "distance", "affinity"):
        raise ValueError(f"mode={mode!r} is not served")
    T, k = idx.shape
    n_cols = T if n_cols is None else n_cols
    keep = mutual(idx, count) if sym else None
    bw = None
    if mode == "affinity":
        bw = bandwidth_of(dist, count, keep) if bandwidth is None else float(bandwidth)
    R = np.zeros((T, n_cols))
    for i in range(T):
        for e in range(count[i]):
            if keep is not None and not keep[i, e]:
                continue
            d = float(dist[i, e])
            R[i, idx[i, e]] = 1.0 if mode == "connectivity" else d if mode == "distance" else np.exp(-d / bw)
    if self:
        R[np.arange(T), np.arange(T)] = 0.0 if mode == "distance" else 1.0
    return R, bw


def recurrence_matrix(X, Y=None, k=None, width=1, metric="euclidean", sym=False, mode="connectivity", bandwidth=None,
                      self=False):
    idx, dist, count = knn(X, Y, k, width, metric)
    return dense(idx, dist, count, None if Y is None else np.asarray(Y).shape[0], mode, sym, bandwidth, self)[0]


def nn_filter(S, idx, count, weights=None, aggregate="mean"):
    """S [T, F] -> [T, F] float64 (median: the dtype of S, as numpy's median of float32 values is float32)."""
    if aggregate not in ("mean", "average", "median"):
        raise ValueError(f"aggregate={aggregate!r} is not served")
    S = np.asarray(S)
    out = np.array(S, dtype=S.dtype if aggregate == "median" else np.float64)
    for i in range(S.shape[0]):
        c = int(count[i])
        if c == 0:
            continue
        rows = S[idx[i, :c]]
        if aggregate == "median":
            out[i] = np.median(rows, axis=0)
        elif aggregate == "mean":
            out[i] = np.mean(rows.astype(np.float64), axis=0)
        else:
            w = np.asarray(weights[i, :c], dtype=np.float64)
            if w.sum() != 0:
                out[i] = (w[:, None] * rows.astype(np.float64)).sum(axis=0) / w.sum()
    return out


def repet_masks(S, R, margin_b=2.0, margin_f=10.0, power=2.0):
    """(mask_f, mask_b) float64 from float32 magnitudes S and their filtered version R."""
    S = np.asarray(S, dtype=np.float32)
    Sf = np.minimum(S, np.asarray(R, dtype=np.float32))
    rest = S - Sf
    mask_b = HR.softmask(Sf, np.float32(margin_b) * rest, power)
    mask_f = HR.softmask(rest, np.float32(margin_f) * Sf, power)
    return mask_f, mask_b


def default_width(sr):
    return max(1, int(round(2.0 * sr / 512)))


def separate_from(Dc, idx, count, length, margin_b=2.0, margin_f=10.0, power=2.0):
    """(foreground, background) float64 of one clip from its complex STFT Dc [T, 1025] and the lists: median nn_filter of
    the float32 magnitudes, the masks, the inverse STFT."""
    S = np.abs(Dc).astype(np.float32)
    R = nn_filter(S, idx, count, aggregate="median")
    mf, mb = repet_masks(S, R, margin_b, margin_f, power)
    return HR.istft((mf * Dc).T, length), HR.istft((mb * Dc).T, length)
