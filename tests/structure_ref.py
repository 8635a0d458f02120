"""Float64 restatement of librosa.segment's structure functions, the contract of csrc/structure.hip.  librosa is not
installed with the tests, so each function restates librosa 0.10's source and tests/test_structure_ref.py pins it to what
is: np.roll, scipy.ndimage.rotate / convolve / median_filter and scikit-learn's AgglomerativeClustering."""
import numpy as np

MODES = ("reflect", "mirror", "nearest", "wrap", "constant", "grid-wrap", "grid-constant")


# ------------------------------------------------------------------ shear (librosa.segment.recurrence_to_lag / lag_to_recurrence)
def recurrence_to_lag(rec, pad=True, axis=-1):
    axis = abs(axis)
    rec = np.asarray(rec)
    t = rec.shape[axis]
    if rec.ndim != 2 or rec.shape[0] != rec.shape[1]:
        raise ValueError("non-square recurrence matrix")
    if pad:
        padding = [(0, 0), (0, 0)]
        padding[1 - axis] = (0, t)
        rec = np.pad(rec, padding, mode="constant")
    lag = rec.copy()
    sl = [slice(None)] * 2
    for i in range(1, t):
        sl[axis] = i
        lag[tuple(sl)] = np.roll(lag[tuple(sl)], -i)
    return lag


def lag_to_recurrence(lag, axis=-1):
    axis = abs(axis)
    lag = np.asarray(lag)
    t = lag.shape[axis]
    if lag.ndim != 2 or lag.shape[1 - axis] not in (t, 2 * t):
        raise ValueError("invalid lag matrix shape")
    rec = lag.copy()
    sl = [slice(None)] * 2
    for i in range(1, t):
        sl[axis] = i
        rec[tuple(sl)] = np.roll(rec[tuple(sl)], i)
    sub = [slice(None)] * 2
    sub[1 - axis] = slice(t)
    return np.ascontiguousarray(rec[tuple(sub)])


# ------------------------------------------------------------------ boundary rules as index maps (scipy.ndimage's)
def boundary_index(x, n, mode):
    """Source index of positions x of an axis of n under scipy.ndimage's rule; -1 where the constant fills."""
    x = np.asarray(x, dtype=np.int64)
    if mode in ("constant", "grid-constant"):
        return np.where((x >= 0) & (x < n), x, -1)
    if mode == "nearest":
        return np.clip(x, 0, n - 1)
    if mode in ("wrap", "grid-wrap"):
        return np.mod(x, n)
    if mode == "reflect":
        p = np.mod(x, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p)
    if mode == "mirror":
        if n == 1:
            return np.zeros_like(x)
        p = np.mod(x, 2 * n - 2)
        return np.where(p < n, p, 2 * n - 2 - p)
    raise ValueError(mode)


# ------------------------------------------------------------------ path_enhance
def diagonal_filter(window, n, slope=1.0, zero_mean=False):
    """librosa.segment.diagonal_filter."""
    from scipy.ndimage import rotate
    from scipy.signal import get_window
    angle = np.arctan(slope)
    win = np.diag(get_window(window, n, fftbins=False))
    if not np.isclose(angle, np.pi / 4):
        win = rotate(win, 45 - angle * 180 / np.pi, order=5, prefilter=False)
    np.clip(win, 0, None, out=win)
    win /= win.sum()
    if zero_mean:
        win -= win.mean()
    return win


def filter_bank(n, window="hann", max_ratio=2.0, min_ratio=None, n_filters=7, zero_mean=False):
    if min_ratio is None:
        min_ratio = 1.0 / max_ratio
    elif min_ratio > max_ratio:
        raise ValueError("min_ratio cannot exceed max_ratio")
    return [diagonal_filter(window, n, slope=r, zero_mean=zero_mean)
            for r in np.logspace(np.log2(min_ratio), np.log2(max_ratio), num=n_filters, base=2)]


def path_enhance(R, n, window="hann", max_ratio=2.0, min_ratio=None, n_filters=7, zero_mean=False, clip=True, **kwargs):
    """librosa.segment.path_enhance in float64: scipy.ndimage.convolve with every filter, the running maximum, the clip."""
    from scipy.ndimage import convolve
    R = np.asarray(R, dtype=np.float64)
    out = None
    for ker in filter_bank(n, window, max_ratio, min_ratio, n_filters, zero_mean):
        c = convolve(R, ker, **kwargs)
        out = c if out is None else np.maximum(out, c)
    if clip:
        np.clip(out, 0, None, out=out)
    return out


def taps_correlate(R, dr, dc, w, mode="reflect", cval=0.0):
    """sum_e w[e] R~[r + dr[e], c + dc[e]] in float64, R~ extended by boundary_index: the form the kernel computes."""
    R = np.asarray(R, dtype=np.float64)
    T, Tc = R.shape
    out = np.zeros((T, Tc))
    rr, cc = np.arange(T), np.arange(Tc)
    for a, b, wt in zip(dr, dc, w):
        mr, mc = boundary_index(rr + a, T, mode), boundary_index(cc + b, Tc, mode)
        v = R[np.maximum(mr, 0)[:, None], np.maximum(mc, 0)[None, :]]
        v = np.where((mr < 0)[:, None] | (mc < 0)[None, :], float(cval), v)
        out += wt * v
    return out


# ------------------------------------------------------------------ diagonal median
def ord_keys(a32):
    """float32 -> uint32 keys in the order of the values, -0 below +0."""
    u = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def keys_value(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def diag_median(R, w, mode="reflect", cval=0.0, pad=True, axis=-1):
    """timelag_filter(median_filter, pad)(R, size=(1, w) [axis 0: (w, 1)], mode, cval) on float32: shear, the median of
    every window along time as an input value (keys order the values, -0 below +0), shear back."""
    R = np.asarray(R, dtype=np.float32)
    ax = abs(axis)
    lag = recurrence_to_lag(R, pad=pad, axis=ax)
    if ax == 0:
        lag = lag.T                                           # [n, t]: time along the columns
    t = lag.shape[1]
    idx = boundary_index(np.arange(t)[:, None] + np.arange(w)[None, :] - w // 2, t, mode)          # [t, w]
    win = lag[:, np.maximum(idx, 0)]                                                                # [n, t, w]
    win = np.where((idx < 0)[None], np.float32(cval), win).astype(np.float32)
    med = keys_value(np.sort(ord_keys(win), axis=-1)[..., w // 2])
    if ax == 0:
        med = med.T
    return lag_to_recurrence(np.ascontiguousarray(med), axis=ax)


def diag_median_scipy(R, w, mode="reflect", cval=0.0, pad=True, axis=-1):
    """The same through scipy.ndimage.median_filter, as librosa.segment.timelag_filter runs it.  Under axis 0 the filter runs
    on the transposed lag matrix with size (1, w), which is the same filter: SciPy 1.15's size (w, 1) reads past a short
    axis (a 2 x 4 matrix under w = 31 gave 6.7e-33 in a cell, and not on every run)."""
    from scipy.ndimage import median_filter
    ax = abs(axis)
    lag = recurrence_to_lag(np.asarray(R, dtype=np.float32), pad=pad, axis=ax)
    lag = lag if ax == 1 else np.ascontiguousarray(lag.T)
    t, h = lag.shape[1], w // 2
    if h <= t:
        f = median_filter(lag, size=(1, w), mode=mode, cval=cval)
    else:
        # a window that folds the row more than once: SciPy 1.15 answered a 2 x 2 matrix under w = 31 wrongly, so the row is
        # extended here by np.pad's rule of the same name and the filter runs on the inside of it
        how = {"reflect": "symmetric", "mirror": "reflect", "nearest": "edge", "wrap": "wrap", "grid-wrap": "wrap"}.get(mode, "constant")
        kw = dict(constant_values=np.float32(cval)) if how == "constant" else {}
        ext = np.pad(lag, ((0, 0), (h, h)), mode=how, **kw) if t > 1 or how in ("edge", "constant", "wrap") else np.repeat(lag, w, axis=1)
        f = median_filter(ext, size=(1, w), mode="nearest")[:, h:h + t]
    f = np.ascontiguousarray(f if ax == 1 else f.T)
    return lag_to_recurrence(f, axis=ax)


# ------------------------------------------------------------------ chain Ward
def chain_ward(X, k):
    """Ward clustering of the chain of frames X [T, D] (float64 arithmetic): the neighbouring pair with the least
    n_a n_b / (n_a + n_b) |S_a / n_a - S_b / n_b|^2 is merged, the leftmost on ties, until k segments remain.
    -> (segment starts, the least relative gap between the best and the second-best cost over the run; inf if none)."""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    if not 1 <= k <= T:
        raise ValueError("k must be in [1, T]")
    S = X.copy()
    nxt = np.arange(1, T + 1)
    prv = np.arange(-1, T - 1)
    cost = np.full(T, np.inf)
    if T > 1:
        cost[:-1] = 0.5 * ((X[:-1] - X[1:]) ** 2).sum(axis=1)

    def ward(a, b):
        na, nb = nxt[a] - a, nxt[b] - b
        d = S[a] / na - S[b] / nb
        return na * nb / (na + nb) * float(d @ d)
    gap = np.inf
    for live in range(T, k, -1):
        a = int(np.argmin(cost))
        if live > 2:
            two = np.partition(cost, 1)[:2]
            if np.isfinite(two[1]):
                gap = min(gap, (two[1] - two[0]) / two[1] if two[1] > 0 else 0.0)
        b = nxt[a]
        c = nxt[b]
        S[a] += S[b]
        nxt[a] = c
        if c < T:
            prv[c] = a
        cost[b] = np.inf
        cost[a] = ward(a, c) if c < T else np.inf
        p = prv[a]
        if p >= 0:
            cost[p] = ward(p, a)
    bounds, a = [], 0
    while a < T:
        bounds.append(a)
        a = nxt[a]
    return np.asarray(bounds, dtype=np.int64), gap


def sklearn_ward(X, k):
    """librosa.segment.agglomerative's route: AgglomerativeClustering over the chain's grid connectivity."""
    from sklearn.cluster import AgglomerativeClustering
    from sklearn.feature_extraction.image import grid_to_graph
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    if n == 1:
        return np.array([0])
    labels = AgglomerativeClustering(n_clusters=k, connectivity=grid_to_graph(n_x=n, n_y=1, n_z=1)).fit(X).labels_
    return np.concatenate(([0], 1 + np.nonzero(np.diff(labels))[0])).astype(np.int64)


# ------------------------------------------------------------------ subsegment, sync
def fix_frames(frames, x_max, pad=True):
    f = np.asarray(frames)
    if np.any(f < 0):
        raise ValueError("negative frame index")
    if pad:
        f = np.concatenate(([0, x_max], np.clip(f, 0, x_max)))
    f = f[(f >= 0) & (f <= x_max)]
    return np.unique(f).astype(int)


def subsegment(X, frames, n_segments=4):
    """librosa.segment.subsegment on frame-major X [T, D]."""
    edges = fix_frames(frames, X.shape[0])
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        out.extend(lo + chain_ward(X[lo:hi], min(hi - lo, n_segments))[0])
    return np.asarray(out, dtype=np.int64)


def sync(X, edges, aggregate="mean"):
    """librosa.util.sync on frame-major X [T, D] over the segments [edges[j], edges[j + 1]): float64."""
    fn = {"mean": np.mean, "max": np.max, "min": np.min}[aggregate]
    X = np.asarray(X, dtype=np.float64)
    return np.stack([fn(X[lo:hi], axis=0) for lo, hi in zip(edges[:-1], edges[1:])])
