"""Float64 restatement of the feature dynamics (sygnals_amd/csrc/dynamics.hip): the contract the device is held to.

delta: convolution with savgol_coeffs + the interp edge matrix + index maps for the other modes; pinned to
scipy.signal.savgol_filter by tests/test_dynamics_ref.py.  cmvn: the per-frame loop over explicit windows is the
definition (Kaldi's centred window); the prefix-sum form is what the larger GPU cases are compared with.  stack_memory:
the formula."""
import numpy as np
from scipy.signal import savgol_coeffs, savgol_filter

VAR_FLOOR = 1e-20
DIRECT_WINDOW = 32          # ops.dynamics_constants()["direct_window"]


def tables(width, order):
    """(c [width], E [width, width]) in float64."""
    c = savgol_coeffs(width, order, deriv=order)
    E = savgol_filter(np.eye(width), width, deriv=order, polyorder=order, axis=-1, mode="interp")
    return c, E


def norm1(width, order):
    return float(np.sum(np.abs(savgol_coeffs(width, order, deriv=order))))


def map_index(idx, T, mode):
    """Positions idx (any integers) -> indices into [0, T); -1 where the constant stands."""
    idx = np.asarray(idx, dtype=np.int64)
    if mode == "nearest":
        return np.clip(idx, 0, T - 1)
    if mode == "wrap":
        return np.mod(idx, T)
    if mode == "mirror":
        if T == 1:
            return np.zeros_like(idx)
        p = 2 * (T - 1)
        r = np.mod(idx, p)
        return np.where(r < T, r, p - r)
    if mode == "constant":
        return np.where((idx >= 0) & (idx < T), idx, -1)
    raise ValueError(mode)


def delta(x, width=9, order=1, mode="interp", cval=0.0, c=None, E=None):
    """The restatement along the last axis of x (any leading axes), float64 (or the dtype of the given tables: pass float32
    tables widened to float64 to see what the device's rounded tables compute)."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    h = width // 2
    if c is None:
        c, E = tables(width, order)
    c = np.asarray(c, dtype=np.float64)
    w = c[::-1]
    y = np.empty_like(x)
    if mode == "interp":
        if T < width:
            raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
        E = np.asarray(E, dtype=np.float64)
        if T > 2 * h:
            win = np.lib.stride_tricks.sliding_window_view(x, width, axis=-1)          # [..., T - 2h, width]
            y[..., h:T - h] = win @ w
        y[..., :h] = x[..., :width] @ E[:, :h]
        y[..., T - h:] = x[..., T - width:] @ E[:, width - h:]
        return y
    idx = map_index(np.arange(T)[:, None] - h + np.arange(width)[None, :], T, mode)    # [T, width]
    g = np.where(idx >= 0, x[..., np.maximum(idx, 0)], cval)                           # [..., T, width]
    return g @ w


def window_of(t, W, T):
    s = t - W // 2
    e = s + W
    if s < 0:
        e -= s
        s = 0
    if e > T:
        s -= e - T
        e = T
    if s < 0:
        s = 0
    return s, e


def windows(T, W):
    """(s [T], e [T]) of every frame, vectorised; W None: all frames."""
    if W is None or W >= T:
        return np.zeros(T, dtype=np.int64), np.full(T, T, dtype=np.int64)
    t = np.arange(T, dtype=np.int64)
    s = t - W // 2
    e = s + W
    neg = s < 0
    e = np.where(neg, e - s, e)
    s = np.where(neg, 0, s)
    over = e > T
    s = np.where(over, s - (e - T), s)
    e = np.where(over, T, e)
    return np.maximum(s, 0), e


def cmvn_loop(x, window=None, variance=True):
    """The definition: per row, per frame, the mean and the population variance over the explicit window, float64."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    flat = x.reshape(-1, T)
    y = np.empty_like(flat)
    W = T if window is None else window
    for t in range(T):
        s, e = window_of(t, W, T)
        seg = flat[:, s:e]
        m = seg.sum(axis=1) / (e - s)
        d = flat[:, t] - m
        if variance:
            v = ((seg - m[:, None]) ** 2).sum(axis=1) / (e - s)
            d = d / np.sqrt(np.maximum(v, VAR_FLOOR))
        y[:, t] = d
    return y.reshape(x.shape)


def cmvn_prefix(x, window=None, variance=True):
    """The same from float64 prefix sums of x and x^2 (v = E[x^2] - m^2).  Windows up to DIRECT_WINDOW frames go to the
    loop, as on the device: two or three frames of a c0-like row can lie within 1e-2 of each other, and E[x^2] - m^2 then
    keeps only a few digits of v whatever the precision of the sums."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    if window is not None and window <= DIRECT_WINDOW and window < T:
        return cmvn_loop(x, window, variance)
    s, e = windows(T, window)
    n = (e - s).astype(np.float64)
    zero = np.zeros(x.shape[:-1] + (1,))
    S = np.concatenate([zero, np.cumsum(x, axis=-1)], axis=-1)
    m = (S[..., e] - S[..., s]) / n
    y = x - m
    if variance:
        Q = np.concatenate([zero, np.cumsum(x * x, axis=-1)], axis=-1)
        v = (Q[..., e] - Q[..., s]) / n - m * m
        y = y / np.sqrt(np.maximum(v, VAR_FLOOR))
    return y


def stack_memory(x, n_steps=2, delay=1):
    """out[..., i K + k, t] = x[..., k, t - i delay], 0 outside [0, T): the formula, element by element over (i, shift)."""
    x = np.asarray(x)
    K, T = x.shape[-2:]
    out = np.zeros(x.shape[:-2] + (n_steps * K, T), dtype=x.dtype)
    for i in range(n_steps):
        sh = i * delay
        t = np.arange(T)
        ok = (t - sh >= 0) & (t - sh < T)
        out[..., i * K:(i + 1) * K, t[ok]] = x[..., :, t[ok] - sh]
    return out


def feature_post(x32, cmvn=None, variance=True, deltas=2, width=9, mode="interp"):
    """[statics | delta | delta2] in float64 from float32 statics (the deltas read the ROUNDED statics)."""
    s = np.asarray(x32, dtype=np.float32)
    if cmvn is not None:
        s = cmvn_prefix(s, None if cmvn == "global" else cmvn, variance).astype(np.float32)
    blocks = [s.astype(np.float64)] + [delta(s, width, d, mode) for d in range(1, deltas + 1)]
    return np.concatenate(blocks, axis=-2)
