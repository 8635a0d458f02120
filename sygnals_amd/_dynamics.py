"""Host side of the feature dynamics (csrc/dynamics.hip): the Savitzky-Golay tables of `delta` and the argument rules.

delta(x, width, order, mode) is librosa.feature.delta, that is scipy.signal.savgol_filter(x, width, deriv=order,
polyorder=order, mode=mode).  With h = width // 2 and c = savgol_coeffs(width, order, deriv=order):
    interior frames h <= t < T - h:  np.convolve(x, c, "valid")
    interp edges:  y[:h] = x[:width] @ E[:, :h],  y[-h:] = x[-width:] @ E[:, -h:]
    E = savgol_filter(eye(width), width, deriv=order, polyorder=order, mode="interp")
The tables are made in float64 and rounded once to float32; no device is needed here."""
from __future__ import annotations

import functools

import numpy as np

MODES = {"interp": 0, "nearest": 1, "mirror": 2, "wrap": 3, "constant": 4}
WIDTH_MAX = 255
ORDER_MAX = 4
MAX_OUT = 1 << 31


def check_width_order(width, order, who: str = "delta"):
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 3 or width % 2 != 1 or width > WIDTH_MAX:
        raise ValueError(f"{who}: width must be an odd integer in [3, {WIDTH_MAX}] (got {width!r})")
    top = min(ORDER_MAX, int(width) - 1)
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= top:
        raise ValueError(f"{who}: order must be an integer in [1, min({ORDER_MAX}, width - 1) = {top}] (got {order!r})")
    return int(width), int(order)


def check_mode(mode, who: str = "delta") -> int:
    if mode not in MODES:
        raise ValueError(f"{who}: unknown mode {mode!r} (served: {', '.join(MODES)})")
    return MODES[mode]


def check_interp(width: int, T: int, mode: str, who: str = "delta") -> None:
    if mode == "interp" and T < width:
        raise ValueError(f"{who}: If mode is 'interp', window_length must be less than or equal to the size of x "
                         f"(width = {width}, frames = {T})")


def check_window(window, who: str = "cmvn") -> int:
    """None -> 0 (all frames); an integer >= 1 -> itself."""
    if window is None:
        return 0
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"{who}: window must be None (all frames) or an integer >= 1 (got {window!r})")
    return int(window)


def check_stack(n_steps, delay, who: str = "stack_memory"):
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
        raise ValueError(f"{who}: n_steps must be an integer >= 1 (got {n_steps!r})")
    if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or delay == 0:
        raise ValueError(f"{who}: delay must be a non-zero integer, either sign (got {delay!r})")
    return int(n_steps), int(delay)


def check_size(who: str, B: int, rows: int, T: int) -> None:
    if min(B, rows, T) < 1:
        raise ValueError(f"{who}: empty input (shape [{B}, {rows}, {T}])")
    if B * rows * T > MAX_OUT:
        raise ValueError(f"{who}: a result of {B * rows * T} elements is above 2^31 = {MAX_OUT}")


@functools.lru_cache(maxsize=None)
def delta_tables64(width: int, order: int):
    """(c [width], E [width, width]) in float64."""
    from scipy.signal import savgol_coeffs, savgol_filter
    width, order = check_width_order(width, order)
    c = savgol_coeffs(width, order, deriv=order)
    E = savgol_filter(np.eye(width), width, deriv=order, polyorder=order, axis=-1, mode="interp")
    c.setflags(write=False)
    E.setflags(write=False)
    return c, E


@functools.lru_cache(maxsize=None)
def delta_tables(width: int, order: int):
    """(c, E) rounded once to float32, cached per (width, order)."""
    c, E = delta_tables64(width, order)
    c32, E32 = c.astype(np.float32), E.astype(np.float32)
    c32.setflags(write=False)
    E32.setflags(write=False)
    return c32, E32


def pack_table(width: int, order: int) -> np.ndarray:
    """The device table of one delta block, width^2 float32: w [width] = c reversed (y[t] = sum_j w[j] x[t - h + j]), the
    left edge rows [h][width] (row t: E[:, t]), the right edge rows [h][width] (row q: E[:, width - h + q])."""
    c, E = delta_tables(width, order)
    h = width // 2
    return np.concatenate([c[::-1], E[:, :h].T.ravel(), E[:, width - h:].T.ravel()]).astype(np.float32)
