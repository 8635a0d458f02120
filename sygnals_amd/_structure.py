"""Host side of the structure analysis (csrc/structure.hip): the diagonal filter bank of path_enhance as tap lists, the
frame fixing of subsegment and sync, and the names served.  Pure NumPy / SciPy in float64; nothing here needs a device."""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

BOUNDARY_MODES = {"reflect": 0, "mirror": 1, "nearest": 2, "wrap": 3, "grid-wrap": 3, "constant": 4, "grid-constant": 4}
SYNC_AGGREGATES = {"mean": 0, "max": 1, "min": 2}
SERVED = ("served: dense float32 matrices, boundary rules " + ", ".join(repr(m) for m in BOUNDARY_MODES)
          + "; median windows odd and up to 63; sync aggregates 'mean', 'max', 'min'")

# taps   int32 [n_taps, 4]: (row offset, column offset, the float32 weight's bits, 0), filter after filter, each filter's in
#        ascending (row offset, column offset): the order the kernel sums them in
# fstart int32 [n_filters + 1]; span (dr_min, dr_max, dc_min, dc_max) over all taps
# w64    float64 [n_taps] the weights before their one rounding; kernels: the float64 filter arrays as librosa makes them
PathFilters = namedtuple("PathFilters", "taps fstart span w64 kernels")


def boundary_code(who: str, mode) -> int:
    if not isinstance(mode, str) or mode not in BOUNDARY_MODES:
        raise ValueError(f"{who}: mode={mode!r} is not served; served: {', '.join(repr(m) for m in BOUNDARY_MODES)}")
    return BOUNDARY_MODES[mode]


def diagonal_filter(window, n: int, slope: float = 1.0, zero_mean: bool = False) -> np.ndarray:
    """librosa.segment.diagonal_filter: the window on the diagonal of an n x n array, rotated to the slope with a quintic
    spline, clipped at 0 and normalised to sum 1."""
    from scipy.ndimage import rotate
    from scipy.signal import get_window
    angle = np.arctan(slope)
    win = np.diag(get_window(window, n, fftbins=False)).astype(np.float64)
    if not np.isclose(angle, np.pi / 4):
        win = rotate(win, 45 - angle * 180 / np.pi, order=5, prefilter=False)
    np.clip(win, 0, None, out=win)
    win /= win.sum()
    if zero_mean:
        win -= win.mean()
    return win


def kernel_taps(kernel: np.ndarray):
    """The taps of scipy.ndimage.convolve(., kernel): (dr, dc, w) lists with convolve(R)[r, c] = sum w R~[r + dr, c + dc].
    Read off convolve's own answer to a unit impulse, so that its flip, its centring and its origin shift at even sizes are
    whatever SciPy does: the impulse at P answers w at (P - dr, P - dc)."""
    from scipy.ndimage import convolve
    kh, kw = kernel.shape
    imp = np.zeros((2 * kh + 1, 2 * kw + 1))
    imp[kh, kw] = 1.0
    resp = convolve(imp, np.asarray(kernel, dtype=np.float64), mode="constant", cval=0.0)
    r, c = np.nonzero(resp)
    dr, dc, w = kh - r, kw - c, resp[r, c]
    order = np.lexsort((dc, dr))
    return dr[order].astype(np.int64), dc[order].astype(np.int64), w[order]


def path_ratios(max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7) -> np.ndarray:
    if isinstance(n_filters, bool) or not isinstance(n_filters, (int, np.integer)) or n_filters < 1:
        raise ValueError(f"path_enhance: n_filters={n_filters!r} must be a positive integer")
    if not np.isfinite(max_ratio) or max_ratio <= 0:
        raise ValueError(f"path_enhance: max_ratio={max_ratio!r} must be positive and finite")
    if min_ratio is None:
        min_ratio = 1.0 / max_ratio
    elif not np.isfinite(min_ratio) or min_ratio <= 0:
        raise ValueError(f"path_enhance: min_ratio={min_ratio!r} must be positive and finite")
    elif min_ratio > max_ratio:
        raise ValueError(f"path_enhance: min_ratio={min_ratio} cannot exceed max_ratio={max_ratio}")
    return np.logspace(np.log2(min_ratio), np.log2(max_ratio), num=int(n_filters), base=2)


def path_filters(n: int, window="hann", max_ratio: float = 2.0, min_ratio=None, n_filters: int = 7,
                 zero_mean: bool = False) -> PathFilters:
    """The filter bank of librosa.segment.path_enhance(n, window, max_ratio, min_ratio, n_filters, zero_mean) as the tap
    lists syg_path_enhance_f32 reads.  Kept per argument tuple."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"path_enhance: n={n!r} must be a positive integer")
    ratios = path_ratios(max_ratio, min_ratio, n_filters)            # (checks before the cache: its key must be hashable)
    wkey = window if isinstance(window, (str, tuple, int, float)) else tuple(np.asarray(window, dtype=np.float64).ravel().tolist())
    return _path_filters(int(n), wkey, tuple(ratios.tolist()), bool(zero_mean))


@lru_cache(maxsize=32)
def _path_filters(n, window, ratios, zero_mean) -> PathFilters:
    if isinstance(window, tuple) and len(window) == n and all(isinstance(v, float) for v in window):
        window = np.asarray(window)
    kernels, rows, w64, fstart = [], [], [], [0]
    for ratio in ratios:
        ker = diagonal_filter(window, n, slope=ratio, zero_mean=zero_mean)
        dr, dc, w = kernel_taps(ker)
        kernels.append(ker)
        rows.append(np.stack([dr, dc], axis=1))
        w64.append(w)
        fstart.append(fstart[-1] + len(w))
    off = np.concatenate(rows)
    w64 = np.concatenate(w64)
    taps = np.zeros((len(w64), 4), dtype=np.int32)
    taps[:, :2] = off
    taps[:, 2] = w64.astype(np.float32).view(np.int32)
    span = (int(off[:, 0].min()), int(off[:, 0].max()), int(off[:, 1].min()), int(off[:, 1].max()))
    for a in (taps, w64):
        a.setflags(write=False)
    return PathFilters(taps, np.asarray(fstart, dtype=np.int32), span, w64, tuple(kernels))


def fix_frames(frames, x_max: int, pad: bool = True) -> np.ndarray:
    """librosa.util.fix_frames(frames, x_min=0, x_max, pad): unique and sorted; with pad clipped to [0, x_max] and both ends
    added, without it the frames past x_max dropped.  Negative frames raise, as in librosa."""
    f = np.asarray(frames)
    if f.ndim != 1 or f.dtype.kind not in "iu":
        raise ValueError("frames must be a one-dimensional array of integers")
    if np.any(f < 0):
        raise ValueError("negative frame index detected")
    if pad:
        f = np.concatenate(([0, x_max], np.clip(f, 0, x_max)))
    f = f[(f >= 0) & (f <= x_max)]
    return np.unique(f).astype(np.int64)
