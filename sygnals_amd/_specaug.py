"""Host side of SpecAugment (csrc/spec_augment.hip): the argument rules and the per-clip draws in exact integer NumPy.
Pure host logic: no torch, no library.

Clip b is generator row r = first_row + b of stream STREAM_SPEC.  Item q is one Philox call at counter (q, 0, r, 2) with
key `seed`, of which words w0 and w1 are used; draw(w, n) = (uint64(w) n) >> 32, in [0, n) and 0 for n = 0:
    warp (q = 0), only if W > 0 and T_b > 2 W:   c = W + draw(w0, T_b - 2 W),  w' = c - W + 1 + draw(w1, 2 W)
    frequency mask i (q = 1 + i):                f = draw(w0, F + 1),  f0 = draw(w1, K - f + 1)      rows [f0, f0 + f)
    time mask j (q = 17 + j):                    We = min(Wt, floor(p T_b)),  t = draw(w0, We + 1),  t0 = draw(w1, T_b - t + 1)
`params` is what the device draws, so a training loop can log or reuse the masks; tests/specaug_ref.py is the
independent restatement."""
from __future__ import annotations

import math

import numpy as np

from . import _rng

STREAM_SPEC = 2
MAX_MASKS = 16
Q_WARP, Q_FREQ, Q_TIME = 0, 1, 17
MAX_ELEMS = 1 << 31
MODES = ("linear",)
_S32 = np.uint64(32)


def _integer(v, what: str, who: str) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{who}: {what} must be an integer (got {v!r})")
    return int(v)


def check_mode(mode, who: str = "spec_augment") -> None:
    if mode == "bicubic":
        raise ValueError(f"{who}: mode 'bicubic' is not served (the time warp is piecewise 'linear')")
    if mode not in MODES:
        raise ValueError(f"{who}: unknown mode {mode!r} (served: 'linear')")


def check_mask_value(mask_value, who: str = "spec_augment"):
    """(mean, value): (True, 0.0) for "mean", (False, the finite float) otherwise."""
    if isinstance(mask_value, str):
        if mask_value != "mean":
            raise ValueError(f"{who}: mask_value must be a finite float or 'mean' (got {mask_value!r})")
        return True, 0.0
    if isinstance(mask_value, (bool, np.bool_)) or not isinstance(mask_value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}: mask_value must be a finite float or 'mean' (got {mask_value!r})")
    value = float(mask_value)
    with np.errstate(over="ignore"):
        fits = math.isfinite(value) and math.isfinite(float(np.float32(value)))      # the device holds it as float32
    if not fits:
        raise ValueError(f"{who}: mask_value must be a finite float or 'mean' (got {mask_value!r})")
    return False, value


def check_args(K: int, T: int, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, who: str = "spec_augment"):
    """The per-call parameters against the clip shape [K, T]: (freq_masks, F, time_masks, Wt, p, W) as Python numbers."""
    nf, nt = _integer(freq_masks, "freq_masks", who), _integer(time_masks, "time_masks", who)
    if not 0 <= nf <= MAX_MASKS:
        raise ValueError(f"{who}: freq_masks must lie in 0 .. {MAX_MASKS} (got {nf})")
    if not 0 <= nt <= MAX_MASKS:
        raise ValueError(f"{who}: time_masks must lie in 0 .. {MAX_MASKS} (got {nt})")
    F = _integer(freq_width, "freq_width", who)
    if not 0 <= F <= K:
        raise ValueError(f"{who}: freq_width must lie in [0, K = {K}] (got {F})")
    Wt, W = _integer(time_width, "time_width", who), _integer(time_warp, "time_warp", who)
    if Wt < 0:
        raise ValueError(f"{who}: time_width must not be negative (got {Wt})")
    if W < 0:
        raise ValueError(f"{who}: time_warp must not be negative (got {W})")
    if isinstance(time_ratio, (bool, np.bool_)) or not isinstance(time_ratio, (int, float, np.integer, np.floating)) \
            or not 0.0 < float(time_ratio) <= 1.0:                       # (NaN fails both comparisons)
        raise ValueError(f"{who}: time_ratio must lie in (0, 1] (got {time_ratio!r})")
    return nf, F, nt, min(Wt, T), float(time_ratio), min(W, T)


def check_shape(B: int, K: int, T: int, who: str = "spec_augment") -> None:
    if min(B, K, T) < 1:
        raise ValueError(f"{who}: empty input (shape [{B}, {K}, {T}])")
    if B * K * T > MAX_ELEMS:
        raise ValueError(f"{who}: {B * K * T} elements are above 2^31 = {MAX_ELEMS}")


def check_lengths(lengths, B: int, T: int, who: str = "spec_augment") -> np.ndarray:
    """int64 [B], every entry in [1, T]; None: T everywhere."""
    if lengths is None:
        return np.full(B, T, dtype=np.int64)
    a = np.asarray(lengths)
    if a.shape != (B,) or a.dtype.kind not in "iu":
        raise ValueError(f"{who}: lengths must be {B} integers, one per clip (got shape {list(a.shape)}, dtype {a.dtype})")
    a = a.astype(np.int64)
    if a.min() < 1 or a.max() > T:
        raise ValueError(f"{who}: lengths must lie in [1, T = {T}] (got {int(a.min())} .. {int(a.max())})")
    return a


def draw(w, n) -> np.ndarray:
    """(uint64(w) n) >> 32 for uint32 words w and 0 <= n < 2^32: in [0, n), 0 for n = 0."""
    return ((np.asarray(w, dtype=np.uint64) * np.asarray(n, dtype=np.uint64)) >> _S32).astype(np.int64)


def _words(seed: int, rows: np.ndarray, q: int) -> np.ndarray:
    return _rng.philox(_rng.counters(q, rows, STREAM_SPEC), _rng.key_of(seed))


def params(seed, first_row, B, K, T, lengths=None, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0,
           time_warp=0) -> dict:
    """The draws of clips 0 .. B - 1 as int64 arrays: lengths [B]; c, w [B] (the warp's centre and its new place, -1 where a
    clip is not warped); f, f0 [B, freq_masks] (rows [f0, f0 + f)); t, t0 [B, time_masks] (frames [t0, t0 + t))."""
    who = "spec_augment"
    check_shape(B, K, T, who)
    nf, F, nt, Wt, p, W = check_args(K, T, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, who)
    seed = _rng.check_seed(seed)
    first_row = _rng.check_rows(first_row, B)
    Tb = check_lengths(lengths, B, T, who)
    rows = first_row + np.arange(B, dtype=np.uint64)
    c = np.full(B, -1, dtype=np.int64)
    wp = np.full(B, -1, dtype=np.int64)
    on = (Tb > 2 * W) if W > 0 else np.zeros(B, dtype=bool)
    if on.any():
        w = _words(seed, rows[on], Q_WARP)
        c[on] = W + draw(w[:, 0], Tb[on] - 2 * W)
        wp[on] = c[on] - W + 1 + draw(w[:, 1], 2 * W)
    f, f0 = np.zeros((B, nf), dtype=np.int64), np.zeros((B, nf), dtype=np.int64)
    for i in range(nf):
        w = _words(seed, rows, Q_FREQ + i)
        f[:, i] = draw(w[:, 0], F + 1)
        f0[:, i] = draw(w[:, 1], K - f[:, i] + 1)
    We = np.minimum(Wt, np.floor(p * Tb.astype(np.float64)).astype(np.int64))
    t, t0 = np.zeros((B, nt), dtype=np.int64), np.zeros((B, nt), dtype=np.int64)
    for j in range(nt):
        w = _words(seed, rows, Q_TIME + j)
        t[:, j] = draw(w[:, 0], We + 1)
        t0[:, j] = draw(w[:, 1], Tb - t[:, j] + 1)
    return {"lengths": Tb, "c": c, "w": wp, "f": f, "f0": f0, "t": t, "t0": t0}
