"""Host plan of syg_resample_poly_f32 (csrc/resample.hip; include/sygnals_hip.h states the table's layout): the arithmetic of
scipy.signal.resample_poly turned into the index form  t = (n + n_pre_remove) down, p = t mod up, q = t div up,
y[n] = sum_j table[p][j] x~[q - j].  Pure NumPy / SciPy, float64 throughout, the float32 table rounded once.  No device and
no library here, so the plan is tested on the CPU."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from math import gcd

import numpy as np
from scipy.signal import firwin

DEFAULT_WINDOW = ("kaiser", 5.0)
# scipy's names -> pad code of the C ABI; the statistic ones run as 'constant' with 0 on the row minus its statistic
PAD_CODES = {"constant": 0, "edge": 1, "wrap": 2, "symmetric": 3, "reflect": 4}
STAT_PADS = ("mean", "minimum", "maximum")
SERVED_PADS = tuple(PAD_CODES) + STAT_PADS
REFUSED_PADS = ("median", "line", "smooth", "antisymmetric", "antireflect")


@dataclass(frozen=True)
class ResamplePlan:
    up: int               # reduced
    down: int             # reduced
    L: int
    n_out: int            # ceil(L up / down)
    n_pre_remove: int
    Kp: int               # taps per phase
    table: np.ndarray     # [up, Kp] float32, table[p][j] = hp[p + j up]; None where up == down == 1
    table64: np.ndarray   # the same before rounding


def reduce_ratio(up, down):
    if int(up) != up or int(down) != down or up < 1 or down < 1:
        raise ValueError(f"up and down must be integers >= 1, got up={up}, down={down}")
    up, down = int(up), int(down)
    g = gcd(up, down)
    return up // g, down // g


def ratio_of_rates(orig_sr, target_sr):
    """(up, down) = target_sr / orig_sr reduced; the rates must be positive and integer-valued."""
    for name, v in (("orig_sr", orig_sr), ("target_sr", target_sr)):
        try:
            ok = float(v) > 0 and float(v) == int(v)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"{name} must be a positive integer-valued rate, got {v!r} (arbitrary ratios are not served)")
    return reduce_ratio(int(target_sr), int(orig_sr))


def check_padtype(padtype, L=None):
    if padtype in REFUSED_PADS or padtype not in SERVED_PADS:
        raise ValueError(f"padtype={padtype!r} is not served; served: {', '.join(SERVED_PADS)}")
    if padtype == "reflect" and L is not None and L < 2:
        raise ValueError("padtype='reflect' needs at least two samples (scipy itself fails on a one-sample row)")


def window_key(window):
    """Hashable form of `window`: a 1-D array of taps becomes ('taps', bytes); anything else is firwin's window spec."""
    if isinstance(window, (np.ndarray, list)):
        a = np.asarray(window, dtype=np.float64)
        if a.ndim != 1 or a.size < 1:
            raise ValueError("window must be a window specification or a 1-D array of filter taps")
        return ("taps", a.tobytes())
    return tuple(window) if isinstance(window, (tuple, list)) else window


@functools.lru_cache(maxsize=32)
def _filter(up: int, down: int, wkey):
    """(up-scaled h in float64, half_len): independent of the row length."""
    if isinstance(wkey, tuple) and wkey and wkey[0] == "taps":
        h = np.frombuffer(wkey[1], dtype=np.float64).copy()
        half_len = (h.size - 1) // 2
    else:
        max_rate = max(up, down)
        half_len = 10 * max_rate
        h = firwin(2 * half_len + 1, 1.0 / max_rate, window=wkey)
    return h * up, half_len


def table_bytes(up: int, down: int, window=DEFAULT_WINDOW) -> int:
    """A lower bound of the table's size that needs no filter design (n_post_pad adds at most one tap per phase)."""
    up, down = reduce_ratio(up, down)
    wkey = window_key(window)
    n = len(wkey[1]) // 8 if isinstance(wkey, tuple) and wkey and wkey[0] == "taps" else 20 * max(up, down) + 1
    return 4 * up * (-(-(n + 1) // up))


@functools.lru_cache(maxsize=64)
def _plan(up: int, down: int, wkey, L: int) -> ResamplePlan:
    n_out = -(-(L * up) // down)
    h, half_len = _filter(up, down, wkey)
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    # upfirdn gives ((L - 1) up + len(hp) - 1) // down + 1 outputs; the least len(hp) that reaches n_out + n_pre_remove
    need = (n_out + n_pre_remove - 1) * down - (L - 1) * up + 1
    n_post_pad = max(0, need - (h.size + n_pre_pad))
    hp = np.concatenate([np.zeros(n_pre_pad), h, np.zeros(n_post_pad)])
    Kp = -(-hp.size // up)
    tab = np.zeros(up * Kp)
    tab[:hp.size] = hp
    tab = np.ascontiguousarray(tab.reshape(Kp, up).T)
    return ResamplePlan(up, down, L, n_out, n_pre_remove, Kp, tab.astype(np.float32), tab)


def resample_plan(up, down, L, window=DEFAULT_WINDOW) -> ResamplePlan:
    """The plan of a row of L samples at up / down (reduced here), cached per (up, down, window, L); the filter design,
    which does not depend on L, is cached on its own."""
    up, down = reduce_ratio(up, down)
    if int(L) != L or L < 1:
        raise ValueError(f"L must be a positive integer, got {L}")
    if up == 1 and down == 1:
        return ResamplePlan(1, 1, int(L), int(L), 0, 0, None, None)
    return _plan(up, down, window_key(window), int(L))
