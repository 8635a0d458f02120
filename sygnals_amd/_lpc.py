"""Host side of linear prediction (csrc/lpc.hip; the float64 restatement is tests/lpc_ref.py): the bounds, the argument
rules and their messages.  No device work."""
from __future__ import annotations

import math

MAX_FRAME = 2048            # longest frame of the frame kernel (syg_lpc_constants: max_frame)
MAX_ORDER = 64              # highest order (max_order)
MAX_ROW = 1 << 26           # the longest whole row
MAX_ELEMS = 1 << 31         # elements of one result at most
METHODS = {"burg": 0, "autocorr": 1}          # SYG_LPC_* of include/sygnals_hip.h
FORMS = (None, "frame", "stage")
AMIN = 1e-10                # floor of the envelope in dB (the power floor of the dB code)


def check_method(method) -> int:
    if method not in METHODS:
        raise ValueError(f"method={method!r} is not served: 'burg' (librosa.lpc's) and 'autocorr' (Levinson-Durbin) are")
    return METHODS[method]


def default_window(method: str, window):
    """Burg takes no window unless one is given; the autocorrelation method defaults to hann."""
    if window is None and method == "autocorr":
        return "hann"
    return window


def _int(v, name: str) -> int:
    try:
        ok = not isinstance(v, bool) and int(v) == v
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def order_bound(N: int) -> int:
    return min(MAX_ORDER, N - 2)


def check_order(order, N: int) -> int:
    """1 <= order <= min(64, N - 2) for frames or rows of N samples."""
    p = _int(order, "order")
    hi = order_bound(N)
    if not 1 <= p <= hi:
        raise ValueError(f"order={p} is outside 1 ... min({MAX_ORDER}, N - 2) = {hi} for N = {N} samples "
                         f"(orders above {MAX_ORDER} are not served)")
    return p


def check_frame(frame_length, hop) -> tuple:
    N, h = _int(frame_length, "frame_length"), _int(hop, "hop_length")
    if N > MAX_FRAME:
        raise ValueError(f"frame_length={N} is above {MAX_FRAME}, the longest frame of the frame form; whole rows of any length "
                         "take lpc_rows (the stage form)")
    if N < 3:
        raise ValueError(f"frame_length={N} is below 3, the shortest frame (order 1 needs order + 2 samples)")
    if h < 1:
        raise ValueError(f"hop_length must be at least 1, got {h}")
    return N, h


def check_row(L: int) -> int:
    if L > MAX_ROW:
        raise ValueError(f"rows of {L} samples are above the longest row, 2^26")
    return int(L)


def check_size(what: str, dims, names) -> None:
    total = 1
    for d in dims:
        total *= int(d)
    if total > MAX_ELEMS:
        shape = " x ".join(f"{int(d)} {n}" for d, n in zip(dims, names))
        raise ValueError(f"{what}: the result of {shape} has {total} elements, above the bound of 2^31; take fewer rows a call")


def check_n_fft(n_fft) -> int:
    n = _int(n_fft, "n_fft")
    if n < 2 or n % 2 or n > 1 << 24:
        raise ValueError(f"n_fft={n} must be even and in [2, 2^24]")
    return n


def check_amin(amin) -> float:
    a = float(amin)
    if not math.isfinite(a) or a < 0.0:
        raise ValueError(f"amin must be finite and >= 0, got {amin}")
    return a
