"""Host side of the Viterbi decoders (ops.viterbi, core/sequence.py): librosa.sequence's transition builders, the argument
checks and the float64 log tables.  NumPy only, no device.

The decoders' definition is tests/sequence_ref.py (a float64 restatement of librosa 0.10's _viterbi and its three
callers).  The logs of the transition, initial and marginal probabilities are taken here, in float64, with
eps = the smallest normal number of the probabilities' dtype, as librosa does; only log(prob + eps) of the emissions is
taken on the device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

SERVED = "served: 1 <= S <= 1024 states, prob in [0, 1], a square row-stochastic transition matrix [S, S] or one per clip"


def tiny(dtype) -> float:
    """eps of the decoders: the smallest normal number of the probabilities' dtype (FLT_MIN / DBL_MIN)."""
    dt = np.dtype(dtype)
    return float(np.finfo(dt if dt.kind == "f" else np.float64).tiny)


def _window(window, width: int) -> np.ndarray:
    try:
        from scipy.signal import get_window
    except ImportError:                                  # SciPy's triang(width, sym=True), the default window
        if window != "triangle":
            raise ValueError(f"transition_local: window={window!r} needs SciPy; without it only 'triangle' is served")
        n = np.arange(1, (width + 1) // 2 + 1, dtype=np.float64)
        if width % 2 == 0:
            w = (2 * n - 1.0) / width
            return np.concatenate([w, w[::-1]])
        w = 2 * n / (width + 1.0)
        return np.concatenate([w, w[-2::-1]])
    return np.asarray(get_window(window, width, fftbins=False), dtype=np.float64)


def _n_states(who: str, n) -> int:
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"{who}: n_states={n!r} must be a positive integer")
    return int(n)


def _per_state(who: str, name: str, v, n: int) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError(f"{who}: {name} must be a scalar or hold one value per state ([{n}]), got shape {a.shape}")
    return a


def transition_uniform(n_states: int) -> np.ndarray:
    """librosa.sequence.transition_uniform: every entry 1 / n_states."""
    n = _n_states("transition_uniform", n_states)
    return np.full((n, n), 1.0 / n)


def transition_loop(n_states: int, prob) -> np.ndarray:
    """librosa.sequence.transition_loop: prob_i on the diagonal, (1 - prob_i) / (n - 1) elsewhere in row i.  n_states = 1
    is refused, as librosa refuses it (its rule divides by n - 1)."""
    n = _n_states("transition_loop", n_states)
    if n <= 1:
        raise ValueError("transition_loop: n_states must be greater than 1 (the off-diagonal share is (1 - prob) / (n - 1))")
    p = _per_state("transition_loop", "prob", prob, n)
    if not (np.all(p >= 0) and np.all(p <= 1)):
        raise ValueError(f"transition_loop: prob={prob!r} must lie in [0, 1]")
    t = np.empty((n, n))
    for i in range(n):
        t[i] = (1.0 - p[i]) / (n - 1)
        t[i, i] = p[i]
    return t


def transition_cycle(n_states: int, prob) -> np.ndarray:
    """librosa.sequence.transition_cycle: prob_i on the diagonal, 1 - prob_i at column (i + 1) mod n."""
    n = _n_states("transition_cycle", n_states)
    if n <= 1:
        raise ValueError("transition_cycle: n_states must be greater than 1")
    p = _per_state("transition_cycle", "prob", prob, n)
    if not (np.all(p >= 0) and np.all(p <= 1)):
        raise ValueError(f"transition_cycle: prob={prob!r} must lie in [0, 1]")
    t = np.zeros((n, n))
    for i in range(n):
        t[i, (i + 1) % n] = 1.0 - p[i]
        t[i, i] = p[i]
    return t


def transition_local(n_states: int, width, *, window="triangle", wrap: bool = False) -> np.ndarray:
    """librosa.sequence.transition_local as recalled (not checked against librosa): row i is the window of width_i samples
    (scipy.signal.get_window, fftbins=False), zero-padded centred to n_states, rolled by n_states // 2 + i + 1 so that it
    is centred on the diagonal, clipped to the band without `wrap`, and normalised to sum 1."""
    n = _n_states("transition_local", n_states)
    if n <= 1:
        raise ValueError("transition_local: n_states must be greater than 1")
    w = np.asarray(width)
    if w.ndim == 0:
        w = np.full(n, w)
    if w.shape != (n,) or w.dtype.kind not in "iu" or np.any(w < 1) or np.any(w > n):
        raise ValueError(f"transition_local: width={width!r} must be an integer in [1, {n}] or one per state")
    t = np.zeros((n, n))
    for i, wi in enumerate(int(v) for v in w):
        row = np.zeros(n)
        lpad = (n - wi) // 2
        row[lpad:lpad + wi] = _window(window, wi)
        row = np.roll(row, n // 2 + i + 1)
        if not wrap:
            row[min(n, i + wi // 2 + 1):] = 0
            row[:max(0, i - wi // 2)] = 0
        t[i] = row
    s = t.sum(axis=1, keepdims=True)
    if np.any(s <= 0):
        raise ValueError("transition_local: a row of the window is all zero")
    return t / s


# ------------------------------------------------------------------------------------------------------------------
# argument checks (ValueError, before any device work) and the log tables

def check_transition(who: str, transition, S: int, n_batch: Optional[int] = None, stochastic: bool = True) -> np.ndarray:
    """transition as float64 [S, S] or [n_batch, S, S]; stochastic: entries >= 0 and rows that sum to 1 (np.allclose)."""
    t = np.asarray(transition, dtype=np.float64)
    if t.ndim not in (2, 3) or t.shape[-1] != t.shape[-2]:
        raise ValueError(f"{who}: transition must be square, [S, S] or one per clip [B, S, S], got shape {t.shape} ({SERVED})")
    if t.shape[-1] != S:
        raise ValueError(f"{who}: transition is {t.shape[-2]} x {t.shape[-1]} but prob has S = {S} states ({SERVED})")
    if t.ndim == 3 and n_batch is not None and t.shape[0] != n_batch:
        raise ValueError(f"{who}: {t.shape[0]} transition matrices for {n_batch} clips ({SERVED})")
    if np.isnan(t).any():
        raise ValueError(f"{who}: transition holds NaN ({SERVED})")
    if stochastic:
        if np.any(t < 0):
            raise ValueError(f"{who}: transition holds negative entries ({SERVED})")
        if not np.allclose(t.sum(axis=-1), 1.0):
            raise ValueError(f"{who}: the rows of transition must sum to 1 ({SERVED})")
    return t


def check_distribution(who: str, name: str, p, S: int, n_batch: Optional[int] = None, stochastic: bool = True) -> np.ndarray:
    """p_init / p_state as float64 [S] or [n_batch, S]: not negative and summing to 1 (np.allclose)."""
    a = np.asarray(p, dtype=np.float64)
    if a.ndim not in (1, 2) or a.shape[-1] != S or (a.ndim == 2 and n_batch is not None and a.shape[0] != n_batch):
        raise ValueError(f"{who}: {name} must hold one value per state ([{S}], or one row per clip), got shape {a.shape}")
    if np.isnan(a).any():
        raise ValueError(f"{who}: {name} holds NaN")
    if stochastic and (np.any(a < 0) or not np.allclose(a.sum(axis=-1), 1.0)):
        raise ValueError(f"{who}: {name} must be a probability distribution: no negative entry, sum 1")
    return a


def check_binary_probability(who: str, name: str, p, n_labels: int) -> np.ndarray:
    """p_init / p_state of viterbi_binary: a scalar or one value per label, in [0, 1] -> float64 [n_labels]."""
    a = np.asarray(p, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n_labels, float(a))
    if a.shape != (n_labels,) or np.isnan(a).any() or np.any(a < 0) or np.any(a > 1):
        raise ValueError(f"{who}: {name} must be a scalar or one value per label ([{n_labels}]) in [0, 1]")
    return a


def check_prob(who: str, prob: np.ndarray, normalised: bool = False) -> None:
    """prob [..., S, T] on the host: inside [0, 1]; normalised: summing to 1 over the states at every frame."""
    if prob.ndim < 2 or prob.shape[-1] < 1 or prob.shape[-2] < 1:
        raise ValueError(f"{who}: prob must be [..., S, T] with at least one state and one frame, got shape {prob.shape}")
    if np.isnan(prob).any() or np.any(prob < 0) or np.any(prob > 1):
        raise ValueError(f"{who}: prob must lie in [0, 1] ({SERVED})")
    if normalised and not np.allclose(prob.sum(axis=-2), 1.0):
        raise ValueError(f"{who}: prob must sum to 1 over the states at every frame (each frame a distribution)")


def log_table(p: np.ndarray, eps: float) -> np.ndarray:
    """log(p + eps) in float64."""
    return np.log(np.asarray(p, dtype=np.float64) + eps)
