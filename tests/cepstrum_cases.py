"""Inputs shared by tests/test_cepstrum_ref.py and tests/test_gpu_cepstrum.py: the clips of the cepstrogram cases and the
rows of the complex-cepstrum cases, float32, built once per size."""
import functools

import numpy as np

SIGNALS = ("noise", "tones", "echo", "train", "zero", "constant")
COMPLEX_ROWS = ("damped", "damped_shift7", "damped_shift_n8", "echo40", "reversed", "three_taps", "negative")


@functools.lru_cache(maxsize=None)
def clip(kind: str, L: int, seed: int = 0) -> np.ndarray:
    """One clip [L] float32 (read-only)."""
    rng = np.random.default_rng(1000 * len(kind) + 7 * L + seed)
    n = np.arange(L)
    if kind == "noise":
        x = rng.standard_normal(L)
    elif kind == "tones":                                   # two tones over noise 40 dB down
        x = np.sin(2 * np.pi * 0.0137 * n + 0.3) + 0.7 * np.sin(2 * np.pi * 0.0911 * n + 1.1) + 0.01 * rng.standard_normal(L)
    elif kind == "echo":                                    # noise plus its echo at 100 samples
        x = rng.standard_normal(L)
        x[100:] += 0.6 * x[:-100].copy() if L > 100 else 0.0
    elif kind == "train":                                   # impulse train of period 80
        x = np.zeros(L)
        x[::80] = 1.0
        x += 1e-3 * rng.standard_normal(L)
    elif kind == "zero":
        x = np.zeros(L)
    elif kind == "constant":
        x = np.full(L, 0.25)
    else:
        raise ValueError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def clips(B: int, L: int) -> np.ndarray:
    """[B, L]: the signals in turn, a fresh seed each round."""
    return np.stack([clip(SIGNALS[b % len(SIGNALS)], L, b // len(SIGNALS)) for b in range(B)])


@functools.lru_cache(maxsize=None)
def complex_row(kind: str, n: int) -> np.ndarray:
    k = np.arange(n, dtype=np.float64)
    damped = 0.9 ** k * np.cos(0.3 * k) + 0.5 * 0.8 ** k
    if kind == "damped":
        x = damped
    elif kind == "damped_shift7":
        x = np.concatenate([np.zeros(7), damped[:n - 7]])
    elif kind == "damped_shift_n8":
        x = np.concatenate([np.zeros(n // 8), damped[:n - n // 8]])
    elif kind == "echo40":
        x = 0.95 ** k
        x[40:] += 0.5 * 0.95 ** k[:n - 40]
    elif kind == "reversed":
        x = (0.9 ** k)[::-1].copy()
    elif kind == "three_taps":
        x = np.zeros(n)
        x[:3] = (0.4, 0.8, -0.5)
    elif kind == "negative":                                # needs the bin-0 rule
        x = -(0.9 ** k)
    else:
        raise ValueError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x
