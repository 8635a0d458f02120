"""Host side of the device noise generator (sygnals_amd/csrc/rng_dev.h): Philox4x32-10 in exact integer NumPy, the stream
layout, seed checks and the per-row draws.  Pure host logic: no torch, no library.

A value depends on (seed, stream, row, n) alone: key = (seed & 0xffffffff, seed >> 32); counter = (q & 0xffffffff,
q >> 32, row, stream) with q = n // 4.  Stream STREAM_NOISE carries the noise samples (generated on the device), stream
STREAM_ROW the per-row draws, which are taken here: B numbers are cheap.  tests/rng_ref.py is the independent
restatement; tests/test_cabi_noise.py holds the stream ids to the library's (syg_rng_constants)."""
from __future__ import annotations

import secrets

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers (Random123)
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments
ROUNDS = 10
STREAM_NOISE, STREAM_ROW = 0, 1
ROW_LIMIT = 1 << 31
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def check_seed(seed) -> int:
    """An integer seed in [0, 2^64) as an int; None draws a fresh one (fresh_seed)."""
    if seed is None:
        return fresh_seed()
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed must be an integer in [0, 2^64) or None (got {seed!r})")
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"seed must be an integer in [0, 2^64) or None (got {seed})")
    return seed


def fresh_seed() -> int:
    """A 64-bit seed from the operating system's entropy."""
    return secrets.randbits(64)


def check_rows(first_row, B) -> int:
    if isinstance(first_row, (bool, np.bool_)) or not isinstance(first_row, (int, np.integer)):
        raise ValueError(f"first_row must be an integer (got {first_row!r})")
    first_row = int(first_row)
    if first_row < 0 or B < 1 or first_row + B > ROW_LIMIT:
        raise ValueError(f"rows first_row .. first_row + B - 1 must lie in [0, 2^31) (got first_row = {first_row}, B = {B})")
    return first_row


def key_of(seed: int) -> np.ndarray:
    seed = check_seed(seed)
    return np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)


def philox(counter, key) -> np.ndarray:
    """counter [n, 4], key [n, 2] (or one key [2]) uint32 -> [n, 4] uint32: ten rounds, the key bumped between rounds."""
    c = np.array(counter, dtype=np.uint64).reshape(-1, 4)
    k = np.broadcast_to(np.array(key, dtype=np.uint64).reshape(-1, 2), (c.shape[0], 2))
    c0, c1, c2, c3 = (c[:, j].copy() for j in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    for _ in range(ROUNDS):
        p0 = np.uint64(M0) * c0                       # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0 = (k0 + np.uint64(W0)) & _MASK
        k1 = (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def counters(q, row, stream) -> np.ndarray:
    """[n, 4] uint32 counters of calls q (an array or a number, < 2^64) of rows `row` in `stream`."""
    q, row = np.broadcast_arrays(np.asarray(q, dtype=np.uint64), np.asarray(row, dtype=np.uint64))
    q, row = q.reshape(-1), row.reshape(-1)
    return np.stack([q & _MASK, q >> _S32, row, np.full_like(q, stream)], axis=1).astype(np.uint32)


def row_words(seed: int, first_row: int, B: int) -> np.ndarray:
    """[B, 4] uint32: the words of counter (0, 0, first_row + r, STREAM_ROW), the per-row draws."""
    first_row = check_rows(first_row, B)
    return philox(counters(0, first_row + np.arange(B, dtype=np.uint64), STREAM_ROW), key_of(seed))


def uniform_rows(seed: int, first_row: int, B: int, lo: float, hi: float) -> np.ndarray:
    """One float64 per row: lo + (hi - lo) (w0 + 0.5) 2^-32 with w0 the row's first word."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"a range (lo, hi) must be finite with lo <= hi (got ({lo}, {hi}))")
    w0 = row_words(seed, first_row, B)[:, 0].astype(np.float64)
    return lo + (hi - lo) * ((w0 + 0.5) * 2.0 ** -32)
