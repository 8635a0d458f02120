"""Clips and float64 references for tests/test_gpu_loudness.py, built once per (fs, C, L, B, seed) and shared.

A clip is white noise whose level steps every 0.3 to 0.9 s among -14, -26, -38, -52 and -96 dBFS, so that blocks fall on
both sides of the absolute gate (-70 LUFS) and of both relative gates.  (Digital silence is left to the edge tests: behind
a loud stretch the filters ring down through hundreds of dB, where a float32 LUFS value no longer resolves 1e-4 dB.)
Which blocks pass a gate is a comparison; the device takes it in float64 as the reference does, and a case is only kept if
every block of the reference lies at least MARGIN LU away from every threshold it is compared with
(tests/loudness_ref.gate_margin): then the device must select exactly the reference's sets.  A draw that does not meet
the margin is drawn again with the next seed."""
import functools

import numpy as np

from sygnals_amd import _loudness as LD
from tests import loudness_ref as R

MARGIN = 0.01                       # LU
LEVELS_DB = (-14.0, -26.0, -38.0, -52.0, -96.0)
DB_TOL = 1e-4                       # momentary, short-term, integrated, LRA, dBTP against the float64 restatement
POWER_TOL = 1e-5                    # segment powers, relative to the row's largest


def draw_clip(rng, fs, C, L):
    x = np.zeros((C, L), dtype=np.float32)
    n = 0
    while n < L:
        m = min(L - n, int(rng.uniform(0.3, 0.9) * fs))
        lev = LEVELS_DB[rng.integers(len(LEVELS_DB))] if n else LEVELS_DB[0]      # every clip opens loud
        g = 10.0 ** (lev / 20.0) * (1.0 + 0.2 * rng.uniform(-1, 1, size=(C, 1)))
        x[:, n:n + m] = (g * rng.standard_normal((C, m))).astype(np.float32)
        n += m
    return x


def clip_with_margin(seed, fs, C, L, weights=None):
    for s in range(seed, seed + 64):
        x = draw_clip(np.random.default_rng(s), fs, C, L)
        if R.gate_margin(x, fs, weights) >= MARGIN:
            return x
    raise AssertionError(f"no draw with a gate margin of {MARGIN} LU in 64 seeds (fs={fs}, C={C}, L={L})")


@functools.lru_cache(maxsize=None)
def case(fs, C, L, B, seed=0, weights=None):
    """(x [B, C, L] float32, ref): ref holds per clip seg [C, n_seg], M, S, I, LRA, TP; read-only, shared between tests."""
    w = None if weights is None else list(weights)
    x = np.stack([clip_with_margin(seed + 1000 * b, fs, C, L, w) for b in range(B)])
    ref = {"seg": [], "M": [], "S": [], "I": [], "LRA": [], "TP": []}
    for b in range(B):
        seg = R.segment_powers(x[b], fs)
        ref["seg"].append(seg)
        ref["M"].append(R.lufs(R.block_powers(seg, fs, LD.MOMENTARY, w)))
        ref["S"].append(R.lufs(R.block_powers(seg, fs, LD.SHORT_TERM, w)))
        ref["I"].append(R.integrated(x[b], fs, w))
        ref["LRA"].append(R.loudness_range(x[b], fs, w))
        ref["TP"].append(R.true_peak(x[b], fs))
    x.setflags(write=False)
    return x, {k: (np.array(v) if k != "seg" else np.stack(v)) for k, v in ref.items()}


def db_error(got, want):
    """Largest |got - want| over the finite entries, after asserting that -inf sits where the reference has it."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), "-inf entries differ from the reference's"
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))


def lengths(fs):
    """The row lengths at which the kernels take another path: around the first momentary block, around chunk boundaries
    (256 k +- 1) next to it, around the first short-term block."""
    s4, s30 = LD.segment_start(4, fs), LD.segment_start(30, fs)
    k = s4 // 256 + 1
    return [s4 - 1, s4, s4 + 1, 256 * k - 1, 256 * k + 1, s30 - 1, s30 + 1]
