"""Case tables and input builders of tests/test_gpu_hpss_params.py (numpy only: importable without a device).  Everything is
seeded; tests/test_hpss_cases.py holds each table to its purpose with the float64 restatement (tests/hpss_ref.py) alone."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

NB = 1025

# (win_harm, win_perc): every size class of the runtime network (<= 8 / 16 / 32 / 64 inputs) at its upper edge and one past
# it, even windows (rank k / 2, not (k - 1) / 2), and 31 on one axis only (the <0, 0> instantiation, not <31, 31>)
MEDIAN_WINDOWS = ((2, 2), (3, 2), (16, 33), (33, 16), (63, 32), (31, 17), (7, 31), (62, 15))
# frames: one; far fewer than a large window (folds many times); a full tile of 16; one frame into the second and the third
# tile; several tiles
MEDIAN_T = (1, 3, 16, 17, 33, 40)
EDGE_T = 33
EDGE_WINDOWS = ((31, 31), (16, 33), (63, 32))

SOFTMASK_WINDOWS = (7, 31)
SOFTMASK_POWERS = (0.5, 1.5, 3.0, 10.0, 1.0, 2.0, np.inf)
SOFTMASK_MARGINS = ((1.0, 1.0), (2.5, 1.0), (1.0, 3.0), (2.0, 3.0))

# output lengths at which the inverse STFT's segment count steps (1 -> 2 and 2 -> 3)
ISTFT_SEAMS = (8192, 8193, 16384, 16385)
ISTFT_SEG = 16                                  # output hops per wave (SEG of csrc/hpss.hip)


def istft_segments(L: int) -> int:
    """Waves per clip and component of syg_istft2048_f32 at output length L (its rule, restated)."""
    hlast = (L - 1 + 1024) // 512
    return -(-(hlast - 1) // ISTFT_SEG)


class HnrCase(NamedTuple):
    fl: int
    hop: int
    center: int
    L: int
    B: int
    pad: int                                    # row stride ld = L + pad

    @property
    def ld(self):
        return self.L + self.pad

    @property
    def id(self):
        return f"fl{self.fl}-hop{self.hop}-c{self.center}-L{self.L}-B{self.B}" + (f"-ld{self.ld}" if self.pad else "")


HNR_CASES = (
    HnrCase(2048, 512, 1, 22050, 3, 0),
    HnrCase(1, 1, 1, 70, 2, 0),
    HnrCase(63, 7, 0, 1000, 5, 0),
    HnrCase(65, 64, 1, 640, 2, 0),              # odd frame, hop divides L: frames_padded is one below frames_expected
    HnrCase(1025, 256, 1, 1024, 1, 0),
    HnrCase(4096, 1024, 0, 4096, 2, 0),         # a single frame
    HnrCase(4096, 1024, 1, 100, 2, 0),          # the frame is longer than the clip
    HnrCase(1000, 250, 1, 3001, 9, 37),         # strided rows; B T is not a multiple of 4
)
HNR_CONSTANTS = (1.1e-5, 0.9e-5)                # interior-frame powers 1.21e-10 and 0.81e-10 about the 1e-10 threshold


def mag32(D):
    """|D| of D [..., 2] float32 exactly as the kernel states it: sqrt_rn(re * re + im * im), every step float32
    round-to-nearest (a denormal square stays denormal, an overflowing one is +inf)."""
    D = np.asarray(D)
    assert D.dtype == np.float32 and D.shape[-1] == 2
    with np.errstate(over="ignore", under="ignore"):
        re, im = D[..., 0], D[..., 1]
        return np.sqrt(re * re + im * im, dtype=np.float32)


def tie_spectrum(B: int, T: int, seed: int = 0):
    """D [B, T, 1025, 2] float32 whose magnitudes take nine values, {0, 3, 4, 5, 6, sqrt 52, 8, sqrt 73, 10} (three in ten
    cells are 0): every median window holds equal values and zeros next to non-zeros.  One block of exact zeros per clip,
    8 frames (all of them at T < 17) x at least 128 bins, gives H = P = 0 for the split-zeros rule; a clip of fewer than 4
    frames gets a wider block so that the batch still holds a thousand such cells."""
    rng = np.random.default_rng([seed, B, T])
    re = rng.choice(np.float32([0, 0, 0, 3, 6]), size=(B, T, NB))
    im = rng.choice(np.float32([0, 0, 4, 8]), size=(B, T, NB))
    D = np.stack([re, im], axis=-1).astype(np.float32)
    nt = 8 if T >= 17 else T
    nb = max(128, -(-512 // nt))
    for b in range(B):
        t0 = int(rng.integers(0, T - nt + 1))
        f0 = int(rng.integers(0, NB - nb + 1))
        D[b, t0:t0 + nt, f0:f0 + nb] = 0.0
    return D


EDGE_KINDS = ("tiny", "huge", "zero")


def edge_cells(T: int, seed: int = 0):
    """Where edge_spectrum puts its cells: kind -> (frames, bins).  Each kind gets a run of 40 bins in one frame and a run
    of 20 frames (all of them below that) in one bin, long enough to be the median of the windows of EDGE_WINDOWS, and a
    dozen single cells."""
    rng = np.random.default_rng([seed, T, 1])
    cells = {}
    for i, kind in enumerate(EDGE_KINDS):
        nt = min(20, T)
        tr, fr = int(rng.integers(0, T)), 100 + 300 * i + int(rng.integers(0, 100))          # the run along bins
        tc, fc = int(rng.integers(0, T - nt + 1)), 60 + 300 * i + int(rng.integers(0, 30))   # the run along frames
        t = np.concatenate([np.full(40, tr), tc + np.arange(nt), rng.integers(0, T, 12)])
        f = np.concatenate([fr + np.arange(40), np.full(nt, fc), rng.integers(0, NB, 12)])
        cells[kind] = (t.astype(np.int64), f.astype(np.int64))
    return cells


def edge_spectrum(T: int, seed: int = 0):
    """Noise-like D [1, T, 1025, 2] float32 with a few dozen cells of three kinds written in (edge_cells): `tiny`, |re| and
    |im| in [1e-21, 1e-19] (the squares are denormal, the magnitude is normal); `huge`, |re| = 3e19 (the square overflows:
    the magnitude is +inf); `zero`, exact zeros."""
    rng = np.random.default_rng([seed, T, 2])
    D = rng.standard_normal((1, T, NB, 2)).astype(np.float32)
    cells = edge_cells(T, seed)
    for kind in EDGE_KINDS:
        t, f = cells[kind]
        n = t.size
        sign = rng.choice(np.float32([-1, 1]), size=(n, 2))
        if kind == "tiny":
            v = (10.0 ** rng.uniform(-21, -19, size=(n, 2))).astype(np.float32) * sign
        elif kind == "huge":
            v = np.stack([np.full(n, 3e19), rng.standard_normal(n)], axis=-1).astype(np.float32) * sign
        else:
            v = np.zeros((n, 2), dtype=np.float32)
        D[0, t, f] = v
    return D


def noise_spectrum(B: int, T: int, seed: int = 0):
    """Random complex D [B, T, 1025, 2] float32, every part standard normal: Im D[..., 0] and Im D[..., 1024], which no
    forward transform of a real signal produces, are of order 1."""
    return np.random.default_rng([seed, B, T, 3]).standard_normal((B, T, NB, 2)).astype(np.float32)


def unit_masks(B: int, T: int, seed: int = 0):
    """Two random masks [B, T, 1025] float32 in [0, 1]."""
    rng = np.random.default_rng([seed, B, T, 4])
    return rng.random((B, T, NB), dtype=np.float32), rng.random((B, T, NB), dtype=np.float32)


def to_complex(D):
    """D [..., T, 1025, 2] float32 -> complex128 [..., 1025, T], the layout of hpss_ref.istft."""
    D = np.asarray(D, dtype=np.float64)
    return np.swapaxes(D[..., 0] + 1j * D[..., 1], -1, -2)


def hnr_rows_input(c: HnrCase, seed: int = 0):
    """(yh, yp) float32 [B, L] of an HNR case, by row index mod 5: two noises; noise over silence (+80); silence over
    noise (-80); both silent (NaN); the constants HNR_CONSTANTS, either side of the power threshold."""
    rng = np.random.default_rng([seed, c.fl, c.hop, c.L, c.B])
    yh = np.zeros((c.B, c.L), dtype=np.float32)
    yp = np.zeros((c.B, c.L), dtype=np.float32)
    for r in range(c.B):
        k = r % 5
        if k in (0, 1):
            yh[r] = rng.standard_normal(c.L) * 0.3
        if k in (0, 2):
            yp[r] = rng.standard_normal(c.L) * 0.1
        if k == 4:
            yh[r], yp[r] = HNR_CONSTANTS
    return yh, yp
