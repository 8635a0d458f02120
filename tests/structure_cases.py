"""The cases of tests/test_gpu_structure.py, and what tests/test_structure_ref.py proves about them on the CPU (the Ward
cases' merge-cost gaps).  Inputs are made once per process and never changed."""
import functools

import numpy as np

from tests import structure_ref as ref

GATE = 1e-5                                        # |out - ref64| <= GATE max|R|: the standing float32 gate
SHEAR_T = (1, 2, 3, 63, 64, 65, 257)
ALL_MODES = ref.MODES
PATH_SIZES = ((1, 1), (2, 2), (17, 5), (64, 64), (65, 127), (257, 257))

# (n, (T, T'), mode, n_filters, zero_mean, clip): every mode at every size under the even 8 x 8 arrays of n = 7; n = 3 and
# the 39 x 39 arrays of n = 31 (wider than a tile's rows) at every size; one filter; zero_mean; no clip
PATH_CASES = ([(7, s, m, 7, False, True) for s in PATH_SIZES for m in ALL_MODES]
              + [(n, s, "reflect", 7, False, True) for n in (3, 31) for s in PATH_SIZES]
              + [(n, s, m, 1, False, True) for n in (3, 31) for s in ((2, 2), (65, 127)) for m in ("mirror", "constant")]
              + [(n, s, m, 7, True, c) for n in (3, 7, 31) for s in ((1, 1), (17, 5), (65, 127)) for m in ("reflect", "wrap")
                 for c in (True, False)]
              + [(n, (64, 64), "nearest", 7, False, False) for n in (3, 7, 31)])
PATH_CVAL = 0.25


def path_id(c):
    n, (T, Tc), mode, nf, zm, clip = c
    return f"n{n}-{T}x{Tc}-{mode}-f{nf}{'-zm' if zm else ''}{'' if clip else '-noclip'}"


@functools.lru_cache(maxsize=None)
def path_matrix(T, Tc, B=1):
    """[B, T, T'] float32 with entries of both signs."""
    rng = np.random.default_rng(1000 * T + Tc)
    R = rng.standard_normal((B, T, Tc)).astype(np.float32)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def path_reference(case):
    n, (T, Tc), mode, nf, zm, clip = case
    return ref.path_enhance(path_matrix(T, Tc)[0], n, n_filters=nf, zero_mean=zm, clip=clip, mode=mode, cval=PATH_CVAL)


MEDIAN_W = (1, 3, 7, 31, 63)
MEDIAN_T = (1, 2, 7, 64, 65, 130)
MEDIAN_MODES = ("reflect", "mirror", "nearest", "wrap", "constant")
MEDIAN_CVAL = -0.5


@functools.lru_cache(maxsize=None)
def median_matrix(t):
    """[t, t] float32: few distinct values (ties), negatives, both zeros and a block of zeros."""
    rng = np.random.default_rng(77 + t)
    R = rng.choice(np.array([-2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0], dtype=np.float32), size=(t, t))
    R = np.where(rng.random((t, t)) < 0.3, rng.standard_normal((t, t)).astype(np.float32), R).astype(np.float32)
    R[t // 4:t // 2, t // 3:(2 * t) // 3] = 0.0
    R.setflags(write=False)
    return R


# (T, D, k) as the issue lists them, then the span at the served cap (agg_t_max of structure_constants)
WARD_CASES = ((1, 3, 1), (2, 3, 1), (2, 3, 2), (5, 1, 2), (64, 12, 5), (257, 20, 8), (300, 1, 300), (1025, 7, 1))
WARD_CAP = (8192, 12, 6)
WARD_RAGGED = ((0, 40, 3), (1, 1, 1), (1, 64, 64), (2, 65, 7), (3, 17, 2))       # (clip, frames, k) of a [4, 65, 6] batch
WARD_GAP = 1e-9

# piecewise constant with integer steps: every cost is exact.  The zero-cost merges go first; then (0, 1) ties with (1, 2) and
# (20, 21) with (21, 22) at cost 1/2 and the leftmost goes: [0 1] [2] [10 10 10] [20 21] [22]
WARD_CRAFTED = (np.array([0, 1, 2, 10, 10, 10, 20, 21, 22], dtype=np.float32)[:, None], 5, np.array([0, 2, 3, 6, 8]))


@functools.lru_cache(maxsize=None)
def ward_frames(T, D, seed=0):
    X = np.random.default_rng(31 * T + D + seed).standard_normal((T, D)).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def ward_reference(T, D, k):
    return ref.chain_ward(ward_frames(T, D), k)


@functools.lru_cache(maxsize=None)
def ward_ragged_batch():
    X = np.random.default_rng(5).standard_normal((4, 65, 6)).astype(np.float32)
    X.setflags(write=False)
    return X


SYNC_EDGES = np.array([0, 1, 3, 67, 132, 133, 140])          # segments of 1, 2, 64, 65, 1 and 7 frames
SYNC_D = (1, 63, 65)
SUBSEGMENT_FRAMES = np.array([90, 30, 30, 7, 500, 64, 65])   # unsorted, repeated, past T = 140
