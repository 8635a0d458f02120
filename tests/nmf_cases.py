"""The cases of the NMF tests: shapes, input kinds, starting factors and the float64 / float32 restatement results, each
computed once and shared (tests/test_nmf_ref.py asserts the conditions on the CPU, tests/test_gpu_nmf.py gates the device).

Shapes (T, F, K): the issue's, and the edges of the kernels' tiles -- 16 frames and 64-bin chunks in the A-step, 64 bins
and 32-frame chunks in the C-step, 64-index chunks in the per-clip sums, and the K at which a thread's output count
changes (4 | 5, 8 | 9, 16 | 17, 32 | 33, 64)."""
import functools
import zlib

import numpy as np

from tests import nmf_ref as R

ISSUE_SHAPES = [(1, 1, 1), (2, 3, 2), (5, 33, 3), (65, 129, 17), (300, 12, 4), (40, 1025, 8), (257, 1025, 64), (3, 2049, 5)]
EDGE_SHAPES = [(15, 63, 4), (16, 64, 16), (17, 65, 5), (31, 127, 9), (32, 128, 32), (33, 130, 33)]
SHAPES = ISSUE_SHAPES + EDGE_SHAPES
KINDS = ("lowrank", "squares", "sparse")
LOSSES = R.LOSSES
BIG = (257, 1025, 64)
GATE = 1e-5
# Multiplicative updates amplify rounding from iteration to iteration, by an amount that depends on the input.  A case is
# gated only where the float32 restatement itself stays within GATE / 3 of float64 (asserted for every case by
# tests/test_nmf_ref.py).  With the inputs below that holds at 10 iterations everywhere (worst 3.0e-6) and at 30
# iterations for every shape but these three, which are gated at one step, one half step and 10 iterations only
# (worst float32 floor at 30 iterations: 6.5e-6, 6.5e-6 and 4.4e-6; 3.0e-6 over the gated cases).  The input seed was chosen, among twelve, as one at
# which every shape of the issue keeps its condition at 30 iterations; the choice used the restatement alone.
TEN_ONLY = (BIG, (16, 64, 16), (32, 128, 32))
SALT = 5


def iters_of(shape):
    return (10,) if tuple(shape) in TEN_ONLY else (10, 30)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """(V [T, F], A0 [T, K], C0 [K, F]) float32, read-only."""
    T, F, K = shape
    g = _rng("nmf", shape, kind, SALT)
    if kind == "lowrank":
        V = np.abs(g.standard_normal((T, K))) @ np.abs(g.standard_normal((K, F))) + 0.05 * np.abs(g.standard_normal((T, F)))
    elif kind == "squares":
        V = g.standard_normal((T, F)) ** 2
    else:
        V = np.abs(g.standard_normal((T, F))) * (g.random((T, F)) < 0.3)          # 30 % of the entries are not zero
        if T > 1:
            V[T // 2, :] = 0.0                                                    # one all-zero frame
        if F > 1:
            V[:, F // 3] = 0.0                                                    # one all-zero bin
    V = V.astype(np.float32)
    A0, C0 = R.init_factors(V if V.any() else np.ones_like(V), K, g.standard_normal(K * F + T * K))
    for x in (V, A0, C0):
        x.setflags(write=False)
    return V, A0, C0


@functools.lru_cache(maxsize=None)
def reference(shape, kind, loss, n_iter, update_A=True, update_C=True, f32=False):
    """The restatement's (A, C) after n_iter iterations from inputs(shape, kind): float64, or the float32 floor."""
    V, A0, C0 = inputs(shape, kind)
    A, C = R.nmf(V, A0, C0, n_iter, loss, update_A, update_C, dtype=np.float32 if f32 else np.float64)
    A.setflags(write=False)
    C.setflags(write=False)
    return A, C


def floor(shape, kind, loss, n_iter):
    """Distance of the float32 restatement from float64, as a fraction of each factor's peak: the larger of the two."""
    A, C = reference(shape, kind, loss, n_iter)
    a, c = reference(shape, kind, loss, n_iter, f32=True)
    return max(R.rel_peak(a, A), R.rel_peak(c, C))


ITERATED = [(s, k, l, n) for s in SHAPES for k in KINDS for l in LOSSES for n in iters_of(s)]
