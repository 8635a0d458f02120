"""The float64 restatement of librosa.sequence.dtw (tests/dtw_ref.py) is pinned by construction: the vectorised form
equals the literal loops bit for bit, the loops equal brute force over every monotone path, the costs equal SciPy's
cdist, and the known answers (identical sequences, doubled frames) come out."""
import itertools

import numpy as np
import pytest

from tests import dtw_ref as R

WEIGHTS = [(None, None), ((1.5, 0.75, 2.0), (0.0, 0.25, 0.5)), ((1.0, 1.0, 1.0), (0.0, 1.0, 1.0))]


def _cost(rng, N, M, ties):
    if ties:
        return rng.integers(0, 4, size=(N, M)).astype(np.float32)
    return rng.random((N, M)).astype(np.float32)


def test_diag_equals_loops_bit_for_bit():
    rng = np.random.default_rng(1)
    shapes = [(n, n) for n in range(1, 41)] + [(1, 17), (17, 1), (3, 40), (40, 3), (23, 37), (37, 23), (2, 2), (5, 31)]
    for i, (N, M) in enumerate(shapes):
        C = _cost(rng, N, M, ties=i % 2 == 0)
        for subseq in (False, True):
            wm, wa = WEIGHTS[i % 3]
            D1, S1 = R.dtw_loops(C, wm, wa, subseq)
            D2, S2 = R.dtw_diag(C, wm, wa, subseq)
            assert np.array_equal(D1, D2) and np.array_equal(S1, S2), (N, M, subseq)


def _all_paths(N, M):
    """every monotone path from (0, 0) to (N - 1, M - 1) over the three steps"""
    def rec(n, m):
        if (n, m) == (N - 1, M - 1):
            yield [(n, m)]
            return
        for dn, dm in ((1, 1), (0, 1), (1, 0)):
            if n + dn < N and m + dm < M:
                for rest in rec(n + dn, m + dm):
                    yield [(n, m)] + rest
    return rec(0, 0)


def test_loops_equal_brute_force_up_to_5x5():
    rng = np.random.default_rng(2)
    for N, M in itertools.product(range(1, 6), repeat=2):
        C = rng.integers(0, 8, size=(N, M)).astype(np.float32)          # integers: every path sum is exact
        for wm, wa in WEIGHTS[:2]:
            wm_, wa_ = R._weights(wm, wa)
            D, steps, wp, _ = R.dtw(C, wm, wa, loops=True)
            best = min(R.path_cost(C.astype(np.float64), p[::-1], wm_, wa_) for p in _all_paths(N, M))
            assert D[-1, -1] == best, (N, M)
            R.check_path(wp, N, M)
            assert R.path_cost(C.astype(np.float64), wp, wm_, wa_) == best


def test_subseq_brute_force():
    rng = np.random.default_rng(3)
    for N, M in ((1, 4), (2, 5), (3, 5), (4, 4)):
        C = rng.integers(0, 8, size=(N, M)).astype(np.float32)
        D, steps, wp, start = R.dtw(C, subseq=True, loops=True)
        best = np.inf
        for m0 in range(M):                                              # free start column: the sub-matrix from m0 on
            for m1 in range(m0, M):
                sub = C[:, m0:m1 + 1].astype(np.float64)
                best = min(best, min(R.path_cost(sub, p[::-1]) for p in _all_paths(N, m1 - m0 + 1)))
        assert D[-1, start] == best == D[-1].min()
        assert start == int(np.argmin(D[-1]))
        R.check_path(wp, N, M, subseq=True, start=start)


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cityblock"])
def test_identical_sequences_cost_zero_on_the_diagonal(metric):
    X = np.random.default_rng(4).standard_normal((5, 23))
    D, steps, wp, _ = R.dtw(R.cost_matrix(X, X, metric))
    assert D[-1, -1] == 0.0
    assert np.array_equal(wp[::-1], np.stack([np.arange(23)] * 2, axis=1))


def test_doubled_frames_cost_zero_and_follow_the_tie_rule():
    X = np.random.default_rng(5).standard_normal((3, 9))
    Y = np.repeat(X, 2, axis=1)
    D, steps, wp, _ = R.dtw(R.cost_matrix(X, Y, "sqeuclidean"))
    assert D[-1, -1] == 0.0
    R.check_path(wp, 9, 18)
    # frame n of X matches frames 2 n and 2 n + 1 of Y at cost 0; into (n, 2 n) the diagonal from (n - 1, 2 n - 1) is the
    # only free step, into (n, 2 n + 1) only the step to the left is: the path is forced
    want = [(n, m) for n in range(9) for m in (2 * n, 2 * n + 1)]
    assert [tuple(p) for p in wp[::-1]] == want


def test_costs_equal_cdist():
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(6)
    X, Y = rng.standard_normal((13, 31)), rng.standard_normal((13, 17))
    for metric in ("euclidean", "sqeuclidean", "cityblock", "cosine"):
        ref = cdist(X.T, Y.T, metric=metric)
        got = R.cost_matrix(X, Y, metric)
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref)), metric
    assert R.cost_matrix(np.arange(4.0), np.arange(3.0), "cityblock").shape == (4, 3)       # (N,) inputs: K = 1


def test_paths_are_always_valid():
    rng = np.random.default_rng(7)
    for N, M in ((1, 1), (1, 9), (9, 1), (7, 12), (12, 7), (20, 20)):
        for subseq in (False, True):
            C = _cost(rng, N, M, ties=True)
            D, steps, wp, start = R.dtw(C, subseq=subseq)
            R.check_path(wp, N, M, subseq=subseq, start=start)
            assert np.isclose(R.path_cost(C.astype(np.float64), wp), D[-1, start])
