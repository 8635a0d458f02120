"""float64 restatement of librosa.sequence.dtw (0.10) for its default step set [[1,1],[0,1],[1,0]]: the contract of
syg_dtw_f32 and sygnals_amd.core.alignment.  librosa is not a dependency, so the restatement is pinned by construction:
(i) `dtw_loops` is librosa's triple loop, in its order and with its tie rule (a later step replaces an earlier one only
if strictly smaller), and its backtrack; (ii) `dtw_diag` is the same recurrence vectorised over anti-diagonals.
tests/test_dtw_ref.py holds (ii) to (i) bit for bit and (i) to brute force over every monotone path."""
import numpy as np

STEPS = np.array([[1, 1], [0, 1], [1, 0]])


def cost_matrix(X, Y, metric="euclidean"):
    """C[n, m] = metric(X[:, n], Y[:, m]) in float64 by direct differences; X (K, N), Y (K, M)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    if metric == "cosine":
        with np.errstate(invalid="ignore", divide="ignore"):
            return 1.0 - (X.T @ Y) / (np.linalg.norm(X, axis=0)[:, None] * np.linalg.norm(Y, axis=0)[None, :])
    d = X[:, :, None] - Y[:, None, :]
    if metric == "cityblock":
        return np.abs(d).sum(axis=0)
    s = (d * d).sum(axis=0)
    if metric == "sqeuclidean":
        return s
    if metric == "euclidean":
        return np.sqrt(s)
    raise ValueError(metric)


def _weights(weights_mul, weights_add):
    wm = np.ones(3) if weights_mul is None else np.asarray(weights_mul, dtype=np.float64)
    wa = np.zeros(3) if weights_add is None else np.asarray(weights_add, dtype=np.float64)
    return wm, wa


def backtrack(steps, subseq=False, start=None):
    """librosa's __dtw_backtracking: from the last row (column `start`, default the last) back to (0, 0), or to row 0
    under subseq; the path is returned end first."""
    n, m = steps.shape[0] - 1, (steps.shape[1] - 1 if start is None else int(start))
    wp = [(n, m)]
    while (subseq and n > 0) or (not subseq and (n, m) != (0, 0)):
        k = steps[n, m]
        n, m = n - STEPS[k][0], m - STEPS[k][1]
        if min(n, m) < 0:
            break
        wp.append((n, m))
    return np.asarray(wp, dtype=np.int64)


def dtw_loops(C, weights_mul=None, weights_add=None, subseq=False):
    """(i) the literal loops: D (N, M) float64, steps (N, M) int."""
    C = np.asarray(C)
    wm, wa = _weights(weights_mul, weights_add)
    N, M = C.shape
    D = np.full((N + 1, M + 1), np.inf)
    D[1, 1] = C[0, 0]
    if subseq:
        D[1, 1:] = C[0, :]
    steps = np.zeros((N + 1, M + 1), dtype=np.int32)
    for n in range(1, N + 1):
        for m in range(1, M + 1):
            for k in range(3):
                cur_D = D[n - STEPS[k][0], m - STEPS[k][1]]
                cur_C = wm[k] * np.float64(C[n - 1, m - 1])
                cur_C += wa[k]
                cur = cur_D + cur_C
                if cur < D[n, m]:
                    D[n, m] = cur
                    steps[n, m] = k
    return D[1:, 1:], steps[1:, 1:]


def dtw_diag(C, weights_mul=None, weights_add=None, subseq=False):
    """(ii) the same recurrence, one anti-diagonal at a time: the cells of one anti-diagonal depend only on the two
    before it, and each takes its candidates in the loops' order."""
    C = np.asarray(C)
    wm, wa = _weights(weights_mul, weights_add)
    N, M = C.shape
    C64 = C.astype(np.float64)
    D = np.full((N + 1, M + 1), np.inf)
    steps = np.zeros((N + 1, M + 1), dtype=np.int32)
    preset = np.full((N, M), np.inf)
    preset[0, 0] = C64[0, 0]
    if subseq:
        preset[0, :] = C64[0, :]
    for d in range(N + M - 1):
        n = np.arange(max(0, d - (M - 1)), min(N - 1, d) + 1)
        m = d - n
        c = C64[n, m]
        best = preset[n, m].copy()
        code = np.zeros(n.size, dtype=np.int32)
        for k in range(3):
            t = wm[k] * c
            t = t + wa[k]
            t = D[n + 1 - STEPS[k][0], m + 1 - STEPS[k][1]] + t
            take = t < best
            best[take] = t[take]
            code[take] = k
        D[n + 1, m + 1] = best
        steps[n + 1, m + 1] = code
    return D[1:, 1:], steps[1:, 1:]


def dtw(C, weights_mul=None, weights_add=None, subseq=False, loops=False):
    """D, steps, wp (end first) and the end column, as librosa.sequence.dtw(C=C, ...) forms them."""
    D, steps = (dtw_loops if loops else dtw_diag)(C, weights_mul, weights_add, subseq)
    start = int(np.argmin(D[-1, :])) if subseq else D.shape[1] - 1
    return D, steps, backtrack(steps, subseq, start), start


def check_path(wp, N, M, subseq=False, start=None):
    """A path end first: monotone, only the three steps, the right end points."""
    wp = np.asarray(wp)
    assert wp.ndim == 2 and wp.shape[1] == 2 and len(wp) >= 1
    assert wp[0, 0] == N - 1 and wp[0, 1] == (M - 1 if start is None else start)
    if subseq:
        assert wp[-1, 0] == 0
    else:
        assert tuple(wp[-1]) == (0, 0)
    d = wp[:-1] - wp[1:]
    assert all(tuple(s) in ((1, 1), (0, 1), (1, 0)) for s in d)
    assert wp.min() >= 0 and wp[:, 0].max() < N and wp[:, 1].max() < M


def path_cost(C64, wp, weights_mul=None, weights_add=None):
    """The float64 cost of walking `wp` (end first) over C64 with the step weights."""
    wm, wa = _weights(weights_mul, weights_add)
    wp = np.asarray(wp)[::-1]
    total = float(C64[wp[0, 0], wp[0, 1]])
    for a, b in zip(wp[:-1], wp[1:]):
        k = {(1, 1): 0, (0, 1): 1, (1, 0): 2}[tuple(b - a)]
        total += wm[k] * float(C64[b[0], b[1]]) + wa[k]
    return total
