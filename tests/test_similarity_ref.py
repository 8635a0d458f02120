"""tests/similarity_ref.py, the float64 contract of the self-similarity kernels: pinned to scikit-learn's brute
NearestNeighbors and scipy's cdist where they define the same thing, known answers, and the condition of every gated
case of the GPU tests (tests/similarity_cases.py)."""
import numpy as np
import pytest

from tests import similarity_cases as SC
from tests import similarity_ref as R


@pytest.mark.parametrize("metric", R.METRICS)
def test_distances_equal_cdist(metric):
    cdist = pytest.importorskip("scipy.spatial.distance").cdist
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((37, 12)).astype(np.float32), rng.standard_normal((29, 12)).astype(np.float32)
    want = cdist(X.astype(np.float64), Y.astype(np.float64), metric)
    assert np.max(np.abs(R.distances(X, Y, metric) - want)) <= 1e-12
    Z = np.zeros((2, 12), dtype=np.float32)                                    # our own definition: scipy gives NaN
    assert np.array_equal(R.distances(Z, Y, "cosine"), np.ones((2, 29)))


@pytest.mark.parametrize("T,D,k,width,metric", [(60, 7, 5, 1, "euclidean"), (90, 12, 9, 3, "cosine"), (41, 3, 12, 2, "sqeuclidean")])
def test_lists_equal_sklearn_pruned_the_librosa_way(T, D, k, width, metric):
    """librosa asks the brute search for k + 2 width neighbours, drops the band, keeps the first k: on tie-free inputs
    that is the top k among the out-of-band candidates."""
    NN = pytest.importorskip("sklearn.neighbors").NearestNeighbors
    X = np.random.default_rng(T).standard_normal((T, D)).astype(np.float32)
    nn = NN(n_neighbors=min(T, k + 2 * width), metric=metric, algorithm="brute").fit(X.astype(np.float64))
    dist, ind = nn.kneighbors(X.astype(np.float64))
    idx, d, count = R.knn(X, k=k, width=width, metric=metric)
    for i in range(T):
        keep = np.abs(ind[i] - i) >= width
        want, wd = ind[i][keep][:k], dist[i][keep][:k]
        assert count[i] == len(want) == k
        assert np.array_equal(idx[i], want)
        assert np.max(np.abs(d[i] - wd)) <= 1e-9


def test_cross_lists_equal_sklearn():
    NN = pytest.importorskip("sklearn.neighbors").NearestNeighbors
    rng = np.random.default_rng(5)
    X, Y = rng.standard_normal((30, 6)).astype(np.float32), rng.standard_normal((44, 6)).astype(np.float32)
    _, ind = NN(n_neighbors=4, algorithm="brute").fit(Y.astype(np.float64)).kneighbors(X.astype(np.float64))
    idx, _, count = R.knn(X, Y, k=4)
    assert np.array_equal(idx, ind) and np.all(count == 4)


def test_default_k_and_refusals():
    assert R.default_k(7750) == 178 and R.default_k(431) == 42 and R.default_k(1) == 2 and R.default_k(10 ** 6) == 256
    assert R.default_k(33, 3) == 12 and R.default_k(4, 5) == 2
    with pytest.raises(ValueError, match="is not served"):
        R.distances(np.zeros((2, 2)), np.zeros((2, 2)), "cityblock")
    with pytest.raises(ValueError):
        R.knn(np.zeros((4, 2)), np.zeros((4, 2)), width=2)
    with pytest.raises(ValueError):
        R.knn(np.zeros((4, 2)), k=257)


def test_repeated_pattern_has_its_repeats_in_index_order():
    P, r = 5, 6
    base = np.arange(P * 3).reshape(P, 3).astype(np.float32) * 2 + 1
    X = np.tile(base, (r, 1))
    idx, dist, count = R.knn(X, k=r - 1, width=1, metric="sqeuclidean")
    for i in range(P * r):
        want = [j for j in range(i % P, P * r, P) if j != i]
        assert list(idx[i]) == want and np.all(dist[i] == 0) and count[i] == r - 1


def test_padding_ragged_and_no_candidates():
    X = np.random.default_rng(1).standard_normal((6, 3)).astype(np.float32)
    idx, dist, count = R.knn(X, k=9)
    assert np.all(count == 5) and np.all(idx[:, 5:] == -1) and np.all(np.isinf(dist[:, 5:]))
    idx, dist, count = R.knn(X, k=2, width=6)
    assert np.all(count == 0) and np.all(idx == -1)
    idx, dist, count = R.knn(X, k=9, x_len=4)
    assert list(count) == [3, 3, 3, 3, 0, 0] and idx[:4, :3].max() == 3


def test_dense_modes_sym_self_and_bandwidth():
    X = np.random.default_rng(2).standard_normal((40, 4)).astype(np.float32)
    idx, dist, count = R.knn(X, k=6)
    Rc, _ = R.dense(idx, dist, count)
    assert Rc.sum() == 40 * 6 and np.all(np.diag(Rc) == 0)
    Rs, _ = R.dense(idx, dist, count, sym=True)
    assert np.array_equal(Rs, Rs.T) and np.array_equal(Rs, np.minimum(Rc, Rc.T))
    Rd, _ = R.dense(idx, dist, count, mode="distance", self=True)
    assert np.all(np.diag(Rd) == 0) and np.array_equal(Rd > 0, Rc > 0)
    Ra, bw = R.dense(idx, dist, count, mode="affinity", sym=True, self=True)
    keep = R.mutual(idx, count)
    rows = [dist[i, :6][keep[i]].max() for i in range(40) if keep[i].any()]
    assert bw == np.median(rows) and np.all(np.diag(Ra) == 1)
    assert np.allclose(Ra[Rs > 0], np.exp(-Rd[Rs > 0] / bw))
    with pytest.raises(ValueError, match="bandwidth is 0"):
        R.dense(*R.knn(np.ones((5, 2), dtype=np.float32), k=2), mode="affinity")
    with pytest.raises(ValueError, match="is not served"):
        R.dense(idx, dist, count, mode="sparse")


def test_nn_filter_known_answers():
    S = np.full((9, 5), 3.25, dtype=np.float32)
    X = np.random.default_rng(3).standard_normal((9, 2)).astype(np.float32)
    idx, dist, count = R.knn(X, k=4)
    for agg in ("mean", "median"):
        assert np.array_equal(R.nn_filter(S, idx, count, None, agg), S)
    assert np.max(np.abs(R.nn_filter(S, idx, count, np.exp(-dist), "average") - S)) <= 1e-14       # sum w S / sum w rounds
    S = np.random.default_rng(4).random((9, 5)).astype(np.float32)
    count[2] = 0                                                               # an empty list keeps the frame
    out = R.nn_filter(S, idx, count, aggregate="median")
    assert np.array_equal(out[2], S[2]) and out.dtype == np.float32
    assert np.array_equal(out[0], np.median(S[idx[0, :4]], axis=0))
    w = np.ones((9, 4)); w[:, 1] = 0
    assert np.allclose(R.nn_filter(S, idx, count, w, "average")[0], S[idx[0, [0, 2, 3]]].astype(np.float64).mean(axis=0))
    with pytest.raises(ValueError, match="is not served"):
        R.nn_filter(S, idx, count, aggregate="max")


def test_repet_masks_known_answers():
    S = np.array([[1.0, 0.0, 2.0, 4.0]], dtype=np.float32)
    Rf = np.array([[1.0, 0.0, 5.0, 1.0]], dtype=np.float32)                    # S = Sf twice (one of them 0), S < R, S > R
    mf, mb = R.repet_masks(S, Rf, 2.0, 10.0, 2.0)
    assert list(mb[0, :3]) == [1.0, 0.0, 1.0] and list(mf[0, :3]) == [0.0, 0.0, 0.0]
    assert mb[0, 3] == pytest.approx(1.0 / (1.0 + 36.0)) and mf[0, 3] == pytest.approx(9.0 / (9.0 + 100.0))


@pytest.mark.parametrize("case", SC.KNN_CASES, ids=SC.case_id)
def test_gated_case_leaves_out_at_most_a_tenth_of_its_rows(case):
    T, D, k, width, metric, kind, seed = case
    gap, scale = R.boundary_gaps(SC.frames(kind, T, D, seed), k=k, width=width, metric=metric)
    left_out = np.mean(gap <= SC.GAP_MIN * scale)
    assert left_out <= SC.LEFT_OUT_MAX, f"{left_out:.3f} of the rows have a boundary gap under {SC.GAP_MIN} of {scale}"


@pytest.mark.parametrize("T,D,k", [(257, 12, 33), (300, 1025, 20), (64, 3, 7), (1000, 40, 64)])
def test_gaps_are_rare_and_float32_reproduces_the_sets(T, D, k):
    """Over random normals at most 2 % of the rows have a boundary gap under 1e-5 of the scale, and a naive float32
    evaluation in difference form reproduces every float64 set of the other rows."""
    X = SC.frames("normal", T, D, 100 + T)
    gap, scale = R.boundary_gaps(X, k=k, metric="euclidean")
    assert np.mean(gap <= 1e-5 * scale) <= 0.02
    idx, _, _ = R.knn(X, k=k, metric="euclidean")
    d32 = np.zeros((T, T), dtype=np.float32)
    for i in range(T):
        e = X[i][None, :] - X
        d32[i] = np.sqrt(np.sum(e * e, axis=1, dtype=np.float32))
    np.fill_diagonal(d32, np.inf)
    for i in np.nonzero(gap > 1e-5 * scale)[0]:
        assert set(np.argsort(d32[i], kind="stable")[:k]) == set(idx[i])
