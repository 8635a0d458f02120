"""The device self-similarity (ops.sim_knn, recurrence_matrix, nn_filter, repet_masks, core.decompose's
separate_repeating) against the float64 restatement tests/similarity_ref.py.  Gates: the sorted kept distances of a row
within 1e-5 of the clip's largest kept distance; neighbour sets equal on the rows whose boundary gap exceeds 2e-5 of that
scale (tests/similarity_cases.py, conditioned on the CPU in tests/test_similarity_ref.py); what is defined exactly is
compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import similarity_cases as SC
from tests import similarity_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops as o
    o.require_gpu()
    return o


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def check_lists(got, X, Y, k, width, metric, what, x_len=None, y_len=None):
    """One clip's device lists against float64: counts and padding exactly, sorted distances within the gate, sets on the
    rows with a clear boundary.  Returns the worst distance error, relative to the scale."""
    idx, dist, count = got
    ridx, rdist, rcount = R.knn(X, Y, k, width, metric, x_len, y_len)
    gap, scale = R.boundary_gaps(X, Y, k, width, metric, x_len, y_len)
    assert np.array_equal(count, rcount), what
    worst = 0.0
    for i in range(X.shape[0]):
        c = rcount[i]
        assert np.all(idx[i, c:] == -1) and np.all(np.isposinf(dist[i, c:])), (what, i)
        assert np.all(np.diff(dist[i, :c]) >= 0), (what, i)
        assert len(set(idx[i, :c])) == c, (what, i)
        if c:
            worst = max(worst, float(np.max(np.abs(dist[i, :c].astype(np.float64) - rdist[i, :c]))))
        if gap[i] > SC.GAP_MIN * scale:
            assert set(idx[i, :c]) == set(ridx[i, :c]), (what, i)
    rel = worst / scale if scale > 0 else worst
    print(f"{what}: worst kept distance off by {rel:.2e} of the scale {scale:.3g}")
    assert rel <= SC.DIST_GATE, (what, rel)
    return rel


@pytest.mark.parametrize("case", SC.KNN_CASES, ids=SC.case_id)
def test_knn_cases(ops, case):
    T, D, k, width, metric, kind, seed = case
    X = SC.frames(kind, T, D, seed)
    got = host(*ops.sim_knn(dev(X)[None], None, k, width, metric))
    assert got[0].shape == (1, T, k) and got[0].dtype == np.int32 and got[2].dtype == np.int32
    check_lists([g[0] for g in got], X, None, k, width, metric, SC.case_id(case))


@pytest.mark.parametrize("metric", R.METRICS)
def test_cross_lists_and_default_k(ops, metric):
    rng = np.random.default_rng(31)
    X, Y = rng.standard_normal((70, 13)).astype(np.float32), rng.standard_normal((45, 13)).astype(np.float32)
    got = host(*ops.sim_knn(dev(X)[None], dev(Y)[None], 9, 1, metric))
    check_lists([g[0] for g in got], X, Y, 9, 1, metric, f"cross {metric}")
    idx, _, _ = ops.sim_knn(dev(X)[None], metric=metric)
    assert idx.shape[2] == R.default_k(70) == ops.sim_default_k(70)


def test_repeated_integer_pattern_is_exact(ops):
    """Equal frames give bit-equal zeros wherever they land (row blocks of 16, column tiles of 64), and equal distances
    resolve to the smaller index."""
    P, r, D = 7, 30, 70
    base = (np.arange(P * D).reshape(P, D) % 11).astype(np.float32) + np.arange(P)[:, None].astype(np.float32)
    X = np.tile(base, (r, 1))
    idx, dist, count = host(*ops.sim_knn(dev(X)[None], None, r - 1, 1, "sqeuclidean"))
    for i in range(P * r):
        assert list(idx[0, i]) == [j for j in range(i % P, P * r, P) if j != i], i
    assert np.all(dist == 0) and not np.any(np.signbit(dist)) and np.all(count == r - 1)
    idx, dist, count = host(*ops.sim_knn(dev(X)[None], None, 12, 3, "cosine"))
    ridx, _, _ = R.knn(X, None, 12, 3, "sqeuclidean")                            # the same ties, the same order
    assert np.array_equal(idx[0], ridx) and np.all(dist[0] == dist[0][:, :1])


def test_batch_ragged_and_shared_y(ops):
    rng = np.random.default_rng(32)
    X = rng.standard_normal((3, 40, 9)).astype(np.float32)
    Y = rng.standard_normal((1, 50, 9)).astype(np.float32)
    Xd = dev(X)
    both = host(*ops.sim_knn(Xd, None, 6, 2, "euclidean"))
    for b in range(3):
        one = host(*ops.sim_knn(Xd[b:b + 1], None, 6, 2, "euclidean"))
        assert all(np.array_equal(w[b], o[0]) for w, o in zip(both, one)), b
    xl = np.array([40, 17, 0], dtype=np.int32)
    got = host(*ops.sim_knn(Xd, None, 20, 1, "cosine", x_len=xl))
    for b in range(3):
        check_lists([g[b] for g in got], X[b], None, 20, 1, "cosine", f"ragged {b}", x_len=xl[b])
    assert np.all(got[2][2] == 0) and np.all(got[2][1, 17:] == 0)
    yl = np.array([50, 3, 33], dtype=np.int32)
    shared = host(*ops.sim_knn(Xd, dev(Y), 5, 1, "sqeuclidean", y_len=yl))         # batch stride 0: one Y for every clip
    for b in range(3):
        check_lists([g[b] for g in shared], X[b], Y[0], 5, 1, "sqeuclidean", f"shared Y {b}", y_len=yl[b])
    wide = dev(np.concatenate([X, X], axis=2))[:, :, :9]                           # strided rows
    assert all(np.array_equal(a, b) for a, b in zip(host(*ops.sim_knn(wide, None, 6, 2, "euclidean")), both))


def test_more_clips_than_grid_rows(ops):
    B = 65537
    X = np.random.default_rng(33).standard_normal((B, 2, 1)).astype(np.float32)
    idx, dist, count = host(*ops.sim_knn(dev(X), None, 1, 1, "sqeuclidean"))
    for b in (0, 65534, 65535, B - 1):
        assert list(idx[b, :, 0]) == [1, 0] and count[b, 0] == 1 == count[b, 1]
        e = X[b, 0, 0] - X[b, 1, 0]
        assert np.all(dist[b, :, 0] == e * e)
    assert np.all(count == 1)


@pytest.mark.parametrize("sym", [False, True])
def test_recurrence_matrix_from_the_device_lists(ops, sym):
    X = SC.frames("normal", 97, 6, 41)
    lists = ops.sim_knn(dev(X)[None], None, 11, 2, "euclidean")
    idx, dist, count = (a[0] for a in host(*lists))
    for mode in ("connectivity", "distance"):
        for self in (False, True):
            got = ops.sim_dense(*lists, mode=mode, sym=sym, self=self)[0].cpu().numpy()
            want, _ = R.dense(idx, dist, count, None, mode, sym, None, self)
            assert np.array_equal(got, want.astype(np.float32)), (mode, self)
            if self:
                assert np.all(np.diag(got) == (0 if mode == "distance" else 1))
    got, bw = ops.sim_dense(*lists, mode="affinity", sym=sym, self=True, return_bandwidth=True)
    want, rbw = R.dense(idx, dist.astype(np.float64), count, None, "affinity", sym, None, True)
    assert abs(float(bw[0]) - rbw) <= 1e-6 * rbw
    assert np.max(np.abs(got[0].cpu().numpy() - want)) <= 1e-5 and np.all(np.diag(got[0].cpu().numpy()) == 1)
    fixed = ops.sim_dense(*lists, mode="affinity", sym=sym, bandwidth=0.75)[0].cpu().numpy()
    assert np.max(np.abs(fixed - R.dense(idx, dist.astype(np.float64), count, None, "affinity", sym, 0.75)[0])) <= 1e-5
    whole = ops.recurrence_matrix(dev(X)[None], k=11, width=2, sym=sym, mode="connectivity")[0].cpu().numpy()
    assert np.array_equal(whole, R.dense(idx, dist, count, None, "connectivity", sym)[0].astype(np.float32))
    if sym:
        assert np.array_equal(whole, whole.T)


def test_cross_similarity_and_librosa_orientation(ops):
    from sygnals_amd.core import similarity as SM
    rng = np.random.default_rng(42)
    X, Y = rng.standard_normal((33, 5)).astype(np.float32), rng.standard_normal((58, 5)).astype(np.float32)
    lists = ops.sim_knn(dev(X)[None], dev(Y)[None], 4, 1, "cosine")
    idx, dist, count = (a[0] for a in host(*lists))
    got = ops.recurrence_matrix(dev(X)[None], dev(Y)[None], k=4, metric="cosine", mode="distance")[0].cpu().numpy()
    assert got.shape == (33, 58) and np.array_equal(got, R.dense(idx, dist, count, 58, "distance")[0].astype(np.float32))
    assert np.array_equal(SM.cross_similarity(X.T, Y.T, k=4, metric="cosine", mode="distance"), got.T)
    rec = SM.recurrence_matrix(X.T, k=3, width=2, sym=True)
    assert rec.shape == (33, 33) and np.array_equal(rec, rec.T) and rec.dtype == np.float32
    with pytest.raises(ValueError, match="bandwidth of a clip is 0"):
        ops.recurrence_matrix(torch.ones(1, 6, 3, device="cuda"), k=2, mode="affinity")


def ulp_ok(got, want):
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want).astype(np.float32)))


def check_filter(ops, S, idx, count, weights, what):
    """ops.nn_filter against the restatement on the same lists: mean and average within 1e-5 of the peak of S, the median
    bit for bit at odd counts and within one float32 spacing at even ones."""
    Sd, idd, cd = dev(S)[None], dev(idx, np.int32)[None], dev(count, np.int32)[None]
    peak = float(np.max(np.abs(S)))
    got = ops.nn_filter(Sd, idd, cd, None, "mean")[0].cpu().numpy()
    err = np.max(np.abs(got - R.nn_filter(S, idx, count, None, "mean"))) / peak
    got = ops.nn_filter(Sd, idd, cd, dev(weights)[None], "average")[0].cpu().numpy()
    erra = np.max(np.abs(got - R.nn_filter(S, idx, count, weights, "average"))) / peak
    print(f"{what}: mean {err:.2e}, average {erra:.2e} of the peak")
    assert err <= 1e-5 and erra <= 1e-5, what
    got = ops.nn_filter(Sd, idd, cd, None, "median")[0].cpu().numpy()
    want = R.nn_filter(S, idx, count, None, "median")
    odd = (count % 2 == 1) | (count == 0)
    assert np.array_equal(got[odd], want[odd]), what
    assert ulp_ok(got[~odd], want[~odd]), what


@pytest.mark.parametrize("F", [1, 63, 64, 65, 1025])
def test_nn_filter_on_given_lists(ops, F):
    """G1: lists made here, with every count that crosses a lane group, an empty list, zeros in S and a zero weight."""
    T, k = 300, 256
    rng = np.random.default_rng(50 + F)
    S = np.abs(rng.standard_normal((T, F))).astype(np.float32)
    S[rng.random((T, F)) < 0.2] = 0
    counts = np.array([0, 1, 2, 63, 64, 65, 255, 256, 3, 4], dtype=np.int32)
    count = counts[np.arange(T) % len(counts)]
    idx = np.full((T, k), -1, dtype=np.int32)
    w = rng.random((T, k)).astype(np.float32)
    w[:, 1] = 0
    for i in range(T):
        idx[i, :count[i]] = rng.permutation(T)[:count[i]]
    check_filter(ops, S, idx, count, w, f"given lists F={F}")
    out = ops.nn_filter(dev(S)[None], dev(idx, np.int32)[None], dev(count, np.int32)[None], None, "median")[0].cpu().numpy()
    assert np.array_equal(out[count == 0], S[count == 0])


def test_nn_filter_on_the_device_lists(ops):
    """G2: the device's own lists, negative values too, a strided S and the affinity weights of core.decompose."""
    from sygnals_amd.core import decompose as DC
    X = SC.frames("normal", 130, 70, 61)
    lists = ops.sim_knn(dev(X)[None], None, 10, 2, "cosine")
    idx, dist, count = (a[0] for a in host(*lists))
    check_filter(ops, X, idx, count, np.exp(-dist).astype(np.float32), "device lists")
    wide = dev(np.concatenate([X, X], axis=1))[None][:, :, :70]
    assert torch.equal(ops.nn_filter(wide, lists[0], lists[2], None, "median"), ops.nn_filter(dev(X)[None], lists[0], lists[2], None, "median"))
    got = DC.nn_filter_batch(dev(X)[None], aggregate="average", k=10, width=2, metric="cosine")[0].cpu().numpy()
    bw = R.bandwidth_of(dist.astype(np.float64), count)
    want = R.nn_filter(X, idx, count, np.exp(-dist.astype(np.float64) / bw), "average")
    assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(X))
    assert np.array_equal(DC.nn_filter(X.T, aggregate=np.median, k=10, width=2, metric="cosine").T,
                          ops.nn_filter(dev(X)[None], lists[0], lists[2], None, "median")[0].cpu().numpy())
    rec = R.dense(idx, np.exp(-dist.astype(np.float64)), count, None, "distance")[0].T          # librosa's orientation
    got = DC.nn_filter(X.T, rec=rec.astype(np.float32), aggregate="average").T
    assert np.max(np.abs(got - R.nn_filter(X, idx, count, np.exp(-dist), "average"))) <= 1e-5 * np.max(np.abs(X))


@pytest.mark.parametrize("power", [1.0, 2.0, 0.5])
def test_repet_masks(ops, power):
    rng = np.random.default_rng(70)
    S = np.abs(rng.standard_normal((2, 37, 65))).astype(np.float32)
    Rf = np.abs(rng.standard_normal((2, 37, 65))).astype(np.float32)
    Rf[0, :5] = S[0, :5]                                                          # S = Sf
    S[1, :4] = 0                                                                  # S = 0
    Rf[1, 2:4] = 0                                                                # both 0
    mf, mb = host(*ops.repet_masks(dev(S), dev(Rf), 2.0, 10.0, power))
    wf, wb = R.repet_masks(S, Rf, 2.0, 10.0, power)
    ef, eb = np.max(np.abs(mf - wf)), np.max(np.abs(mb - wb))
    print(f"repet_masks power={power}: foreground {ef:.2e}, background {eb:.2e}")
    assert ef <= 1e-6 and eb <= 1e-6
    assert np.all(mf[0, :5] == 0) and np.all(mb[0, :5] == 1) and np.all(mf[1, :4] == 0) and np.all(mb[1, 2:4] == 0)


@pytest.mark.parametrize("L", [8192, 16385])
def test_separate_repeating_against_the_restatement(ops, L):
    """(a) fed the device's STFT and lists, both outputs within 1e-5 of the clip's peak."""
    from sygnals_amd.core import decompose as DC
    rng = np.random.default_rng(L)
    t = np.arange(L) / 22050.0
    y = (0.5 * np.sin(2 * np.pi * 220 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.1 * rng.standard_normal(L)).astype(np.float32)
    out, D, idx, count = DC.separate_repeating_batch(dev(y)[None], width=2, return_parts=True)
    assert out.shape == (1, 2, L)
    Dc = D[0].cpu().numpy().astype(np.float64)
    fg, bg = R.separate_from(Dc[..., 0] + 1j * Dc[..., 1], idx[0].cpu().numpy(), count[0].cpu().numpy(), L)
    peak = float(np.max(np.abs(y)))
    got = out[0].cpu().numpy()
    ef, eb = np.max(np.abs(got[0] - fg)) / peak, np.max(np.abs(got[1] - bg)) / peak
    print(f"separate_repeating L={L}: foreground {ef:.2e}, background {eb:.2e} of the peak")
    assert ef <= 1e-5 and eb <= 1e-5
    f1, b1 = DC.separate_repeating(y, 22050, width_seconds=2 * 512 / 22050)
    assert np.array_equal(f1, got[0]) and np.array_equal(b1, got[1])


def test_separate_repeating_of_a_periodic_clip(ops):
    """(b) a clip tiled from one period of 512 samples (the hop): the frames clear of the padding are bit-identical, so
    the filter returns them unchanged, the foreground is exactly 0 wherever only such frames reach and the background is
    the STFT round trip there."""
    from sygnals_amd.core import decompose as DC
    L = 16384
    period = np.random.default_rng(80).standard_normal(512).astype(np.float32)
    y = np.tile(period, L // 512)
    out, D, idx, count = DC.separate_repeating_batch(dev(y)[None], width=3, return_parts=True)
    S = ops.cabs_pow(D, 1)[0].cpu().numpy()
    assert np.all(S[2:31] == S[2])                                               # frames 2 .. 30 see no padding
    assert idx.shape[2] == R.default_k(33, 3) and np.all((idx[0, 2:31].cpu().numpy() >= 2) & (idx[0, 2:31].cpu().numpy() <= 30))
    lo, hi = 2 * 512 + 1024, 30 * 512 - 1024                                     # samples that frames 2 .. 30 alone reach
    fg, bg = out[0, 0].cpu().numpy(), out[0, 1].cpu().numpy()
    assert np.all(fg[lo:hi] == 0)
    back = ops.istft2048(D, length=L)[0].cpu().numpy()
    assert np.max(np.abs(bg[lo:hi] - back[lo:hi])) <= 1e-6 * np.max(np.abs(y))


def test_ragged_blocks_after_full_lists_past_the_grid_cap(ops):
    """A workgroup that filled its 16 lists for clip b meets, 65 535 clips later, a clip whose rows of that block all lie
    past x_len (or whose searched frames are none): no tile follows the sentinels there, and the lists must come out
    empty all the same."""
    B, T, k = 65537, 32, 4
    X = np.random.default_rng(34).standard_normal((B, T, 1)).astype(np.float32)
    xl = np.full(B, T, dtype=np.int32)
    xl[65535], xl[65536] = 5, 0                                                  # block 1 past x_len; nothing at all
    Xd = dev(X)
    got = host(*ops.sim_knn(Xd, None, k, 1, "sqeuclidean", x_len=xl))
    assert np.all(got[2][:65535] == k)
    for b in (0, 65534, 65535, 65536):
        check_lists([g[b] for g in got], X[b], None, k, 1, "sqeuclidean", f"clip {b}", x_len=xl[b])
    assert np.all(got[2][65535, 5:] == 0) and np.all(got[0][65535, 5:] == -1) and np.all(got[2][65536] == 0)
    yl = np.zeros(B, dtype=np.int32)
    yl[:65535] = T
    idx, dist, count = host(*ops.sim_knn(Xd, Xd, k, 1, "sqeuclidean", y_len=yl))   # y_len = 0: queries without candidates
    assert np.all(count[:65535] == k) and np.all(count[65535:] == 0) and np.all(idx[65535:] == -1) and np.all(np.isposinf(dist[65535:]))


def test_nn_filter_on_the_restatement_lists(ops):
    """G1 as the issue names it: the lists of the float64 restatement (the given-lists test above builds its own, to reach
    every count), and the refusal of lists that point outside the clip."""
    X = SC.frames("magnitudes", 90, 65, 62)
    idx, dist, count = R.knn(X, None, 9, 2, "cosine")
    check_filter(ops, X, idx, count, np.exp(-dist).astype(np.float32), "restatement lists")
    bad = idx.copy()
    bad[3, 0] = 90
    with pytest.raises(ValueError, match="entries of idx below it in \\[0, 90\\)"):
        ops.nn_filter(dev(X)[None], dev(bad, np.int32)[None], dev(count, np.int32)[None])
