"""The device structure analysis (ops.recurrence_to_lag, lag_to_recurrence, path_enhance, diag_median, agglomerative,
subsegment, segment_sync) against the float64 restatement tests/structure_ref.py.  Gates: the shear, the diagonal median,
the boundaries and the max / min aggregates are exact; path_enhance |out - ref64| <= 1e-5 max|R| per matrix; the segment
mean within 1e-6 of the segment's peak.  The Ward cases' merge-cost gaps are proved on the CPU in
tests/test_structure_ref.py."""
import numpy as np
import pytest
import torch

from tests import structure_cases as SC
from tests import structure_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from sygnals_amd import ops as o
    o.require_gpu()
    return o


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def square(t, B=1, seed=0):
    return np.random.default_rng(9 * t + seed).standard_normal((B, t, t)).astype(np.float32)


# ------------------------------------------------------------------ shear
@pytest.mark.parametrize("t", SC.SHEAR_T)
@pytest.mark.parametrize("axis", (-1, 0))
@pytest.mark.parametrize("pad", (True, False))
def test_shear_is_exact_and_inverts(ops, t, axis, pad):
    for B in (1, 3):
        rec = square(t, B)
        lag = ops.recurrence_to_lag(dev(rec), pad=pad, axis=axis)
        want = np.stack([R.recurrence_to_lag(r, pad=pad, axis=axis) for r in rec])
        assert lag.shape == want.shape and np.array_equal(bits(lag.cpu().numpy()), bits(want)), (t, axis, pad, B)
        back = ops.lag_to_recurrence(lag, axis=axis).cpu().numpy()
        assert np.array_equal(bits(back), bits(rec)), (t, axis, pad, B)
        # a lag matrix that is no shear of anything: the inverse alone against the restatement
        free = np.random.default_rng(t).standard_normal(want.shape).astype(np.float32)
        got = ops.lag_to_recurrence(dev(free), axis=axis).cpu().numpy()
        assert np.array_equal(bits(got), bits(np.stack([R.lag_to_recurrence(f, axis=axis) for f in free]))), (t, axis, pad, B)


def test_shear_strided_rows_and_shared_batch(ops):
    t = 65
    wide = dev(square(2 * t, 2))
    view = wide[:, 3:3 + t, 5:5 + t]                         # row stride 2 t, batch stride 4 t t
    want = np.stack([R.recurrence_to_lag(r) for r in view.cpu().numpy()])
    assert np.array_equal(bits(ops.recurrence_to_lag(view).cpu().numpy()), bits(want))
    lagw = dev(np.random.default_rng(1).standard_normal((2, 2 * t + 1, t + 7)))
    lv = lagw[:, :2 * t, 7:]
    want = np.stack([R.lag_to_recurrence(r) for r in lv.cpu().numpy()])
    assert np.array_equal(bits(ops.lag_to_recurrence(lv).cpu().numpy()), bits(want))
    same = view[:1].expand(3, t, t)                          # batch stride 0
    got = ops.recurrence_to_lag(same, axis=0).cpu().numpy()
    assert np.array_equal(bits(got[0]), bits(got[2])) and np.array_equal(bits(got[0]), bits(R.recurrence_to_lag(view[0].cpu().numpy(), axis=0)))


def test_shear_past_the_grid_cap(ops):
    B = 65537                                                # more matrices than rows of a grid's y dimension
    rec = np.arange(B * 4, dtype=np.float32).reshape(B, 2, 2)
    lag = ops.recurrence_to_lag(dev(rec)).cpu().numpy()
    want = np.zeros((B, 4, 2), dtype=np.float32)
    want[:, 0, 0], want[:, 1, 0], want[:, 0, 1], want[:, 3, 1] = rec[:, 0, 0], rec[:, 1, 0], rec[:, 1, 1], rec[:, 0, 1]
    assert np.array_equal(lag, want)
    assert np.array_equal(ops.lag_to_recurrence(dev(lag)).cpu().numpy(), rec)


# ------------------------------------------------------------------ path_enhance
@pytest.mark.parametrize("case", SC.PATH_CASES, ids=SC.path_id)
def test_path_enhance_cases(ops, case):
    """Measured on MI355X: worst 3.6e-7 of max|R| over the 101 cases in two runs of this file alone; in one run of the whole
    suite n31-2x2-reflect-f7 came out 18 max|R| off (cause not found: it depends on what ran before in the process)."""
    n, (T, Tc), mode, nf, zm, clip = case
    Rm = SC.path_matrix(T, Tc)
    got = ops.path_enhance(dev(Rm), n, n_filters=nf, zero_mean=zm, clip=clip, mode=mode, cval=SC.PATH_CVAL).cpu().numpy()[0]
    want = SC.path_reference(case)
    err = float(np.max(np.abs(got.astype(np.float64) - want))) / float(np.max(np.abs(Rm)))
    print(f"path_enhance {SC.path_id(case)}: worst error {err:.2e} of max|R|")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= SC.GATE, (SC.path_id(case), err)
    if not clip and T * Tc > 1:
        assert (Rm < 0).any() and (want < 0).any()           # negative entries in, negative outputs kept


@pytest.mark.parametrize("n,size", ((7, (17, 5)), (31, (65, 127)), (3, (2, 2))))
def test_path_enhance_batch_equals_rows_and_strides(ops, n, size):
    Rm = dev(SC.path_matrix(size[0], size[1], 3))
    whole = ops.path_enhance(Rm, n, mode="mirror").cpu().numpy()
    again = ops.path_enhance(Rm, n, mode="mirror").cpu().numpy()
    assert np.array_equal(bits(whole), bits(again))
    for b in range(3):
        assert np.array_equal(bits(whole[b]), bits(ops.path_enhance(Rm[b:b + 1], n, mode="mirror").cpu().numpy()[0])), b
    wide = torch.zeros((3, size[0] + 2, size[1] + 9), device="cuda")
    wide[:, 1:-1, 4:4 + size[1]] = Rm
    assert np.array_equal(bits(ops.path_enhance(wide[:, 1:-1, 4:4 + size[1]], n, mode="mirror").cpu().numpy()), bits(whole))


@pytest.mark.parametrize("n", (3, 7, 31))
def test_path_enhance_impulse_returns_the_taps(ops, n):
    """One filter, a unit impulse at P, zeros around: out[P - (dr, dc)] is the float32 tap bit for bit, 0 elsewhere."""
    from sygnals_amd import _structure as ST
    for ratio in (0.5, 1.0, 2.0):
        F = ST.path_filters(n, max_ratio=ratio, min_ratio=ratio, n_filters=1)
        T, Tc, P = 70, 90, (33, 47)
        imp = np.zeros((1, T, Tc), dtype=np.float32)
        imp[0, P[0], P[1]] = 1.0
        got = ops.path_enhance(dev(imp), n, max_ratio=ratio, min_ratio=ratio, n_filters=1, mode="constant").cpu().numpy()[0]
        want = np.zeros((T, Tc), dtype=np.float32)
        want[P[0] - F.taps[:, 0], P[1] - F.taps[:, 1]] = F.taps[:, 2].view(np.float32)
        assert np.array_equal(bits(got), bits(want)), (n, ratio)


# ------------------------------------------------------------------ diagonal median
@pytest.mark.parametrize("t", SC.MEDIAN_T)
@pytest.mark.parametrize("w", SC.MEDIAN_W)
def test_diag_median_bit_for_bit(ops, t, w):
    Rm = SC.median_matrix(t)
    for mode in SC.MEDIAN_MODES:
        for axis in (-1, 0):
            got = ops.diag_median(dev(Rm)[None], w, mode=mode, cval=SC.MEDIAN_CVAL, axis=axis).cpu().numpy()[0]
            want = R.diag_median(Rm, w, mode, SC.MEDIAN_CVAL, True, axis)
            assert np.array_equal(bits(got), bits(want)), (t, w, mode, axis)


def test_diag_median_unpadded_batch_and_strides(ops):
    t = 65
    Rm = np.stack([SC.median_matrix(t), -SC.median_matrix(t), SC.median_matrix(t).T])
    for pad in (True, False):
        got = ops.diag_median(dev(Rm), 7, mode="wrap", pad=pad).cpu().numpy()
        for b in range(3):
            assert np.array_equal(bits(got[b]), bits(R.diag_median(Rm[b], 7, "wrap", 0.0, pad, -1))), (pad, b)
    wide = torch.zeros((3, t, 2 * t), device="cuda")
    wide[:, :, 9:9 + t] = dev(Rm)
    got = ops.diag_median(wide[:, :, 9:9 + t], 31, axis=0).cpu().numpy()
    for b in range(3):
        assert np.array_equal(bits(got[b]), bits(R.diag_median(Rm[b], 31, "reflect", 0.0, True, 0))), b


# ------------------------------------------------------------------ agglomerative
def starts(bounds, count, s=0):
    b, c = bounds[s].cpu().numpy(), int(count[s])
    assert np.all(b[c:] == -1)
    return b[:c]


@pytest.mark.parametrize("case", SC.WARD_CASES, ids=lambda c: "T%d-D%d-k%d" % c)
def test_agglomerative_cases(ops, case):
    T, D, k = case
    bounds, count = ops.agglomerative(dev(SC.ward_frames(T, D))[None], k)
    assert bounds.dtype == torch.int32 and tuple(bounds.shape) == (1, k) and int(count[0]) == k
    assert np.array_equal(starts(bounds, count), SC.ward_reference(T, D, k)[0])


def test_agglomerative_at_the_served_cap(ops):
    T, D, k = SC.WARD_CAP
    assert T == ops.structure_constants()["agg_t_max"]
    bounds, count = ops.agglomerative(dev(SC.ward_frames(T, D))[None], k)
    assert np.array_equal(starts(bounds, count), SC.ward_reference(T, D, k)[0])


def test_agglomerative_leftmost_on_ties(ops):
    X, k, want = SC.WARD_CRAFTED
    bounds, count = ops.agglomerative(dev(X)[None], k)
    assert np.array_equal(starts(bounds, count), want)
    assert np.array_equal(R.chain_ward(X, k)[0], want)


def test_agglomerative_ragged_spans_and_strides(ops):
    X = SC.ward_ragged_batch()
    B, T, D = X.shape
    off = [b * T + (5 if i == 0 else 0) for i, (b, _, _) in enumerate(SC.WARD_RAGGED)]
    off[2] = 1 * T + 1                                        # two spans of clip 1: frame 0 alone, then frames 1 .. 64
    ln = [n for _, n, _ in SC.WARD_RAGGED]
    ks = [k for _, _, k in SC.WARD_RAGGED]
    wide = torch.zeros((B, T, 2 * D + 3), device="cuda")
    wide[:, :, 2:2 + D] = dev(X)
    for Xd in (dev(X), wide[:, :, 2:2 + D], dev(X)[:, :, :]):
        bounds, count = ops.agglomerative(Xd, ks, off, ln)
        assert tuple(bounds.shape) == (5, max(ks))
        for s in range(5):
            b, t0 = divmod(off[s], T)
            assert np.array_equal(starts(bounds, count, s), R.chain_ward(X[b, t0:t0 + ln[s]], ks[s])[0]), s
    whole, _ = ops.agglomerative(dev(X), 4)                   # every clip one span; a batch equals its rows
    for b in range(B):
        assert np.array_equal(whole[b].cpu().numpy(), ops.agglomerative(dev(X[b:b + 1]), 4)[0][0].cpu().numpy())
        assert np.array_equal(whole[b].cpu().numpy(), R.chain_ward(X[b], 4)[0])


# ------------------------------------------------------------------ subsegment, segment_sync
def test_subsegment_matches_the_restatement(ops):
    X = np.random.default_rng(3).standard_normal((2, 140, 5)).astype(np.float32)
    for n_segments in (1, 4, 9):
        bounds, count = ops.subsegment(dev(X), SC.SUBSEGMENT_FRAMES, n_segments)
        for b in range(2):
            want = R.subsegment(X[b], SC.SUBSEGMENT_FRAMES, n_segments)
            assert int(count[b]) == len(want) and np.array_equal(bounds[b].cpu().numpy(), want), (n_segments, b)


@pytest.mark.parametrize("D", SC.SYNC_D)
def test_segment_sync(ops, D):
    X = np.random.default_rng(D).standard_normal((3, 140, D)).astype(np.float32)
    wide = torch.zeros((3, 140, D + 5), device="cuda")
    wide[:, :, 1:1 + D] = dev(X)
    for Xd in (dev(X), wide[:, :, 1:1 + D]):
        for agg in ("mean", "max", "min"):
            got = ops.segment_sync(Xd, SC.SYNC_EDGES, agg).cpu().numpy()
            assert got.shape == (3, len(SC.SYNC_EDGES) - 1, D)
            for b in range(3):
                want = R.sync(X[b], SC.SYNC_EDGES, agg)
                if agg == "mean":
                    peak = np.stack([np.abs(X[b, lo:hi]).max(axis=0) for lo, hi in zip(SC.SYNC_EDGES[:-1], SC.SYNC_EDGES[1:])])
                    assert np.all(np.abs(got[b] - want) <= 1e-6 * peak), (D, b)
                else:
                    assert np.array_equal(got[b].astype(np.float64), want), (D, agg, b)
    per_clip = np.stack([SC.SYNC_EDGES, SC.SYNC_EDGES // 2, np.minimum(SC.SYNC_EDGES * 2, 140)])
    got = ops.segment_sync(dev(X), per_clip, "max").cpu().numpy()
    for b in range(3):
        e = per_clip[b]
        for j in range(len(e) - 1):
            want = X[b, e[j]:e[j + 1]].max(axis=0) if e[j + 1] > e[j] else np.zeros(D, np.float32)
            assert np.array_equal(got[b, j], want), (b, j)
