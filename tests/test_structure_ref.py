"""tests/structure_ref.py pinned to what is installed (np.roll, scipy.ndimage, scikit-learn), the host tables of
sygnals_amd/_structure.py, and the condition of the gated GPU cases of tests/structure_cases.py.  No device."""
import numpy as np
import pytest

from sygnals_amd import _structure as ST
from tests import structure_cases as SC
from tests import structure_ref as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ shear
@pytest.mark.parametrize("t", (1, 2, 3, 8, 65))
def test_shear_is_np_roll_column_by_column(t):
    rec = np.random.default_rng(t).standard_normal((t, t)).astype(np.float32)
    for pad in (True, False):
        n = 2 * t if pad else t
        ext = np.concatenate([rec, np.zeros((n - t, t), np.float32)])
        want = np.stack([np.roll(ext[:, i], -i) for i in range(t)], axis=1)          # lag[l, i] = R~[(l + i) mod n, i]
        assert np.array_equal(R.recurrence_to_lag(rec, pad=pad), want)
        assert np.array_equal(R.recurrence_to_lag(rec, pad=pad, axis=0), R.recurrence_to_lag(rec.T, pad=pad).T)
        assert np.array_equal(R.lag_to_recurrence(want), rec)
        free = np.random.default_rng(t + 1).standard_normal((n, t))
        assert np.array_equal(R.lag_to_recurrence(free), np.stack([np.roll(free[:, i], i) for i in range(t)], axis=1)[:t])
        assert np.array_equal(R.lag_to_recurrence(free.T, axis=0), R.lag_to_recurrence(free).T)
    with pytest.raises(ValueError):
        R.recurrence_to_lag(np.ones((2, 3)))
    with pytest.raises(ValueError):
        R.lag_to_recurrence(np.ones((3, 2)))


# ------------------------------------------------------------------ filter bank and path_enhance
@pytest.mark.parametrize("n", (3, 7))
def test_tap_lists_reproduce_convolve_on_unit_impulses(n):
    """Every filter of the bank, a unit impulse at every position of a 9 x 9 matrix: the tap list places the float64
    weights where scipy.ndimage.convolve does, exactly."""
    from scipy.ndimage import convolve
    F = ST.path_filters(n)
    assert len(F.kernels) == 7 and any(k.shape[0] % 2 == 0 for k in F.kernels)        # rotated arrays do come out even-sized
    for f, ker in enumerate(F.kernels):
        lo, hi = F.fstart[f], F.fstart[f + 1]
        assert hi - lo == np.count_nonzero(ker)
        for p in range(9):
            for q in range(9):
                imp = np.zeros((9, 9))
                imp[p, q] = 1.0
                got = R.taps_correlate(imp, F.taps[lo:hi, 0], F.taps[lo:hi, 1], F.w64[lo:hi], "constant")
                assert np.array_equal(got, convolve(imp, ker, mode="constant")), (n, f, p, q)


@pytest.mark.parametrize("n", (3, 4, 7, 8, 31))
def test_filter_bank_is_librosas_recipe(n):
    from scipy.ndimage import rotate
    from scipy.signal import get_window
    F = ST.path_filters(n)
    ratios = np.logspace(-1, 1, 7, base=2)
    for ker, ratio, mine in zip(F.kernels, ratios, R.filter_bank(n)):
        win = np.diag(get_window("hann", n, fftbins=False))
        if not np.isclose(np.arctan(ratio), np.pi / 4):
            win = rotate(win, 45 - np.degrees(np.arctan(ratio)), order=5, prefilter=False)
        win = np.clip(win, 0, None)
        assert np.allclose(ker, win / win.sum(), rtol=0, atol=1e-15) and np.array_equal(ker, mine)  # (the sum's order is the layout's)
    assert np.array_equal(F.taps[:, 2].view(np.float32), F.w64.astype(np.float32)) and np.all(F.taps[:, 3] == 0)
    assert F.fstart[0] == 0 and F.fstart[-1] == len(F.w64) and F.taps.dtype == np.int32 and F.fstart.dtype == np.int32
    assert F.span == (F.taps[:, 0].min(), F.taps[:, 0].max(), F.taps[:, 1].min(), F.taps[:, 1].max())
    assert ST.path_filters(n) is F                                                    # kept per argument tuple
    zm = ST.path_filters(n, zero_mean=True)
    assert all(np.count_nonzero(k) == k.size for k in zm.kernels) and abs(sum(k.sum() for k in zm.kernels)) < 1e-12


def test_filter_bank_sparsity_at_51():
    F = ST.path_filters(51)
    counts = np.diff(F.fstart)
    assert sorted(k.shape[0] for k in F.kernels) == [51, 56, 56, 61, 61, 65, 65]
    assert counts.min() == 49 and 500 <= counts.max() <= 527 and counts.sum() < 3300


def test_filter_bank_refusals():
    with pytest.raises(ValueError, match="min_ratio=4.0 cannot exceed max_ratio=2.0"):
        ST.path_filters(7, min_ratio=4.0)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n=.* must be a positive integer"):
            ST.path_filters(bad)
    with pytest.raises(ValueError, match="n_filters"):
        ST.path_filters(7, n_filters=0)
    with pytest.raises(ValueError, match="max_ratio"):
        ST.path_filters(7, max_ratio=-1.0)
    assert len(ST.path_filters(7, n_filters=1).kernels) == 1
    with pytest.raises(ValueError, match="mode='cubic' is not served"):
        ST.boundary_code("x", "cubic")


@pytest.mark.parametrize("shape", ((1, 1), (2, 2), (5, 3), (40, 33)))
@pytest.mark.parametrize("n", (3, 4, 7, 8))
def test_tap_form_equals_ndimage_convolve(shape, n):
    """Every served mode, odd and even filter sizes: the tap lists over the periodic index maps against
    scipy.ndimage.convolve in float64, within 1e-12 of the peak; and the whole path_enhance built from them."""
    from scipy.ndimage import convolve
    Rm = np.random.default_rng(shape[0] * 100 + n).standard_normal(shape)
    peak = np.abs(Rm).max()
    for zm in (False, True):
        F = ST.path_filters(n, zero_mean=zm)
        for mode in R.MODES:
            best = None
            for f, ker in enumerate(F.kernels):
                lo, hi = F.fstart[f], F.fstart[f + 1]
                got = R.taps_correlate(Rm, F.taps[lo:hi, 0], F.taps[lo:hi, 1], F.w64[lo:hi], mode, 0.25)
                assert np.abs(got - convolve(Rm, ker, mode=mode, cval=0.25)).max() <= 1e-12 * peak, (shape, n, mode, f)
                best = got if best is None else np.maximum(best, got)
            for clip in (True, False):
                want = R.path_enhance(Rm, n, zero_mean=zm, clip=clip, mode=mode, cval=0.25)
                assert np.abs((np.clip(best, 0, None) if clip else best) - want).max() <= 1e-12 * peak, (shape, n, mode, clip)


def test_path_gate_has_room_in_float32():
    """The gate of the GPU cases, 1e-5 max|R|, against float32: a filter's weights are not negative and sum to 1 (to 2 in
    absolute value under zero_mean), so rounding the weights once moves a sum by at most 2^-24 * 2 max|R| = 1.2e-7, and
    four partial sums of at most 1521 / 4 = 381 fmas each (the 39 x 39 arrays of n = 31 under zero_mean) carry at most
    (381 + 2) 2^-24 * 2 max|R| = 4.6e-5 in the worst case and its root, 2.4e-6, on random signs."""
    for n in (3, 7, 31):
        for zm in (False, True):
            F = ST.path_filters(n, zero_mean=zm)
            for f in range(7):
                w = F.w64[F.fstart[f]:F.fstart[f + 1]]
                assert np.abs(w).sum() <= 2.0 + 1e-9 and len(w) <= 1521
                assert np.abs(w.astype(np.float32).astype(np.float64) - w).sum() <= 2.0 ** -24 * 2.0


# ------------------------------------------------------------------ diagonal median
@pytest.mark.parametrize("t", SC.MEDIAN_T)
def test_diag_median_is_shear_median_filter_shear(t):
    """Against scipy.ndimage.median_filter between the two shears: every value equal, and bit for bit wherever the median is
    not a zero (SciPy returns either of -0 and +0 when both stand in a window; the restatement orders -0 below +0)."""
    Rm = SC.median_matrix(t)
    assert (Rm < 0).any() or t == 1
    assert t < 7 or (np.signbit(Rm) & (Rm == 0)).any() and (~np.signbit(Rm) & (Rm == 0)).any()
    for w in SC.MEDIAN_W:
        for mode in SC.MEDIAN_MODES:
            for axis in (-1, 0):
                for pad in (True, False):
                    a = R.diag_median(Rm, w, mode, SC.MEDIAN_CVAL, pad, axis)
                    b = R.diag_median_scipy(Rm, w, mode, SC.MEDIAN_CVAL, pad, axis)
                    assert a.dtype == np.float32 and np.array_equal(a, b), (t, w, mode, axis, pad)
                    nz = a != 0
                    assert np.array_equal(bits(a)[nz], bits(b)[nz]), (t, w, mode, axis, pad)
    assert np.array_equal(bits(R.diag_median(Rm, 1)), bits(Rm))


def test_order_keys():
    v = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], dtype=np.float32)
    k = R.ord_keys(v)
    assert np.all(np.diff(k.astype(np.int64)) > 0) and np.array_equal(bits(R.keys_value(k)), bits(v))


# ------------------------------------------------------------------ chain Ward
def test_chain_ward_is_sklearns_connectivity_ward():
    pytest.importorskip("sklearn")
    for T, D, k in SC.WARD_CASES:
        assert np.array_equal(SC.ward_reference(T, D, k)[0], R.sklearn_ward(SC.ward_frames(T, D), k)), (T, D, k)
    X = SC.ward_ragged_batch()
    for b, n, k in SC.WARD_RAGGED:
        assert np.array_equal(R.chain_ward(X[b, :n], k)[0], R.sklearn_ward(X[b, :n], k)), (b, n, k)


def test_ward_cases_meet_the_gap_condition():
    """Every gated case: throughout the restatement's run the best merge cost stays clear of the second best by more than
    1e-9 of it, so a float64 device sum in another order picks the same merges."""
    for T, D, k in SC.WARD_CASES + (SC.WARD_CAP,):
        bounds, gap = SC.ward_reference(T, D, k)
        assert len(bounds) == k and bounds[0] == 0 and np.all(np.diff(bounds) > 0)
        assert gap > SC.WARD_GAP, (T, D, k, gap)
    X = SC.ward_ragged_batch()
    for b, n, k in SC.WARD_RAGGED:
        off = 5 if (b, n) == (0, 40) else (1 if (b, n) == (1, 64) else 0)
        assert R.chain_ward(X[b, off:off + n], k)[1] > SC.WARD_GAP
    for b in range(4):
        assert R.chain_ward(X[b], 4)[1] > SC.WARD_GAP
    Xs = np.random.default_rng(3).standard_normal((2, 140, 5)).astype(np.float32)     # the subsegment test's clips
    edges = R.fix_frames(SC.SUBSEGMENT_FRAMES, 140)
    for b in range(2):
        for lo, hi in zip(edges[:-1], edges[1:]):
            for ns in (1, 4, 9):
                assert R.chain_ward(Xs[b, lo:hi], min(ns, hi - lo))[1] > SC.WARD_GAP


def test_crafted_ties_go_left():
    X, k, want = SC.WARD_CRAFTED
    assert np.array_equal(R.chain_ward(X, k)[0], want)
    assert np.array_equal(R.chain_ward(X, 9)[0], np.arange(9)) and np.array_equal(R.chain_ward(X, 1)[0], [0])
    assert np.array_equal(R.chain_ward(X, 3)[0], [0, 3, 6])
    for bad in (0, 10):
        with pytest.raises(ValueError):
            R.chain_ward(X, bad)


# ------------------------------------------------------------------ subsegment, sync, frame fixing
def test_fix_frames_and_definitions():
    assert np.array_equal(ST.fix_frames(SC.SUBSEGMENT_FRAMES, 140), [0, 7, 30, 64, 65, 90, 140])
    assert np.array_equal(ST.fix_frames(SC.SUBSEGMENT_FRAMES, 140, pad=False), [7, 30, 64, 65, 90])
    assert np.array_equal(ST.fix_frames([5], 5), [0, 5]) and np.array_equal(ST.fix_frames([0, 0], 3), [0, 3])
    for f, x, p in ((SC.SUBSEGMENT_FRAMES, 140, True), ([3, 1, 1], 9, False)):
        assert np.array_equal(ST.fix_frames(f, x, p), R.fix_frames(f, x, p))
    with pytest.raises(ValueError, match="negative frame index"):
        ST.fix_frames([3, -1], 9)
    with pytest.raises(ValueError, match="one-dimensional array of integers"):
        ST.fix_frames([1.5], 9)
    X = np.random.default_rng(0).standard_normal((140, 3)).astype(np.float32)
    sub = R.subsegment(X, SC.SUBSEGMENT_FRAMES, 4)
    edges = [0, 7, 30, 64, 65, 90, 140]
    want = np.concatenate([lo + R.chain_ward(X[lo:hi], min(4, hi - lo))[0] for lo, hi in zip(edges[:-1], edges[1:])])
    assert np.array_equal(sub, want) and len(sub) == 4 * 5 + 1 and np.all(np.diff(sub) > 0)
    s = R.sync(X, SC.SYNC_EDGES, "mean")
    assert s.shape == (6, 3) and np.allclose(s[2], X[3:67].astype(np.float64).mean(axis=0), rtol=0, atol=1e-15)
    assert np.array_equal(R.sync(X, SC.SYNC_EDGES, "max")[3], X[67:132].max(axis=0))
    assert np.array_equal(R.sync(X, SC.SYNC_EDGES, "min")[0], X[0])
    assert list(np.diff(SC.SYNC_EDGES)) == [1, 2, 64, 65, 1, 7]
