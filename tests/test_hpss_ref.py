"""The float64 HPSS restatement (tests/hpss_ref.py) against its own definition, scipy and the reference's own test."""
import numpy as np
import pytest
import scipy.ndimage as nd

from tests import hpss_ref as R

# (k, T) pairs where scipy 1.15's 2-D median_filter with size (1, k), mode "reflect", departs from the definition of
# hpss_ref.median_filter_axis (which is the contract); pinned so that a scipy change is noticed
SCIPY_DEPARTURES = {2: 16, 4: 32, 6: 48}    # T: smallest k at which scipy departs (for every larger k <= 63 too)


def _signals():
    rng = np.random.default_rng(3)
    return [R.sine(), R.clicks(), rng.standard_normal(7680) * 0.3]


def test_identities():
    for y in _signals():
        D = R.stft(y)
        Mh, Mp, _, _ = R.masks(np.abs(D), 31, 2.0, 1.0, tiny=np.finfo(np.float64).tiny)
        assert np.abs(Mh + Mp - 1).max() <= 2.3e-16
        yh, yp = R.hpss(y)
        pk = np.abs(y).max()
        assert np.abs(yh + yp - y).max() <= 7e-16 * max(pk, 1.0)
        assert np.abs(R.istft(D, len(y)) - y).max() <= 6e-16 * max(pk, 1.0)


def test_median_definition_against_scipy():
    rng = np.random.default_rng(0)
    found = {}
    for T in range(1, 71):
        X = rng.random((3, T))
        for k in range(1, 64):
            ours = R.median_filter_axis(X, k, axis=1)
            sp = nd.median_filter(X, size=(1, k), mode="reflect")
            if not np.array_equal(ours, sp):
                found.setdefault(T, k)
                assert T in SCIPY_DEPARTURES and k >= SCIPY_DEPARTURES[T], (T, k)
    assert found == SCIPY_DEPARTURES


def test_median_is_rank_of_folded_window():
    rng = np.random.default_rng(1)
    for n in range(1, 17):
        x = rng.random(n)
        for k in (1, 2, 8, 15, 16, 30, 31, 63):
            ours = R.median_filter_axis(x[None, :], k, axis=1)[0]
            ext = np.concatenate([x, x[::-1]])
            for i in range(n):
                win = np.array([ext[(i - k // 2 + j) % (2 * n)] for j in range(k)])
                assert ours[i] == np.sort(win)[k // 2]
    # bins axis == time axis on the transpose, even windows take the upper median
    X = rng.random((40, 9))
    assert np.array_equal(R.median_filter_axis(X, 6, axis=0), R.median_filter_axis(X.T, 6, axis=1).T)
    assert np.array_equal(R.median_filter_axis(np.array([[1.0, 2.0]]), 2, axis=1), [[1.0, 2.0]])


def test_softmask_rules():
    X = np.array([0.0, 1.0, 2.0, 0.0])
    Xr = np.array([0.0, 1.0, 1.0, 3.0])
    assert np.array_equal(R.softmask(X, Xr, 2.0, split_zeros=True), [0.5, 0.5, 0.8, 0.0])
    assert np.array_equal(R.softmask(X, Xr, 2.0, split_zeros=False), [0.0, 0.5, 0.8, 0.0])
    assert np.array_equal(R.softmask(X, Xr, np.inf), [0.0, 0.0, 1.0, 0.0])
    assert R.softmask(np.float32([1e-39]), np.float32([0.0]), 1.0, True)[0] == 0.5
    with pytest.raises(ValueError):
        R.masks(np.ones((5, 5)), 31, 2.0, (0.5, 1.0))


def test_reference_expectations():
    hs = R.harmonic_to_noise_ratio(R.sine(), 1024, 256)
    hc = R.harmonic_to_noise_ratio(R.clicks(), 1024, 256)
    assert len(hs) == len(hc) == 1 + 22050 // 256 == 87
    assert np.nanmean(hs) > 10.0 and np.nanmean(hc) < 5.0
    assert np.all(np.isnan(R.harmonic_to_noise_ratio(np.zeros(4096))))
