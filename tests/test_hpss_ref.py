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


def test_median_with_ties_against_scipy():
    """The window pairs of tests/hpss_cases.py on an input of nine values (ties, zeros next to non-zeros), T below the window
    included, wherever scipy keeps to the definition (SCIPY_DEPARTURES)."""
    from tests import hpss_cases as K
    compared = 0
    for T in K.MEDIAN_T:
        S = K.mag32(K.tie_spectrum(2, T))[:, :, :200]                                # [2, T, 200]
        for kh, kp in K.MEDIAN_WINDOWS:
            H = R.median_filter_axis(S, kh, axis=1)
            P = R.median_filter_axis(S, kp, axis=2)
            for b in range(2):                           # (scipy in the 2-D form test_median_definition_against_scipy pins)
                X = np.ascontiguousarray(S[b])
                if T not in SCIPY_DEPARTURES or kh < SCIPY_DEPARTURES[T]:
                    assert np.array_equal(H[b], nd.median_filter(X.T.copy(), size=(1, kh), mode="reflect").T), (T, kh)
                    compared += 1
                assert np.array_equal(P[b], nd.median_filter(X, size=(1, kp), mode="reflect")), (T, kp)
                # the batch axis is a plain leading axis
                assert np.array_equal(H[b], R.median_filter_axis(S[b], kh, axis=0))
                assert np.array_equal(P[b], R.median_filter_axis(S[b], kp, axis=1))
    assert compared == 2 * len(K.MEDIAN_T) * len(K.MEDIAN_WINDOWS)                   # none of these T is a departure


def test_rms_power_uncentred_against_a_loop():
    rng = np.random.default_rng(5)
    for fl, hop, L in ((63, 7, 1000), (4096, 1024, 4096), (64, 64, 640), (5, 3, 6)):
        y = rng.standard_normal(L)
        got = R.rms_power(y, fl, hop, center=False)
        want = np.array([np.mean(y[s:s + fl] ** 2) for s in range(0, L - fl + 1, hop)])
        assert got.shape == want.shape == (1 + (L - fl) // hop,)
        np.testing.assert_allclose(got, want, rtol=1e-14)
        yh, yp = y, rng.standard_normal(L) * 0.1
        hnr, ph, pp = R.hnr_from_components(yh, yp, fl, hop, center=False)
        np.testing.assert_allclose(hnr, 10 * np.log10(want / R.rms_power(yp, fl, hop, center=False)), rtol=1e-12)
    # the defaults are the centred framing existing callers have
    y = rng.standard_normal(700)
    assert np.array_equal(R.rms_power(y, 64, 16), R.rms_power(y, 64, 16, center=True))
    assert len(R.rms_power(y, 64, 16)) == 1 + 700 // 16
    assert np.array_equal(R.hnr_from_components(y, y[::-1], 64, 16)[0], R.hnr_from_components(y, y[::-1], 64, 16, True)[0])


def test_istft_of_fewer_frames_than_the_length_asks():
    rng = np.random.default_rng(6)
    D = rng.standard_normal((1025, 5)) + 1j * rng.standard_normal((1025, 5))
    y = R.istft(D, 8000)
    assert y.shape == (8000,) and np.isfinite(y).all()
    assert np.flatnonzero(y).max() == 3071 and not y[3072:].any()                    # frame 4 ends at sample 4 * 512 + 1023
    assert np.array_equal(y[:3000], R.istft(D, 3000))
    # irfft ignores the imaginary parts of the first and the last bin
    D0 = D.copy()
    D0[0] = D0[0].real
    D0[1024] = D0[1024].real
    assert np.array_equal(R.istft(D0, 8000), y)
    # frames past those the length needs are not read
    D9 = np.concatenate([D, np.full((1025, 4), np.nan)], axis=1)
    assert np.array_equal(R.istft(D9, 500), R.istft(D, 500))


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
