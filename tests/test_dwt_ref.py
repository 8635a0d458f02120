"""Pins tests/dwt_ref.py (the float64 restatement of PyWavelets' dwt / idwt / wavedec / waverec that the device wavelet
transform is held to) by published known answers and self-checks, and sygnals_amd/_wavelets.py against it."""
import math
import warnings

import numpy as np
import pytest

from tests import dwt_ref as R

DB = [f"db{n}" for n in range(1, 11)]
R2 = math.sqrt(0.5)


def test_known_answers_from_the_pywavelets_documentation():
    cA2, cD2, cD1 = R.wavedec(np.arange(1.0, 9.0), "db1", level=2)
    np.testing.assert_allclose(cA2, [5.0, 13.0], atol=1e-12)
    np.testing.assert_allclose(cD2, [-2.0, -2.0], atol=1e-12)
    np.testing.assert_allclose(cD1, [-R2] * 4, atol=1e-12)
    cA, cD = R.dwt(np.arange(1.0, 7.0), "db1")
    np.testing.assert_allclose(cA, [2.12132034, 4.94974747, 7.77817459], atol=5e-9)
    np.testing.assert_allclose(cD, [-R2] * 3, atol=1e-12)
    cA, cD = R.dwt(np.arange(1.0, 7.0), "db2", "symmetric")
    np.testing.assert_allclose(cA, [1.76776695, 2.31078903, 5.13921616, 8.13172798], atol=5e-9)
    np.testing.assert_allclose(cD, [-0.61237244, 0.0, 0.0, 0.61237244], atol=5e-9)


def test_db2_closed_form_and_db4_digits():
    s3 = math.sqrt(3.0)
    want = np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * math.sqrt(2.0))
    dec_lo, dec_hi, rec_lo, rec_hi = R.wavelet_filters("db2")
    np.testing.assert_allclose(rec_lo, want, atol=1e-14)
    np.testing.assert_allclose(dec_lo, want[::-1], atol=1e-14)
    np.testing.assert_allclose(dec_hi, [-want[0], want[1], -want[2], want[3]], atol=1e-14)
    np.testing.assert_allclose(rec_hi, dec_hi[::-1], atol=0)
    np.testing.assert_allclose(R.wavelet_filters("db4")[2], [0.23037781, 0.71484657, 0.63088077, -0.02798377, -0.18703481,
                                                             0.03084138, 0.03288301, -0.01059740], atol=5e-9)
    for a, b in zip(R.wavelet_filters("haar"), R.wavelet_filters("db1")):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(R.wavelet_filters("haar")[2], [R2, R2], atol=1e-15)


@pytest.mark.parametrize("name", DB)
def test_orthonormal_with_n_vanishing_moments(name):
    N = int(name[2:])
    dec_lo, dec_hi, rec_lo, rec_hi = R.wavelet_filters(name)
    assert rec_lo.size == 2 * N
    assert abs(rec_lo.sum() - math.sqrt(2.0)) <= 1e-12
    for h in (rec_lo, dec_hi):
        for m in range(N):
            s = float(np.dot(h[:h.size - 2 * m], h[2 * m:]))
            assert abs(s - (1.0 if m == 0 else 0.0)) <= 1e-12, (name, m, s)
    for m in range(-N + 1, N):                  # low and high pass are orthogonal at every even shift
        a, b = (rec_lo[2 * m:], rec_hi[:rec_hi.size - 2 * m]) if m >= 0 else (rec_lo[:2 * m], rec_hi[-2 * m:])
        assert abs(float(np.dot(a, b))) <= 1e-12
    k = np.arange(2.0 * N)
    for p in range(N):                          # sum_k k^p dec_hi[k] = 0, relative to the size of the terms
        terms = k ** p * dec_hi
        assert abs(terms.sum()) <= 1e-9 * np.abs(terms).sum(), (name, p)
    assert abs(np.sum(k ** N * dec_hi)) > 1e-3  # and no more than N


def _rule(i, N, mode):
    """The extension table of the issue: index of ext(x)[i], or None for a zero."""
    if 0 <= i < N:
        return i
    if mode == "reflect" and N == 1:
        mode = "constant"
    if mode == "symmetric":
        m = i % (2 * N)
        return 2 * N - 1 - m if m >= N else m
    if mode == "reflect":
        m = i % (2 * N - 2)
        return 2 * N - 2 - m if m >= N else m
    if mode == "periodic":
        return i % N
    if mode == "constant":
        return min(max(i, 0), N - 1)
    return None


@pytest.mark.parametrize("mode", R.MODES)
def test_extension_follows_the_index_rules_even_many_times_over(mode):
    pad = 19                                    # db10: F - 1
    for N in range(1, 12):
        x = np.arange(1.0, N + 1.0)
        want = [0.0 if _rule(i, N, mode) is None else x[_rule(i, N, mode)] for i in range(-pad, N + pad)]
        assert np.array_equal(R.extend(x, pad, mode), np.array(want)), (mode, N)


def test_dwt_is_the_stated_sum():
    rng = np.random.default_rng(3)
    for name, N, mode in (("db3", 11, "reflect"), ("db10", 5, "symmetric"), ("db2", 1, "periodic"), ("db5", 16, "zero")):
        x = rng.standard_normal(N)
        dec_lo, dec_hi, _, _ = R.wavelet_filters(name)
        F = dec_lo.size
        cA, cD = R.dwt(x, name, mode)
        assert cA.size == cD.size == (N + F - 1) // 2
        for o in range(cA.size):
            xs = [0.0 if _rule(2 * o + 1 - j, N, mode) is None else x[_rule(2 * o + 1 - j, N, mode)] for j in range(F)]
            assert abs(cA[o] - float(np.dot(dec_lo, xs))) <= 1e-13 and abs(cD[o] - float(np.dot(dec_hi, xs))) <= 1e-13


@pytest.mark.parametrize("mode", R.MODES)
def test_perfect_reconstruction(mode):
    worst = 0.0
    for name in R.WAVELETS:
        for L in list(range(1, 41)) + [100, 257]:
            x = np.random.default_rng(1000 + L).standard_normal(L)
            y = R.waverec(R.wavedec(x, name, mode=mode), name)
            assert y.size in (L, L + 1)
            worst = max(worst, float(np.max(np.abs(y[:L] - x))))
    assert worst <= 1e-12, worst


def test_lengths_and_max_level():
    for n, f, want in ((8, 2, 3), (1000, 8, 7), (6, 8, 0), (7, 8, 0), (13, 8, 0), (14, 8, 1), (1, 2, 0), (5, 20, 0),
                       (18, 20, 0), (19, 20, 0), (38, 20, 1), (1 << 24, 2, 24), (32768, 8, 12)):
        assert R.dwt_max_level(n, f) == want, (n, f)
    for n in range(1, 60):
        for name in ("db1", "db2", "db4", "db10"):
            F = R.wavelet_filters(name)[0].size
            assert R.dwt(np.zeros(n), name)[0].size == R.dwt_coeff_len(n, F) == (n + F - 1) // 2
    c = R.wavedec(np.zeros(1000), "db4", level=3)
    assert [a.size for a in c] == [131, 131, 255, 503]
    assert len(R.wavedec(np.zeros(5), "db4")) == 2        # level=None: max(1, 0)
    with pytest.raises(ValueError):
        R.waverec([np.zeros(5), np.zeros(7)], "db1")
    assert R.waverec([np.zeros(6), np.zeros(5)], "db1").size == 10     # the approximation's last sample is dropped


# ---------------------------------------------------------------- sygnals_amd/_wavelets.py against the restatement
def test_host_tables_agree_with_the_restatement():
    from sygnals_amd import _wavelets as W
    assert set(W.WAVELETS) == set(R.WAVELETS) and set(W.MODES) == set(R.MODES)
    for name in R.WAVELETS:
        for a, b in zip(W.filters(name), R.wavelet_filters(name)):
            assert a.dtype == np.float64 and np.max(np.abs(a - b)) <= 1e-12, name
        assert W.filter_length(name) == R.wavelet_filters(name)[0].size
    for n in list(range(1, 100)) + [1000, 32768, 1 << 24]:
        for f in (2, 4, 8, 20):
            assert W.dwt_max_level(n, f) == R.dwt_max_level(n, f), (n, f)
            assert W.dwt_coeff_len(n, f) == R.dwt_coeff_len(n, f)
    assert W.wavedec_lengths(1000, 8, 3) == [131, 131, 255, 503]
    assert W.waverec_length([131, 131, 255, 503], 8) == 1000
    assert W.waverec_length([6, 5], 2) == 10


def test_host_tables_refuse_what_is_not_served():
    from sygnals_amd import _wavelets as W
    for name in ("sym5", "coif1", "bior3.7", "db11", "db0", "dmey", 4):
        with pytest.raises(ValueError, match="wavelets served are haar, db1, db2"):
            W.filters(name)
    for mode in ("periodization", "smooth", "antisymmetric", "antireflect", "wrap"):
        with pytest.raises(ValueError, match="modes served are symmetric, reflect, periodic, constant, zero"):
            W.mode_code(mode)
    assert [W.mode_code(m) for m in ("zero", "constant", "symmetric", "reflect", "periodic")] == [0, 1, 2, 3, 4]
    for level in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="integer >= 1"):
            W.resolve_level(1000, 8, level)
    assert W.resolve_level(1000, 8, None) == 7 and W.resolve_level(5, 8, None) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert W.resolve_level(1000, 8, 7) == 7
    with pytest.warns(UserWarning, match="too high"):
        assert W.resolve_level(1000, 8, 9) == 9
    for lens in ([5, 7], [8, 5], [5]):
        with pytest.raises(ValueError):
            W.waverec_length(lens, 2)
    with pytest.raises(ValueError):
        W.waverec_length([3, 3], 8)             # fewer pairs than half the filter
