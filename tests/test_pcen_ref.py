"""The float64 restatement of PCEN (tests/pcen_ref.py) against closed forms, direct formulas, a brute-force reflected maximum
and, where it imports, librosa; the host rules of sygnals_amd/_pcen.py against it.  No device.  Every check holds to 1e-12."""
import numpy as np
import pytest

from sygnals_amd import _pcen as PC
from tests import pcen_ref as R

TOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def spec(M=6, T=50, seed=0):
    return np.random.default_rng(seed).standard_normal((M, T)) ** 2


def test_b_values():
    assert abs(R.b_of(0.4, 22050, 512) - 0.05638943879134889) <= TOL
    assert abs(R.b_of(0.4, 16000, 160) - 0.024689453048712014) <= TOL
    assert abs(PC.b_from_time_constant(0.4, 22050, 512) - 0.05638943879134889) <= TOL
    assert abs(PC.b_from_time_constant(0.4, 16000, 160) - 0.024689453048712014) <= TOL


def test_impulse_response():
    for b in (1.0, 0.3, 0.056, 1e-3):
        x = np.zeros((1, 40))
        x[0, 0] = 1.0
        M, zf = R.smoother(x, b, zi=np.zeros((1, 1)))
        assert close(M[0], b * (1 - b) ** np.arange(40))
        assert close(zf[0, 0], (1 - b) * M[0, -1])


def test_constant_row_closed_form():
    S = np.ones((3, 30))
    b = R.b_of()
    M, zf = R.smoother(S, b)
    assert close(M, 1.0) and close(zf, 1 - b)                    # the default state is that of a unit step: not scaled by S
    gain, bias, power, eps = 0.98, 2.0, 0.5, 1e-6
    want = (1.0 / (eps + 1.0) ** gain + bias) ** power - bias ** power
    assert close(R.pcen(S), want)
    assert not close(R.pcen(3.0 * S)[:, 0], (3.0 / (eps + 3.0) ** gain + bias) ** power - bias ** power)


def test_power_zero_and_bias_zero_against_direct_formulas():
    S = spec()
    b = 0.1
    M, _ = R.smoother(S, b)
    for gain, eps in ((0.98, 1e-6), (0.5, 1e-3), (0.0, 1e-6)):
        smooth = (eps + M) ** (-gain)
        assert close(R.pcen(S, b=b, gain=gain, eps=eps, power=0.0), np.log1p(S * smooth))
        assert close(R.pcen(S, b=b, gain=gain, eps=eps, bias=0.0, power=0.7), (S * smooth) ** 0.7)
        assert close(R.pcen(S, b=b, gain=gain, eps=eps, bias=2.0, power=0.5), (S * smooth + 2.0) ** 0.5 - 2.0 ** 0.5)


def test_zero_rows_are_exactly_zero():
    S = spec()
    S[2] = 0.0
    S[4, 10:20] = 0.0
    for kw in ({}, {"power": 0.0}, {"bias": 0.0}, {"bias": 0.0, "power": 1.0}):
        y = R.pcen(S, **kw)
        assert np.all(y[2] == 0.0) and np.all(y[4, 10:20] == 0.0) and np.all(np.isfinite(y))


def test_max_size_against_brute_force():
    import scipy.ndimage
    for M in range(1, 10):
        S = spec(M, 7, seed=M)
        for ms in range(1, M + 1):
            want = R.reflected_max(S, ms)
            assert np.array_equal(scipy.ndimage.maximum_filter1d(S, ms, axis=-2), want), (M, ms)
            ref = S if ms == 1 else want
            Mm, _ = R.smoother(ref, 0.2)
            assert close(R.pcen(S, b=0.2, max_size=ms), (S * (1e-6 + Mm) ** -0.98 + 2.0) ** 0.5 - 2.0 ** 0.5)


def test_per_band_vectors_equal_scalar_calls():
    M = 5
    S = spec(M, 40, seed=3)
    gain = np.array([0.98, 0.5, 0.0, 0.8, 1.0])
    bias = np.array([2.0, 0.0, 1.0, 10.0, 0.0])
    power = np.array([0.5, 0.25, 0.0, 1.0, 0.0])
    eps = np.array([1e-6, 1e-3, 1e-6, 1e-9, 1.0])
    b = np.array([0.05, 1.0, 0.3, 1e-3, 0.5])
    zi = np.linspace(0.1, 0.9, M)
    y, zf = R.pcen(S, gain=gain, bias=bias, power=power, eps=eps, b=b, zi=zi, return_zf=True)
    for m in range(M):
        ym, zm = R.pcen(S[m:m + 1], gain=gain[m], bias=bias[m], power=power[m], eps=eps[m], b=b[m], zi=zi[m:m + 1], return_zf=True)
        assert np.array_equal(y[m], ym[0]) and zf[m] == zm[0]
    # one vector among scalars
    y = R.pcen(S, b=b)
    for m in range(M):
        assert np.array_equal(y[m], R.pcen(S[m:m + 1], b=b[m])[0])
    # the table's cases are decided per band
    vals, per_band = PC.check_params(M, gain, bias, power, eps, b)
    tab = PC.pack_table(vals, 1024)
    assert per_band and tab.shape == (M, PC.TABLE_WORDS) and list(tab[:, 7]) == [0, 2, 1, 0, 1]
    assert close(tab[:, 1], (1 - b) ** 1024) and close(tab[:, 6], bias ** power) and np.array_equal(tab[:, 0], b)
    assert PC.check_params(M, 0.98, 2, 0.5, 1e-6, 0.05) == ([0.98, 2.0, 0.5, 1e-6, 0.05], False)


@pytest.mark.parametrize("piece", [1, 7, 64, 1000])
def test_pieces_chained_by_zf_equal_the_whole(piece):
    S = spec(4, 1500, seed=piece)
    for ms in (1, 3):
        whole, zf_whole = R.pcen(S, max_size=ms, return_zf=True)
        zi, parts = None, []
        for t0 in range(0, S.shape[1], piece):
            y, zi = R.pcen(S[:, t0:t0 + piece], max_size=ms, zi=zi, return_zf=True)
            parts.append(y)
        assert close(np.concatenate(parts, axis=1), whole) and close(zi, zf_whole)


def test_scale_is_a_factor_on_S():
    S = spec()
    assert np.array_equal(R.pcen(S, scale=2.0 ** 31), R.pcen(S * 2.0 ** 31))


def test_against_librosa():
    librosa = pytest.importorskip("librosa")
    S = spec(8, 100, seed=5)
    for kw in ({}, {"max_size": 3}, {"power": 0.0}, {"bias": 0.0}, {"b": 0.2, "gain": 0.5}):
        assert np.allclose(R.pcen(S, **kw), librosa.pcen(S, **kw), rtol=1e-10, atol=1e-12)
    y, zf = librosa.pcen(S, return_zf=True)
    y2, zf2 = R.pcen(S, return_zf=True)
    assert np.allclose(zf[..., 0], zf2, rtol=1e-12)
