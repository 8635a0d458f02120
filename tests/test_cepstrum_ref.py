"""tests/cepstrum_ref.py is pinned by construction (no library on the test machines has a cepstrum): closed forms of the
real and complex cepstrum, the unwrap as integer counts against np.unwrap, the bin-0 rule, the round trip and the peak
picker's rules."""
import numpy as np
import pytest
import scipy.fft

from tests import cepstrum_cases as CS
from tests import cepstrum_ref as R

NS = (255, 256, 1000, 1024, 4096, 4099)


@pytest.mark.parametrize("n", (64, 255, 1000))
@pytest.mark.parametrize("d", (0, 1, 7, 31))
def test_scaled_impulse(n, d):
    a = 2.5
    x = np.zeros(n)
    x[d] = a
    c = R.real_cepstrum(x)
    assert abs(c[0] - np.log(a)) < 1e-12 and np.max(np.abs(c[1:])) < 1e-12
    cc, nd = R.complex_cepstrum(x)
    assert nd == -d
    if n % 2 == 0 or d == 0:                        # (an odd n leaves a residue of the ramp: the documented limit)
        assert abs(cc[0] - np.log(a)) < 1e-12 and np.max(np.abs(cc[1:])) < 1e-11


def test_echo_series():
    """x + alpha roll(x, d): the real cepstrum gains (-1)^(m+1) alpha^m / (2 m) at q = m d (and at n - m d), the even part of
    the series of log(1 + alpha e^(-i w d))."""
    n, d, alpha = 4096, 100, 0.6
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32).astype(np.float64)
    y = x + alpha * np.roll(x, d)
    assert np.min(np.abs(np.fft.fft(x))) > 1e-3 and np.min(np.abs(np.fft.fft(y))) > 1e-3      # the floor is not in play
    diff = np.fft.ifft(R.log_magnitude(np.fft.fft(y)) - R.log_magnitude(np.fft.fft(x))).real
    for m in (1, 2, 3):
        want = (-1) ** (m + 1) * alpha ** m / (2 * m)
        assert abs(diff[m * d] - want) < 1e-9 and abs(diff[n - m * d] - want) < 1e-9
    # and through the float32 rounding of y the cepstrum itself shows them
    c = R.real_cepstrum(y) - R.real_cepstrum(x)
    assert abs(c[d] - alpha / 2) < 1e-5 and abs(c[2 * d] + alpha ** 2 / 4) < 1e-5 and abs(c[3 * d] - alpha ** 3 / 6) < 1e-5


def test_complex_cepstrum_of_a_geometric_row():
    a, n = 0.9, 2048
    x = a ** np.arange(n)
    c, nd = R.complex_cepstrum(x)
    q = np.arange(1, 400)
    assert nd == 0 and abs(c[0]) < 1e-7
    assert np.max(np.abs(c[q] - a ** q / q)) < 1e-7             # (float32 rounding of the row: 6e-8 relative a sample)
    X = np.fft.fft(x)                                           # the float64 row: the series to 1e-12
    phi_u, ndelay, center = R.unwrapped_phase(X)
    c64 = np.fft.ifft(np.log(np.abs(X)) + 1j * phi_u).real
    assert ndelay == 0 and np.max(np.abs(c64[q] - a ** q / q)) < 1e-12


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", CS.COMPLEX_ROWS)
def test_unwrap_counts_equal_np_unwrap(kind, n):
    X = R.spectrum(CS.complex_row(kind, n))
    phi = R.phase(X)
    M = R.wrap_counts(phi)
    assert M[0] == 0 and set(np.unique(M)) <= {-1, 0, 1}
    assert np.max(np.abs(phi + 2 * np.pi * np.cumsum(M) - np.unwrap(phi))) < 1e-9
    # the conditions under which the device is gated on these rows hold on every one of them
    phi_u, ndelay, center = R.unwrapped_phase(X)
    assert R.unwrap_margin(phi) > 0.1 and abs(phi_u[center] / np.pi - ndelay) < 0.25


def test_unwrap_ties():
    phi = np.array([0.0, np.pi, 0.0, -np.pi, 0.0, 3.0, -3.0, 3.0])
    M = R.wrap_counts(phi)
    assert list(M) == [0, 0, 0, 0, 0, 0, 1, -1]
    assert np.max(np.abs(phi + 2 * np.pi * np.cumsum(M) - np.unwrap(phi))) < 1e-12


@pytest.mark.parametrize("n", (256, 1000))
def test_shift_gives_minus_ndelay(n):
    for kind, d in (("damped", 0), ("damped_shift7", 7), ("damped_shift_n8", n // 8), ("echo40", 0), ("three_taps", 1),
                    ("reversed", -1), ("negative", -1)):
        assert R.complex_cepstrum(CS.complex_row(kind, n))[1] == -d, kind


@pytest.mark.parametrize("n", (255, 256, 1000))
def test_bin0_rule_row_and_negation(n):
    """-x has every phase turned by pi: bin 0 counts as +pi whatever the sign of a zero imaginary part, ndelay grows by one,
    and c changes by the fixed sequence ifft(i pi (1 - k / center)).real."""
    for kind in ("damped", "echo40", "damped_shift7"):
        x = CS.complex_row(kind, n)
        c, nd = R.complex_cepstrum(x)
        cm, ndm = R.complex_cepstrum(-x)
        center = (n + 1) // 2
        assert ndm == nd + 1
        ramp = np.fft.ifft(1j * np.pi * (1 - np.arange(n) / center)).real
        assert np.max(np.abs(cm - c - ramp)) < 1e-10
    X = np.fft.fft(CS.complex_row("negative", n).astype(np.float64))
    for im in (0.0, -0.0):                                     # the sign of the zero decides nothing
        X[0] = complex(X[0].real, im)
        assert R.phase(X)[0] == np.pi


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", CS.COMPLEX_ROWS)
def test_round_trip(kind, n):
    """Exact for even n, and for odd n at ndelay = 0.  The sign of the row's sum is not held by (c, ndelay): a row of
    negative sum comes back as x - 2 mean(x), to the same precision."""
    x = CS.complex_row(kind, n).astype(np.float64)
    c, nd = R.complex_cepstrum(x)
    back = R.inverse_complex_cepstrum(c, nd)
    want = x if x.sum() >= 0 else x - 2 * x.mean()
    if n % 2 == 0 or nd == 0:
        assert np.max(np.abs(back - want)) < 1e-12
    else:
        assert np.max(np.abs(back - want)) > 1e-9               # the documented limit: not repaired


def test_real_cepstrum_equals_scipy():
    rng = np.random.default_rng(5)
    for n in (256, 1000, 4096):
        x = rng.standard_normal(n).astype(np.float32)
        want = scipy.fft.irfft(np.log(np.maximum(np.abs(scipy.fft.rfft(x.astype(np.float64))), R.AMIN)), n)
        assert np.max(np.abs(R.real_cepstrum(x) - want)) < 1e-13
    x = rng.standard_normal(300).astype(np.float32)
    for n in (200, 512):                                       # cut and zero-padded
        want = scipy.fft.irfft(np.log(np.maximum(np.abs(scipy.fft.rfft(x.astype(np.float64), n)), R.AMIN)), n)
        assert np.max(np.abs(R.real_cepstrum(x, n) - want)) < 1e-13


def test_cepstrogram_frames_and_zero_frame():
    y = CS.clip("noise", 6000)
    c, K = R.cepstrogram(y, 2048, 512, True, "hann", None, None)
    assert c.shape == (1025, 1 + 6000 // 512) and np.all(K >= 1.0)
    t = 5                                                       # an interior frame: rows 512 t - 1024 .. + 2048
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2048) / 2048)
    xw = y[512 * t - 1024:512 * t + 1024].astype(np.float64) * w.astype(np.float32)
    assert np.max(np.abs(c[:, t] - np.fft.ifft(R.log_magnitude(np.fft.fft(xw))).real[:1025])) < 1e-12
    c, K = R.cepstrogram(np.zeros(3000, dtype=np.float32), 2048, 512, True, np.ones(2048), None, 7)
    assert c.shape == (7, 6) and np.all(c[0] == np.log(R.AMIN)) and not c[1:].any() and np.all(K == 1.0)
    assert R.cepstrogram(y, 1000, 250, False)[0].shape == (501, 1 + (6000 - 1000) // 250)
    c, _ = R.cepstrogram(y, 2048, 512, True, "hann", 1024, 13)
    assert c.shape == (13, 12)
    with pytest.raises(ValueError):
        R.cepstrogram(y[:100], 2048, 512, False)


def test_peaks_rules():
    Q, T = 40, 6
    c = np.zeros((Q, T), dtype=np.float32)
    c[10:13, 0] = 0.5                                           # a plateau: the first of it, no shift (denominator 0)
    c[5, 1] = 0.9                                               # a peak at qmin: no shift
    c[30, 2] = 0.9                                              # a peak at qmax: no shift
    c[20, 3], c[19, 3], c[21, 3] = 0.8, 0.2, 0.6                # an interior peak leaning right
    c[20, 4] = 0.12                                             # under the threshold
    c[:, 5] = 0.0                                               # all equal: qmin
    f0, s, q, v = R.peaks(c, 5, 30, 22050.0)
    assert list(q) == [10, 5, 30, 20, 20, 5] and list(v) == [True, True, True, True, False, False]
    # the plateau's first point: c[9] = 0 < c[10] = c[11] gives a negative denominator and a shift to the right
    a, m, r = 0.0, 0.5, 0.5
    assert f0[0] == 22050.0 / (10 + 0.5 * (a - r) / (a - 2 * m + r))
    assert f0[1] == 22050.0 / 5 and f0[2] == 22050.0 / 30
    a, m, r = np.float64(np.float32(0.2)), np.float64(np.float32(0.8)), np.float64(np.float32(0.6))
    assert f0[3] == 22050.0 / (20 + 0.5 * (a - r) / (a - 2 * m + r)) and 20 < 22050.0 / f0[3] < 20.5
    assert np.isnan(f0[4]) and np.isnan(f0[5]) and s[4] == np.float32(0.12)
    assert R.quefrency_range(22050, 82, 1000, 2048) == (23, 268) and R.quefrency_range(22050, 10, 1000, 2048) == (23, 1023)
    for bad in ((22050, 500, 400, 2048), (22050, 5000, 6000, 8)):      # fmax under fmin; a frame too short for fmax
        with pytest.raises(ValueError):
            R.quefrency_range(*bad)
