"""The float64 restatement of the tonal features (tests/chroma_ref.py) pinned by construction: properties that follow
from librosa's definitions and need no librosa.  The package's own host tables (sygnals_amd/_chroma.py) are held to the
restatement here too, so the device tests compare kernels, not tables."""
import warnings

import numpy as np
import pytest
import scipy.ndimage
import scipy.signal

from tests import chroma_ref as R


def test_filters_chroma_column_norms_are_the_octave_weight():
    sr, n_fft, nc = 22050, 2048, 12
    w = R.filters_chroma(sr, n_fft, dtype=np.float64)
    assert w.shape == (12, 1025)
    fr = np.linspace(0, sr, n_fft, endpoint=False)[1:]
    fb = nc * R.hz_to_octs(fr, 0.0, nc)
    fb = np.concatenate(([fb[0] - 1.5 * nc], fb))[:1025]
    octw = np.exp(-0.5 * ((fb / nc - 5.0) / 2) ** 2)
    assert np.allclose(np.sqrt((w ** 2).sum(axis=0)), octw, rtol=1e-12, atol=0)
    flat = R.filters_chroma(sr, n_fft, octwidth=None, dtype=np.float64)
    assert np.allclose(np.sqrt((flat ** 2).sum(axis=0)), 1.0, rtol=1e-12, atol=0)
    assert (w >= 0).all() and R.filters_chroma(sr, n_fft).dtype == np.float32


def test_filters_chroma_a440_row():
    sr, n_fft = 22050, 2048
    k = int(round(440.0 * n_fft / sr))
    assert k == 41
    assert int(np.argmax(R.filters_chroma(sr, n_fft)[:, k])) == 9
    assert int(np.argmax(R.filters_chroma(sr, n_fft, base_c=False)[:, k])) == 0


def test_half_bin_tuning_is_the_odd_rows_of_the_24_table():
    """A tuning of +0.5 bins with 12 rows centres row c where the 24-row table centres row 2 c + 1: the wrapped distances D
    of the two tables satisfy D24 = 2 D12 there, which the un-normalised Gaussians show at equal widths."""
    sr, n_fft = 22050, 4096
    fr = np.linspace(0, sr, n_fft, endpoint=False)[1:]
    f12 = 12 * R.hz_to_octs(fr, 0.5, 12)
    f24 = 24 * R.hz_to_octs(fr, 0.0, 24)
    for c in range(12):
        d12 = np.remainder(f12 - c + 6 + 120, 12) - 6
        d24 = np.remainder(f24 - (2 * c + 1) + 12 + 240, 24) - 12
        assert np.allclose(d24, 2 * d12, atol=1e-9)
    a = R.filters_chroma(sr, n_fft, n_chroma=12, tuning=0.5, base_c=False, dtype=np.float64)
    b = R.filters_chroma(sr, n_fft, n_chroma=24, tuning=0.0, base_c=False, dtype=np.float64)
    ks = np.arange(200, 2000)
    ra, rb = np.argmax(a[:, ks], axis=0), np.argmax(b[:, ks], axis=0)
    odd = rb % 2 == 1
    assert odd.sum() > 500 and (ra[odd] == (rb[odd] - 1) // 2).all()       # nearest row 2 c + 1 of 24 <=> nearest row c of 12


def test_cq_to_chroma_shapes():
    eye = R.cq_to_chroma(84, 12, 12, dtype=np.float64)
    assert (eye == np.tile(np.eye(12), 7)).all()
    w = R.cq_to_chroma(252, 36, 12, dtype=np.float64)
    assert set(np.unique(w)) == {0.0, 1.0} and (w.sum(axis=0) == 1).all()
    for c in range(12):
        for o in range(7):
            cols = np.nonzero(w[c, 36 * o:36 * (o + 1)])[0]
            want = (np.array([-1, 0, 1]) + 3 * c) % 36            # centred on the semitone's own bin 3 c
            assert sorted(cols) == sorted(want)
    a1 = 440.0 * 2.0 ** ((33 - 69) / 12.0)
    assert (R.cq_to_chroma(84, 12, 12, fmin=a1, dtype=np.float64) == np.roll(eye, 9, axis=0)).all()
    assert (R.cq_to_chroma(84, 12, 12, fmin=a1, base_c=False, dtype=np.float64) == eye).all()
    part = R.cq_to_chroma(253, 36, 12, dtype=np.float64)
    assert part.shape == (12, 253) and (part[:, :252] == w).all() and (part[:, 252] == w[:, 0]).all()
    with pytest.raises(ValueError, match="integer multiple"):
        R.cq_to_chroma(84, 36, 24)
    win = np.array([0.25, 0.5, 0.25])
    sm = R.cq_to_chroma(84, 12, 12, window=win)
    assert np.allclose(sm, scipy.signal.convolve(eye, win[None, :], mode="same"))


def test_normalize_rules():
    x = np.array([[3.0, 0.0, 1e-39], [-4.0, 0.0, 1e-39]])
    assert np.allclose(R.normalize(x, np.inf, axis=0)[:, 0], [0.75, -1.0])
    assert np.allclose(R.normalize(x, 1, axis=0)[:, 0], [3 / 7, -4 / 7])
    assert np.allclose(R.normalize(x, 2, axis=0)[:, 0], [0.6, -0.8])
    for n in (np.inf, 1, 2):
        y = R.normalize(x, n, axis=0)
        assert (y[:, 1] == 0).all() and (y[:, 2] == 1e-39).all()             # below tiny: left as it is
    assert R.normalize(x, None) is not None and (R.normalize(x, None) == x).all()


def test_tonnetz_of_a_pitch_class_and_of_a_fifth():
    phi = R.tonnetz_phi(12)
    for c in range(12):
        ch = np.zeros((12, 3))
        ch[c] = 2.5
        assert np.allclose(R.tonnetz(ch), phi[:, [c]] * np.ones((1, 3)))
    # closed form: phi[0, c] = sin(7 pi c / 6), phi[1, c] = cos(7 pi c / 6): the pair is the unit vector at angle 7 pi c / 6 from
    # the second axis, so a shift by a fifth (7 semitones) turns it by 7 pi / 6 * 7 = 49 pi / 6 = pi / 6 (mod 2 pi)
    c = np.arange(12)
    assert np.allclose(phi[0], np.sin(7 * np.pi * c / 6)) and np.allclose(phi[1], np.cos(7 * np.pi * c / 6))
    assert np.allclose(phi[2], np.sin(3 * np.pi * c / 2)) and np.allclose(phi[4], 0.5 * np.sin(2 * np.pi * c / 3))
    rng = np.random.default_rng(3)
    ch = rng.uniform(0.1, 1.0, (12, 5))
    t0, t1 = R.tonnetz(ch), R.tonnetz(np.roll(ch, 7, axis=0))
    th = np.pi / 6
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])     # (sin, cos) pairs turn clockwise in this basis
    assert np.allclose(t1[:2], rot @ t0[:2])


@pytest.mark.parametrize("cents", [-37, 0, 12, 49])
def test_pitch_tuning_of_detuned_equal_temperament(cents):
    midi = np.arange(48, 84)
    f = 440.0 * 2.0 ** ((midi - 69) / 12.0) * 2.0 ** (cents / 1200.0)
    edges = np.linspace(-0.5, 0.5, 101)
    got = R.pitch_tuning(f, 0.01, 12)
    # the edge containing cents / 100; a residual that sits on an edge up to rounding may fall in either neighbour
    k = int(np.floor((cents / 100.0 + 0.5) / 0.01 + 1e-9))
    assert got in (edges[k], edges[max(k - 1, 0)]) and abs(got - cents / 100.0) <= 0.01 + 1e-12


def test_pitch_tuning_inside_a_bin_is_exact():
    """12.5 and -36.5 cents lie strictly inside a bin, half a bin from either edge: the answer is that bin's left edge alone."""
    f = 440.0 * 2.0 ** ((np.arange(48, 84) - 69) / 12.0)
    edges = np.linspace(-0.5, 0.5, 101)
    assert R.pitch_tuning(f * 2.0 ** (12.5 / 1200.0), 0.01, 12) == edges[62]              # [0.12, 0.13)
    assert R.pitch_tuning(f * 2.0 ** (-36.5 / 1200.0), 0.01, 12) == edges[13]             # [-0.37, -0.36)
    assert R.pitch_tuning(f * 2.0 ** (12.5 / 1200.0), 0.05, 12) == np.linspace(-0.5, 0.5, 21)[12]      # [0.10, 0.15)
    assert R.pitch_tuning(f * 2.0 ** (12.5 / 3600.0), 0.01, 36) == edges[62]              # the same residual at 36 bins an octave


def test_pitch_tuning_empty_warns():
    with pytest.warns(UserWarning, match="empty frequency set"):
        assert R.pitch_tuning(np.array([0.0, -1.0])) == 0.0


def test_piptrack_recovers_a_parabola():
    sr, n_fft, F = 22050, 2048, 1025
    k = np.arange(F, dtype=np.float64)
    for v in (100.3, 57.75, 300.5 - 1e-3):
        S = np.maximum(5.0 - 0.01 * (k - v) ** 2, 0.0)[:, None]
        p, m = R.piptrack(S, sr, n_fft)
        (kk,), = [np.nonzero(p[:, 0])]
        assert len(kk) == 1 and kk[0] == int(np.round(v))
        assert abs(p[kk[0], 0] - v * sr / n_fft) < 1e-9
        assert abs(m[kk[0], 0] - 5.0) < 1e-9                                  # the vertex value
    out = np.maximum(5.0 - 0.01 * (k - 5.2) ** 2, 0.0)[:, None]               # below fmin = 150 Hz (bin 13.9)
    assert not R.piptrack(out, sr, n_fft)[0].any()


def test_estimate_tuning_no_peak_and_median():
    with pytest.warns(UserWarning, match="empty frequency set"):
        assert R.estimate_tuning(np.zeros((1025, 3)), 22050) == 0.0
    k = np.arange(1025, dtype=np.float64)
    S = np.zeros((1025, 1))
    for v, h in ((100.0, 5.0), (200.0, 4.0), (301.0, 3.0)):
        S[:, 0] += np.maximum(h - 0.5 * (k - v) ** 2, 0.0)
    d = {}
    R.estimate_tuning(S, 22050, detail=d)
    assert d["n_peaks"] == 3 and d["threshold"] == 4.0 and d["counts"].sum() == 2     # the median itself stays


def test_cens_of_a_constant_chroma_is_constant_inside():
    ch = np.tile(np.array([8, 4, 2, 1, 0.5, 0.2, 0, 0, 3, 0, 0, 1.0])[:, None], (1, 200))
    for wl in (None, 1, 2, 41, 42):
        c = R.cens_from_chroma(ch, win_len_smooth=wl)
        h = 0 if not wl else wl + 2
        inner = c[:, h:200 - h]
        assert np.allclose(inner, inner[:, :1]) and np.allclose(np.sqrt((c ** 2).sum(axis=0)), 1.0)
        q = np.array([1, 0.75, 0.5, 0.25, 0, 0, 0, 0, 0.5, 0, 0, 0.25])      # 8 / 19.7 = 0.406, 4 / 19.7 = 0.203, ...
        assert np.allclose(inner[:, 0], q / np.linalg.norm(q))


def test_package_tables_match_the_restatement():
    from sygnals_amd import _chroma as CH
    for kw in ({}, {"tuning": 0.23}, {"n_chroma": 24}, {"octwidth": None}, {"base_c": False}, {"ctroct": 4.0, "octwidth": 1.5}):
        for sr, n_fft in ((22050, 2048), (16000, 1000), (8000, 2)):
            assert np.array_equal(CH.chroma_filterbank(sr, n_fft, **kw), R.filters_chroma(sr, n_fft, **kw))
    a1 = 440.0 * 2.0 ** ((33 - 69) / 12.0)
    for args in ((84, 12, 12), (252, 36, 12), (253, 36, 12), (72, 36, 36), (60, 24, 12)):
        for fmin in (None, a1):
            assert np.array_equal(CH.cq_to_chroma(*args, fmin=fmin), R.cq_to_chroma(*args, fmin=fmin))
    win = np.array([0.25, 0.5, 0.25])
    assert np.array_equal(CH.cq_to_chroma(84, 12, 12, window=win), R.cq_to_chroma(84, 12, 12, window=win).astype(np.float32))
    for nc in (1, 12, 24, 36):
        assert np.array_equal(CH.tonnetz_phi(nc), R.tonnetz_phi(nc).astype(np.float32))
    assert np.array_equal(CH.tuning_bins(0.05), R.tuning_edges(0.05)) and CH.check_resolution(0.01, "t") == 100
    rng = np.random.default_rng(0)
    q = rng.integers(0, 5, (3, 50)) * 0.25
    for wl in (1, 2, 41, 42, 255):
        for name in ("hann", "boxcar", "triang"):
            taps, left = CH.cens_window(wl, name)
            win = scipy.signal.get_window(name, wl + 2, fftbins=False)
            want = scipy.ndimage.convolve(q, (win / win.sum())[None, :], mode="constant")
            qp = np.pad(q, ((0, 0), (left, len(taps) - 1 - left)))
            got = np.stack([np.convolve(r, taps.astype(np.float64)[::-1], mode="valid") for r in qp])
            assert got.shape == want.shape and np.abs(got - want).max() < 1e-7
    assert CH.cens_window(None)[1] == 0 and CH.cens_window(None)[0].tolist() == [1.0]
    assert CH.pip_bins(22050, 2048) == (14, 372) and CH.pip_bins(22050, 2048, 0.0, 1e9) == (0, 1024)
    f = 440.0 * 2.0 ** ((np.arange(48, 84) - 69) / 12.0) * 2.0 ** (12 / 1200.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert CH.pitch_tuning(f) == R.pitch_tuning(f)
