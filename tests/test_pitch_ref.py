"""KATs of the float64 yin / pyin restatement (tests/pitch_ref.py) and of the shared host tables (sygnals_amd/_pitch.py)."""
import math

import numpy as np
import pytest
from scipy.stats import beta

from sygnals_amd import _pitch as P
from tests import pitch_ref as R


def test_constants():
    assert P.periods(48000, P.C2, P.C7, 2048, 1024) == (22, 734)
    assert P.n_pitch_bins(P.C2, P.C7) == 601 and P.n_pitch_bins(75.0, 600.0) == 361
    assert P.transition_width(48000, 512) == 51 and P.transition_width(16000, 512) == 141
    assert P.transition_width(22050, 512) == 101
    assert P.cand_stride(713) == 358


@pytest.mark.parametrize("n,width", [(601, 51), (601, 101), (37, 101), (360, 51)])
def test_transition_rows(n, width):
    T = R.P.transition_local(n, width)
    assert np.allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    h = width // 2
    assert np.all(T[np.abs(np.subtract.outer(np.arange(n), np.arange(n))) > h] == 0)
    if n > width:                                     # edge rows are cut and renormalised: larger diagonal
        assert T[0, 0] > T[n // 2, n // 2] and T[n - 1, n - 1] > T[n // 2, n // 2]
        tabs, Rr, hh = P.transition_tables(n, width)
        assert Rr == 2 * h + 1 and tabs.shape == (2, Rr, 2 * h + 1)


@pytest.mark.parametrize("n,width", [(39, 141), (361, 551), (4, 5), (608, 611), (2, 31)])
def test_transition_wider_than_states(n, width):
    """width > n (a chosen behaviour, not pinned against librosa, which may reject it): the n centre entries of the
    triangle window are rolled onto each row and masked to |j - i| <= width // 2, so inside the band the row reads the
    window at the CIRCULAR offset (j - i) mod n; with width // 2 >= n - 1 nothing is masked."""
    from scipy.signal import get_window
    T = P.transition_local(n, width)
    h = width // 2
    m = (n - 1) // 2                                                    # the centre, as librosa's pad_center
    w = get_window("triangle", width, fftbins=False)[h - m:h - m + n]     # offsets -m .. n - 1 - m
    for i in range(n):
        j = np.arange(n)
        raw = np.where(np.abs(j - i) <= h, w[(j - i + m) % n], 0.0)
        np.testing.assert_allclose(T[i], raw / math.fsum(raw), rtol=1e-15, atol=0, err_msg=f"row {i}")
        assert np.argmax(T[i]) == i, f"row {i}: the peak is off the diagonal"
    if h >= n - 1:
        assert T[0, n - 1] == T[0, 1] > 0
    tabs, Rr, hh = P.transition_tables(n, width)
    assert Rr == n and hh == h


def test_beta_and_boltzmann():
    assert math.isclose(P.beta_probs().sum(), beta.cdf(1, 2, 18), rel_tol=0, abs_tol=1e-15)
    for n in (1, 2, 7, 50):
        assert math.isclose(P.boltzmann_pmf(np.arange(n), n).sum(), 1.0, abs_tol=1e-14)
    assert np.all(np.isfinite(P.boltzmann_pmf(np.arange(3), 0)))


def _tone(f, sr, secs=1.0):
    t = np.arange(int(sr * secs)) / sr
    return sum(0.5 / k * np.sin(2 * np.pi * k * f * t) for k in (1, 2, 3))


@pytest.mark.parametrize("f", [110.0, 220.0, 440.0, 880.0])
def test_harmonic_tone_within_one_bin(f):
    sr = 22050
    r = R.pyin(_tone(f, sr), sr)
    v = r["voiced"]
    assert v[2:-2].all()
    assert np.all(np.abs(120 * np.log2(r["f0"][2:-2] / f)) <= 1.0)


def test_silence_unvoiced():
    r = R.pyin(np.zeros(22050), 22050)
    assert not r["voiced"].any() and np.isnan(r["f0"]).all()


def test_duplicate_bin_and_top_bin_traps():
    sr, fmin, n = 48000, P.C2, 601
    min_p = 22
    # two troughs whose periods round to the same bin: the larger lag must win the bin
    c = np.ones(60)
    c[30], c[32] = 0.05, 0.04               # periods 52 and 54 + shifts 0
    c[29] = c[31] = c[33] = 0.5
    sh = np.zeros_like(c)
    fa, fb = sr / (min_p + 30), sr / (min_p + 32)
    ba, bb = (round(120 * math.log2(f / fmin)) for f in (fa, fb))
    assert ba != bb                         # not the same bin in general; force one with a shift
    sh[30] = (sr / fmin / 2 ** (bb / 120)) - (min_p + 30)   # the period of trough 30 moved onto bin bb
    assert abs(sh[30]) < 3
    b, p, vp = R.pyin_frame(c, sr, min_p, fmin, n, shift=sh)
    assert list(b) == [bb] and len(p) == 1
    full_b, full_p, _ = R.pyin_frame(c, sr, min_p, fmin, n, shift=np.zeros_like(c))
    assert p[0] == full_p[list(full_b).index(bb)]       # the value of the larger lag
    # a trough at the top bin (bin == n_bins) is dropped and does not count in voiced_prob
    c2 = np.ones(40)
    c2[0] = 0.01
    c2[1] = 0.5
    b2, p2, vp2 = R.pyin_frame(c2, sr, 10, 100.0, 5)
    assert n not in b2 and len(b2) == 0 and vp2 == 0.0


# besides the edge-rows + interior-pattern tables: R == n with width > n (39, 141), width == n, jitter's 75-600 Hz range at
# hop 2048 / 16 kHz (361, 551), h = 0 (601, 1: hop 32 / 48 kHz), a single pitch bin and an even n below the width
@pytest.mark.parametrize("n,width", [(40, 11), (61, 21), (25, 31), (39, 141), (51, 51), (1, 1), (1, 51), (361, 551),
                                     (601, 1), (40, 51)])
def test_band_viterbi_equals_dense(n, width):
    rng = np.random.default_rng(n + width)
    for _ in range(3):
        Tn = 30
        obs = np.zeros((2 * n, Tn))
        vps = rng.uniform(0, 1, Tn)
        for t in range(Tn):
            k = rng.integers(0, 4)
            bins = rng.choice(n, size=min(k, n), replace=False)
            obs[bins, t] = rng.uniform(0, 0.5, len(bins))
        obs[n:, :] = (1 - vps[None, :]) / n
        p_init = np.zeros(2 * n)
        p_init[n:] = 1 / n
        st_d, _ = R.viterbi_dense(obs, R.full_transition(n, width), p_init)
        st_b = R.viterbi_band(obs, n, width)
        assert np.array_equal(st_d, st_b)


def test_pyin_against_librosa_where_installed():
    librosa = pytest.importorskip("librosa")
    sr = 22050
    y = _tone(220.0, sr)
    f0, vf, vp = librosa.pyin(y, fmin=P.C2, fmax=P.C7, sr=sr, fill_na=np.nan)
    r = R.pyin(y, sr)
    assert np.mean(vf == r["voiced"]) >= 0.99
    both = vf & r["voiced"]
    assert np.all(np.abs(120 * np.log2(f0[both] / r["f0"][both])) <= 1.0)
    np.testing.assert_allclose(vp, r["voiced_prob"], atol=1e-6)
    np.testing.assert_allclose(librosa.yin(y, fmin=P.C2, fmax=P.C7, sr=sr),
                               R.yin_from_cmndf(R.cmndf(R.frames(y), 1024, *P.periods(sr, P.C2, P.C7, 2048, 1024)), sr,
                                                P.periods(sr, P.C2, P.C7, 2048, 1024)[0])[1], rtol=1e-6)
