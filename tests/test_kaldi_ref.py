"""tests/kaldi_ref.py, the float64 contract of the Kaldi front end, pinned by construction: known answers of every stage,
and the condition of every gated GPU case (tests/kaldi_cases.py) asserted here on the CPU."""
import math

import numpy as np
import pytest

from sygnals_amd import _kaldi as KD
from tests import kaldi_cases as KC
from tests import kaldi_ref as KR


def test_mel_scale_and_sizes():
    assert KR.mel(1000.0) == pytest.approx(1127.0 * math.log(17.0 / 7.0), rel=1e-15)
    assert float(KD.mel_scale(1000.0)) == pytest.approx(1127.0 * math.log(17.0 / 7.0), rel=1e-15)
    for name, (sr, fl, fs) in KC.SIZES.items():
        assert KD.sizes(sr, fl, fs) == KC.EXPECTED_SIZES[name]
    assert KD.EPS == 1.1920928955078125e-07 and np.float32(KD.LOG_EPS) == np.float32(math.log(KD.EPS))


@pytest.mark.parametrize("M,N,sr,low,high", [(23, 512, 16000.0, 20.0, 0.0), (80, 512, 16000.0, 20.0, -400.0),
                                              (128, 2048, 48000.0, 0.0, 0.0), (40, 256, 8000.0, 100.0, 3800.0)])
def test_mel_triangles(M, N, sr, low, high):
    w = KR.mel_banks(M, N, sr, low, high)
    assert w.shape == (M, N // 2) and w.min() >= 0.0 and w.max() <= 1.0
    hi = high + sr / 2 if high <= 0 else high
    ml, mh = KR.mel(low), KR.mel(hi)
    delta = (mh - ml) / (M + 1)
    mk = KR.mel(np.arange(N // 2) * sr / N)
    inside = (mk >= ml + delta) & (mk <= mh - delta)                # between the first and the last centre
    assert inside.sum() > 0
    np.testing.assert_allclose(w.sum(axis=0)[inside], 1.0, rtol=0, atol=1e-12)
    # the Nyquist bin has no column; a matrix one column wider would hold the weight the contract drops
    assert w.shape[1] == N // 2
    if high <= 0 and hi == sr / 2:
        assert abs(KR.mel(sr / 2) - mh) < 1e-9                     # the last triangle ends at Nyquist: weight 0 there anyway


def test_windows():
    for wl in (200, 400, 551):
        hann = KR.window("hanning", wl)
        assert abs(hann[0]) < 1e-15 and abs(hann[-1]) < 1e-15
        assert KR.window("hamming", wl)[0] == pytest.approx(0.08) and KR.window("hamming", wl)[-1] == pytest.approx(0.08)
        np.testing.assert_allclose(KR.window("povey", wl), hann ** 0.85, rtol=0, atol=0)
        assert np.all(KR.window("rectangular", wl) == 1.0)
        b = KR.window("blackman", wl, 0.42)
        assert abs(b[0]) < 1e-15 and b[(wl - 1) // 2] == pytest.approx(1.0, abs=1e-3)    # (an even wl has no centre sample)
        for name in KD.WINDOWS:
            w = KR.window(name, wl)
            np.testing.assert_allclose(w, w[::-1], rtol=0, atol=1e-13)
            assert w.max() <= 1.0 + 1e-15


def test_frame_counts():
    for L, T in ((399, 0), (400, 1), (559, 1), (560, 2)):
        assert KD.num_frames(L, 400, 160, True) == T and KR.frames(np.zeros(L), 400, 160, True).shape == (T, 400)
    for L, T in ((79, 0), (80, 1)):
        assert KD.num_frames(L, 400, 160, False) == T and KR.frames(np.ones(L), 400, 160, False).shape == (T, 400)
    for T in (0, 1, 2, 15, 16, 17, 33):
        for snip in (True, False):
            for wl, hop in ((400, 160), (200, 80), (551, 220), (1200, 480)):
                L = KC.length_for(T, wl, hop, snip)
                assert L >= 1 and KD.num_frames(L, wl, hop, snip) == T
                if T:
                    assert KD.num_frames(L - 1, wl, hop, snip) == T - 1


def test_reflect_rule():
    g = np.random.default_rng(1)
    wl, hop = 400, 160
    for L in (500, 801, 1500):                                       # L exceeds the pad: symmetric padding is defined
        x = g.standard_normal(L)
        fr = KR.frames(x, wl, hop, False)
        pad = wl // 2 - hop // 2
        xp = np.pad(x, (pad, wl), mode="symmetric")
        for t in range(fr.shape[0]):
            np.testing.assert_array_equal(fr[t], xp[t * hop:t * hop + wl])
    fr = KR.frames(np.array([0.25]), 400, 1, False)                    # L = 1: every index reflects onto the one sample
    assert fr.shape == (1, 400) and np.all(fr == 0.25)
    assert np.isfinite(KR.fbank(np.array([0.25]), 16000.0, frame_shift=0.0625, snip_edges=False)).all()
    for L in (1, 2, 7):
        s = np.arange(-30, 40)
        assert [KR.reflect(int(v), L) for v in s] == list(KD.reflect_index(s, L))


def test_preemphasis_known_answers():
    ramp = np.arange(6, dtype=np.float64)[None, :]
    np.testing.assert_allclose(KR.preemphasis(ramp, 0.5), [[0.0, 1.0, 1.5, 2.0, 2.5, 3.0]])
    np.testing.assert_allclose(KR.preemphasis(np.full((1, 5), 2.0), 0.97), np.full((1, 5), 2.0 * 0.03), rtol=1e-15)
    np.testing.assert_array_equal(KR.preemphasis(ramp, 0.0), ramp)


@pytest.mark.parametrize("k,A", [(37, 0.5), (100, 3.0)])
def test_bin_centred_cosine(k, A):
    sr, N = 16000.0, 512
    x = A * np.cos(2 * np.pi * k * np.arange(N) / N)
    E, _ = KR.mel_energies(x, sr, num_mel_bins=23, frame_length=32.0, window_type="rectangular", remove_dc_offset=False,
                           preemphasis_coefficient=0.0)
    basis = KR.mel_banks(23, N, sr)
    np.testing.assert_allclose(E[0], basis[:, k] * (A * N / 2) ** 2, rtol=1e-10, atol=1e-9)
    assert E[0].max() > 0


def test_dct_and_lifter():
    d = KR.dct_matrix(23, 23)
    np.testing.assert_allclose(d @ d.T, np.eye(23), atol=1e-13)
    np.testing.assert_allclose(KR.dct_matrix(13, 23), d[:13])
    Q = 22.0
    lf = KR.lifter(13, Q)
    assert lf[0] == 1.0 and lf[11] == pytest.approx(1.0 + 0.5 * Q)          # i = Q / 2: sin(pi / 2)
    assert np.all(KR.lifter(13, 0.0) == 1.0)


def test_column_orders_and_subtract_mean():
    x = np.random.default_rng(3).standard_normal(1200)
    base = KR.fbank(x, 16000.0)
    E, e = KR.mel_energies(x, 16000.0)
    np.testing.assert_allclose(base, np.log(np.maximum(E, KR.EPS)))
    first = KR.fbank(x, 16000.0, use_energy=True, energy_floor=0.0)
    last = KR.fbank(x, 16000.0, use_energy=True, energy_floor=0.0, htk_compat=True)
    np.testing.assert_array_equal(first[:, 1:], base)
    np.testing.assert_array_equal(last[:, :-1], base)
    np.testing.assert_array_equal(first[:, 0], last[:, -1])
    np.testing.assert_allclose(first[:, 0], e)
    floored = KR.fbank(1e-4 * x, 16000.0, use_energy=True, energy_floor=1.0)
    assert np.all(floored[:, 0] == 0.0)                                     # log(1): the floor is active
    c = KR.mfcc(x, 16000.0)
    ce = KR.mfcc(x, 16000.0, use_energy=True, energy_floor=0.0)
    ch = KR.mfcc(x, 16000.0, use_energy=True, energy_floor=0.0, htk_compat=True)
    np.testing.assert_array_equal(ce[:, 1:], c[:, 1:])
    np.testing.assert_allclose(ce[:, 0], e)
    np.testing.assert_array_equal(ch[:, :-1], ce[:, 1:])
    np.testing.assert_array_equal(ch[:, -1], ce[:, 0])
    np.testing.assert_allclose(c, KR.cepstra(base, 13, 22.0))
    for f in (KR.fbank(x, 16000.0, subtract_mean=True), KR.mfcc(x, 16000.0, subtract_mean=True)):
        assert np.max(np.abs(f.mean(axis=0))) < 1e-12
    assert KR.fbank(x[:399], 16000.0).shape == (0, 23) and KR.mfcc(x, 16000.0, min_duration=1.0).shape == (0, 13)
    for bad in (dict(round_to_power_of_two=False), dict(vtln_warp=1.1)):
        with pytest.raises(ValueError):
            KR.fbank(x, 16000.0, **bad)


def test_host_tables_equal_the_restatement():
    for wl in (200, 400, 551, 1200):
        for name in KD.WINDOWS:
            np.testing.assert_allclose(KD.window(name, wl), KR.window(name, wl), rtol=0, atol=1e-15)
    np.testing.assert_allclose(KD.window("blackman", 400, 0.3), KR.window("blackman", 400, 0.3), rtol=0, atol=1e-15)
    for M, N, sr, low, high in ((23, 512, 16000.0, 20.0, 8000.0), (80, 1024, 22050.0, 20.0, 11025.0), (256, 2048, 48000.0, 0.0, 24000.0),
                                (3, 256, 8000.0, 300.0, 3600.0)):
        ref = KR.mel_banks(M, N, sr, low, high)
        np.testing.assert_allclose(KD.mel_banks(M, N, sr, low, high), ref, rtol=0, atol=1e-12)
        bp = KD.mel_padded_f32(M, N, sr, low, high)
        assert bp.dtype == np.float32 and bp.shape == (-(-M // 16) * 16, N // 2) and not bp[M:].any()
        np.testing.assert_array_equal(bp[:M], KD.mel_banks(M, N, sr, low, high).astype(np.float32))     # rounded once
    for nc, M, Q in ((13, 23, 22.0), (20, 80, 0.0), (40, 40, 22.0)):
        np.testing.assert_allclose(KD.dct_lifter(nc, M, Q), KR.dct_matrix(nc, M) * KR.lifter(nc, Q)[:, None], rtol=0, atol=1e-14)
    tw = KD.twiddle_f32(512)
    k = np.arange(512)
    np.testing.assert_array_equal(tw[:512, 0], np.cos(2 * np.pi * k / 512).astype(np.float32))
    np.testing.assert_array_equal(tw[512:, 1], (-np.sin(2 * np.pi * np.arange(256) / 256)).astype(np.float32))
    assert list(KD.cep_columns(4, False)) == [0, 1, 2, 3] and list(KD.cep_columns(4, True)) == [3, 0, 1, 2]


CASES = KC.cases()


def test_cases_cover_the_issue():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    got = {KD.sizes(c["sr"], c["kw"]["frame_length"], c["kw"]["frame_shift"]) for c in CASES}
    assert set(KC.EXPECTED_SIZES.values()) <= got
    for snip in (True, False):
        Ts = {KD.num_frames(c["L"], *KD.sizes(c["sr"], c["kw"]["frame_length"], c["kw"]["frame_shift"])[:2], snip)
              for c in CASES if c["kw"]["snip_edges"] == snip}
        assert {1, 2, 15, 16, 17, 33} <= Ts
    assert {c["B"] for c in CASES} >= {1, 3, 33}
    assert {c["kw"].get("num_mel_bins", 23) for c in CASES} >= {3, 16, 17, 23, 80, 128, 256}
    assert {c["kw"].get("window_type", "povey") for c in CASES} == set(KD.WINDOWS)
    assert {c["amp"] for c in CASES} >= {1e-3, 1.0, 32768.0} and any(c["kind"] == "dc" for c in CASES)
    assert {c["layout"] for c in CASES} == {"ct", "tc"} and any(c["strided"] for c in CASES)
    assert {(c["L"], c["kw"]["snip_edges"]) for c in CASES} >= {(1, False), (80, False), (399, False)}


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_condition_of_gated_case(c):
    """Every frame of every energy-gated case has max_m E_ref > 1e6 eps, and so at least one dominant cell."""
    x = KC.case_input(c)
    assert x.dtype == np.float32 and x.shape == (c["B"], c["L"])
    E, _, f = KC.reference(c, x[:3])
    assert E.shape[1] >= 1 and np.isfinite(f).all()
    assert E.max(axis=-1).min() > KC.SCALE_MIN, (c["id"], E.max(axis=-1).min())
    e_err, l_err, n_dom = KC.gates(f[..., KC.mel_columns(c)], E, c["kw"].get("use_log_fbank", True))
    assert e_err < 1e-12 and l_err < 1e-12 and n_dom >= 1          # the contract passes its own gates


def test_condition_of_weak_band_and_impulse_cases():
    for M in (23, 80):
        fc = KC.band_centres(M, 16000.0)
        basis = KR.mel_banks(M, 512, 16000.0)
        assert np.all(np.diff(fc) > 0) and fc[0] > 20.0 and fc[-1] < 8000.0
        n = np.arange(560)
        for m in (0, M // 2, M - 1):
            E, _ = KR.mel_energies(np.cos(2 * np.pi * fc[m] * n / 16000.0).astype(np.float32), 16000.0, num_mel_bins=M)
            assert E.max(axis=1).min() > KC.SCALE_MIN
            assert np.all(E[:, m] >= KC.DOMINANT * E.max(axis=1))           # the band takes its turn among the dominant cells
        assert basis.sum(axis=1).min() > KC.SCALE_MIN                        # an impulse frame: E[m] = sum_k basis[m, k]
    x = np.zeros(400)
    x[7] = 1.0
    E, _ = KR.mel_energies(x, 16000.0, window_type="rectangular", remove_dc_offset=False, preemphasis_coefficient=0.0)
    np.testing.assert_allclose(E[0], KR.mel_banks(23, 512, 16000.0).sum(axis=1), rtol=1e-12)
