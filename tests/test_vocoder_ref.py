"""Pins tests/vocoder_ref.py without librosa: what the phase vocoder must do by construction, its lengths, and that the
product-of-phasors form (the device's arithmetic) is the angle form."""
import numpy as np
import pytest

from tests import hpss_ref as R
from tests import vocoder_ref as V


def _noise_stft(T, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((1025, T)) + 1j * rng.standard_normal((1025, T))


def test_rate_one_returns_the_input():
    D = _noise_stft(23)
    out = V.phase_vocoder(D, 1.0)
    assert out.shape == D.shape
    # the angle form's accumulator reaches pi * hop * T rad at the top bin; cos / sin of it carry its rounding
    tol = 4 * np.finfo(np.float64).eps * np.pi * V.HOP * D.shape[1]
    assert np.max(np.abs(out - D)) <= tol * np.max(np.abs(D))


@pytest.mark.parametrize("k", [64, 65])
@pytest.mark.parametrize("rate", [0.5, 2.0])
def test_bin_centred_tone_stays_the_tone(rate, k):
    """A stationary tone at a bin centre advances every bin's phase by w * hop a frame (bin 64: a multiple of 2 pi, bin
    65: pi / 2), so resampling the frame axis gives the frames of the same tone: the stretched STFT is the tone's STFT at
    T' frames, and its inverse is the tone at its amplitude.  The clip's first and last frames see the zero padding and
    are no part of the stationary tone: the frames are those of the interior, continued to both ends."""
    T, amp, ph = 40, 0.7, 0.4
    w = 2 * np.pi * k / V.N_FFT
    col = R.stft(amp * np.cos(w * np.arange(16384) + ph))[:, 8]                   # an interior frame, centred on 8 * hop
    frames = lambda n: col[:, None] * np.exp(1j * w * V.HOP * (np.arange(n) - 8))[None, :]
    out = V.phase_vocoder(frames(T), rate)
    To = int(np.ceil(T / rate))
    assert out.shape == (1025, To)
    keep = To - int(np.ceil(1 / rate))                                            # the last step(s) read the zero padding
    assert np.max(np.abs(out[:, :keep] - frames(To)[:, :keep])) <= 1e-9 * np.max(np.abs(col))
    y = R.istft(out, V.HOP * (To - 1))                                            # the vocoder's output, inverted
    n = np.arange(2048, V.HOP * (To - 1) - 2048)
    assert np.max(np.abs(y[n] - amp * np.cos(w * n + ph))) <= 1e-9 * amp


@pytest.mark.parametrize("T,rate", [(1, 0.25), (7, 0.37), (65, 0.8), (65, 1.25), (65, 3.7), (5, 9.0), (129, 2.0)])
def test_output_frames(T, rate):
    assert V.phase_vocoder(_noise_stft(T), rate).shape[1] == int(np.ceil(T / rate))


def test_output_length_rounds_half_to_even():
    assert V.stretch_length(2049, 2.0) == 1024           # 1024.5 -> 1024
    assert V.stretch_length(2051, 2.0) == 1026           # 1025.5 -> 1026
    assert len(V.time_stretch(np.ones(2049), 2.0)) == 1024
    assert len(V.time_stretch(np.ones(8192), 0.8)) == 10240


def _cases():
    rng = np.random.default_rng(5)
    noise = R.stft(rng.standard_normal(40000))
    n = np.arange(40000)
    tones = R.stft(0.5 * np.sin(2 * np.pi * 0.0213 * n) + 0.2 * np.sin(2 * np.pi * 0.17 * n + 1.0))
    zero_frame = noise.copy()
    zero_frame[:, 17] = 0.0
    neg_zero = noise.copy()
    neg_zero[300, 9] = complex(-0.0, 0.0)
    return {"noise": noise, "tones": tones, "zero_frame": zero_frame, "neg_zero": neg_zero}


@pytest.mark.parametrize("name", ["noise", "tones", "zero_frame", "neg_zero"])
@pytest.mark.parametrize("rate", [0.37, 0.8, 1.25, 2.0])
def test_product_form_is_the_angle_form(name, rate):
    """np.angle(-0 + 0j) is pi, so the unit phasor of an all-zero element is (copysign(1, re), 0), not (1, 0): with
    (1, 0) the 'neg_zero' case is off by a sign in every later frame of that bin."""
    D = _cases()[name]
    a, p = V.phase_vocoder(D, rate), V.phase_vocoder_product(D, rate)
    assert np.max(np.abs(a - p)) <= 1e-8 * np.max(np.abs(a))
    if name == "neg_zero":
        u = V.unit(np.array([complex(-0.0, 0.0), complex(0.0, 0.0), complex(0.0, -0.0)]))
        assert np.array_equal(u.real, [-1.0, 1.0, 1.0]) and np.all(u.imag == 0)
        assert np.allclose(np.exp(1j * np.angle(np.array([complex(-0.0, 0.0)]))), [-1.0])


def test_add_noise_restatement_against_the_recorded_reference():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_augment.npz"))
    n = int(g["n_cases"])
    assert n >= 12
    for i in range(n):
        y, snr, seed, want = g[f"y_{i}"], float(g["snr_db"][i]), int(g["seed"][i]), g[f"out_{i}"]
        got = V.add_noise(y, snr, seed)
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300), i
        if g["silent"][i]:
            assert np.array_equal(want, y)
