"""The float64 effects restatement (tests/effects_ref.py) against the reference's recorded output
(tests/golden/ref_effects.npz, written by tests/golden/make_golden_effects.py) and against its own definition."""
import os

import numpy as np
import pytest

from tests import effects_ref as R
from tests import hpss_ref as H

TOL = 1e-12                       # float64 against float64, of the peak


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_effects.npz"))


def close(a, b, what):
    assert a.shape == b.shape, what
    pk = max(np.max(np.abs(b)), 1e-300)
    assert np.max(np.abs(a - b)) <= TOL * pk, f"{what}: {np.max(np.abs(a - b)) / pk:.2e}"


def test_delay(g):
    y, sr = g["y"], int(g["sr"])
    for i, (dt, fb, wet, dry) in enumerate(g["delay_params"]):
        close(R.apply_delay(y, sr, dt, fb, wet, dry), g[f"delay_{i}"], f"delay {i}")
    assert R.delay_samples(g["delay_params"][2][0], sr) == 1 and R.delay_samples(g["delay_params"][5][0], sr) > len(y)


def test_delay_definition():
    """The per-residue lfilter form against the recurrence written out."""
    rng = np.random.default_rng(5)
    y = rng.standard_normal(300)
    for D in (1, 7, 299, 300, 305):
        w = np.zeros(300)
        out = np.zeros(300)
        for n in range(300):
            wd = w[n - D] if n >= D else 0.0
            out[n] = 0.9 * y[n] + 0.6 * wd
            w[n] = y[n] + 0.7 * wd
        close(R.delay_core(y, D, 0.7, 0.6, 0.9), out, f"D={D}")


def test_chorus_is_a_fixed_delay(g):
    """apply_chorus interpolates left of its grid: it is apply_delay with ceil((delay + depth) sr) + 2 samples, whatever
    the LFO's rate and shape."""
    y, sr = g["y"][:3000], int(g["sr"])
    for i, (rate, depth, delay, fb, wet, dry) in enumerate(g["chorus_params"]):
        D = R.chorus_delay_samples(delay, depth, sr)
        close(R.delay_core(y, D, fb, wet, dry), g[f"chorus_{i}"], f"chorus {i}")


def test_tremolo(g):
    y, sr = g["y"][:2048], int(g["sr"])
    for shp in ("sine", "triangle", "square"):
        for i, (rate, depth) in enumerate(g["tremolo_params"]):
            close(R.apply_tremolo(y, 22050 if i == 0 else sr, rate, depth, shp), g[f"tremolo_{shp}_{i}"], f"{shp} {i}")


def test_compression(g):
    y = g["y"][:2048]
    for i, (thr, ratio) in enumerate(g["compress_params"]):
        out = R.compress(y, thr, ratio)
        close(out, g[f"compress_{i}"], f"compress {i}")
        below = np.abs(y) <= thr
        assert np.array_equal(out[below], y[below]) and np.array_equal(g[f"compress_{i}"][below], y[below])


def test_reverb(g):
    y, sr = g["y"], int(g["sr"])
    for i, (dec, wet, dry) in enumerate(g["reverb_params"]):
        ir = R.basic_ir(sr, dec, 7)
        assert np.array_equal(ir, g[f"reverb_ir_{i}"])                 # the same seed gives the reference's IR
        out = R.apply_reverb(y, sr, dec, wet, dry, 7)
        assert len(out) == len(y) + len(ir) - 1
        close(out, g[f"reverb_{i}"], f"reverb {i}")
    assert len(g["reverb_ir_0"]) == 1 and len(g["reverb_ir_1"]) == int(1.5 * sr * 0.01)


def test_gain_and_midside(g):
    for i, db in enumerate(g["gain_db"]):
        close(R.adjust_gain(g["y"][:2048], db), g[f"gain_{i}"], f"gain {i}")
    for i, wd in enumerate(g["width"]):
        close(R.midside(g["stereo"], wd), g[f"midside_{i}"], f"midside {i}")


def _noisy_tone(L=7680, sr=8000, seed=2):
    rng = np.random.default_rng(seed)
    y = 0.05 * rng.standard_normal(L)
    y[L // 2:] += 0.6 * np.sin(2 * np.pi * 440.0 * np.arange(L - L // 2) / sr)
    return y


def test_denoise_properties():
    y, sr = _noisy_tone(), 8000
    # nothing subtracted: the inverse of the forward transform
    out0 = R.noise_reduction_spectral(y, sr, 0.1, 0.0)
    assert np.max(np.abs(out0 - H.istft(H.stft(y), len(y)))) <= 1e-13 * np.max(np.abs(y))
    # the profile segment is the whole clip and the subtraction aggressive: every bin goes to zero
    n = 0.1 * np.random.default_rng(4).standard_normal(4000)
    outz = R.noise_reduction_spectral(n, sr, len(n) / sr, 1e6)
    assert np.max(np.abs(outz)) == 0.0
    # the gain is a mask in [0, 1], and applying it to D is what the reference's magnitude / phase form computes
    D = H.stft(y)
    N = R.noise_profile(H.stft(y[:800]))
    for a in (0.5, 1.0, 2.0):
        G = R.gate(np.abs(D) ** 2, N, a)
        assert G.min() >= 0.0 and G.max() <= 1.0
        out = R.noise_reduction_spectral(y, sr, 0.1, a)
        assert np.max(np.abs(H.istft(G * D, len(y)) - out)) <= 1e-13 * np.max(np.abs(y))
    assert np.array_equal(R.gate(np.zeros((3, 2)), np.zeros(3), 1.0), np.zeros((3, 2)))


def test_transient_shaping_identity():
    y = _noisy_tone(4096)
    assert np.max(np.abs(R.transient_shaping_hpss(y, 8000, 1.0) - y)) <= 1e-14
    yh, yp = H.hpss(y, 31, 2.0, (2.0, 3.0))
    assert np.array_equal(R.transient_shaping_hpss(y, 8000, 2.5, 2.0, 3.0), yh + 2.5 * yp)
