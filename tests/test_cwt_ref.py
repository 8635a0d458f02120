"""tests/cwt_ref.py, the float64 restatement of pywt.cwt the device is held to, checked on its own: the central
frequencies PyWavelets documents, the identity the host plan rests on (the differenced filter of sygnals_amd/_cwt.py
against conv-then-diff), linearity, the response to a constant and to a tone, and pywt's refusal of a scale too small."""
import numpy as np
import pytest

from sygnals_amd import _cwt as CW
from tests import cwt_ref as R

WAVELETS = ("morl", "mexh", "gaus1", "cmor1.5-1.0")
SCALES = (1, 1.5, 2, 7.3, 64.5, 300)


def test_central_frequencies():
    for name, f in (("morl", 0.8125), ("mexh", 0.25), ("gaus1", 0.2), ("cmor1.5-1.0", 1.0), ("cmor2.0-0.5", 0.5)):
        assert R.central_frequency(name) == pytest.approx(f, abs=1e-12)
        assert CW.central_frequency(name) == R.central_frequency(name)
    s = np.array([1.0, 2.0, 8.0])
    assert np.allclose(CW.scale2frequency("morl", s), 0.8125 / s, rtol=0, atol=1e-15)
    assert np.array_equal(CW.scalogram_scales(64, 2048), np.geomspace(1.0, 256.0, 64))
    assert np.array_equal(CW.scalogram_scales(0, 4), np.geomspace(1.0, 2.0, 1))


@pytest.mark.parametrize("name", WAVELETS)
def test_differenced_filter_equals_conv_then_diff(name):
    """Filters longer than the row (L = 1, 2, 17 under up to 4802 taps) and scales where j is cut at 1024 (1, 1.5, 2)
    included.  Both the plan's filter and the restatement's own h_filter."""
    rng = np.random.default_rng(3)
    plan = CW.cwt_plan(SCALES, name)
    worst = 0.0
    for L in (1, 2, 17, 1000):
        x = rng.standard_normal(L)
        for i, s in enumerate(SCALES):
            ref = R.cwt_scale(x, name, s)
            A = plan.l1[i] * np.abs(x).max()
            for h, off in ((plan.table64[i], int(plan.offset[i])), R.h_filter(name, s)):
                got = np.convolve(x, h)[off + 1:off + 1 + L]
                assert got.shape == ref.shape == (L,)
                worst = max(worst, np.abs(got - ref).max() / A)
            assert np.array_equal(plan.table64[i], R.h_filter(name, s)[0]) and plan.offset[i] == R.h_filter(name, s)[1]
            assert plan.taps[i] == R.kernel(name, s).size + 1
    print(f"{name}: differenced against conv-then-diff, worst {worst:.2e} of A_s")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", WAVELETS)
def test_linear_and_blind_to_a_constant(name):
    rng = np.random.default_rng(5)
    scales = [1, 2, 7.3, 20]
    a, b = rng.standard_normal(400), rng.standard_normal(400)
    Wa, Wb, Wab = (R.cwt(v, scales, name)[0] for v in (a, b, 2.0 * a - 3.0 * b))
    assert np.abs(Wab - (2.0 * Wa - 3.0 * Wb)).max() <= 1e-12 * np.abs(Wab).max()
    Wc = R.cwt(np.full(1000, 0.75), scales, name)[0]
    plan = CW.cwt_plan(scales, name)
    for i in range(len(scales)):
        t = int(plan.taps[i])
        assert abs(plan.table64[i].sum()) <= 1e-12 * plan.l1[i]          # sum h = 0 by telescoping
        assert np.abs(Wc[i, t:1000 - t]).max() <= 1e-12 * plan.l1[i]
        assert np.abs(Wc[i, :t]).max() > 1e-3 * plan.l1[i]               # the edges do see the step


@pytest.mark.parametrize("name", WAVELETS)
def test_tone_peaks_at_its_scale(name):
    f = 0.02
    x = np.cos(2 * np.pi * f * np.arange(4096))
    grid = np.geomspace(2.0, 200.0, 25)
    W, freqs = R.cwt(x, grid, name, sampling_period=1.0 / 8000.0)
    assert np.allclose(freqs, R.central_frequency(name) / grid * 8000.0, rtol=1e-15)
    # the peak of |W| over the middle of the row (away from the edges) sits at the grid scale nearest central_frequency / f.
    # gaus1 is the exception, by arithmetic and not by tolerance: central_frequency is a bin of a 256-point transform over
    # a support of 10, i.e. a multiple of 0.1, and gaus1's spectrum w exp(-w^2 / 4) is broad.  With the sqrt(s) of step 3
    # the response to a tone goes as s^1.5 exp(-(2 pi f s)^2 / 4), which peaks at s = sqrt(3) / (2 pi f) = 0.2757 / f, not at
    # 0.2 / f.  (The same derivation gives sqrt(2.5) / (2 pi f) = 0.2516 / f for mexh, its documented 0.25.)
    peak = np.sqrt(3.0) / (2 * np.pi * f) if name == "gaus1" else R.central_frequency(name) / f
    got = int(np.argmax(np.abs(W[:, 1024:3072]).max(axis=1)))
    assert got == int(np.argmin(np.abs(np.log(grid) - np.log(peak))))


def test_scale_too_small_in_pywt_words():
    for fn in (lambda: R.cwt(np.zeros(8), [0.01], "morl"), lambda: CW.cwt_plan([4.0, 0.01], "morl"),
               lambda: R.h_filter("gaus1", 0.01)):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == "Selected scale of 0.01 too small."
    assert R.cwt(np.ones(8), [0.2], "morl")[0].shape == (1, 8)           # two samples of the kernel: d = 0, nothing cropped
