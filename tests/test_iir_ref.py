"""The references and the host side of the causal IIR / FIR / EQ work, without a device: SciPy's float64 sosfilt against a
long-double sample loop on every design and input the GPU tests use; the designers against SciPy bit for bit; the EQ biquads
by construction."""
import os

import numpy as np
import pytest
from scipy import signal

from tests import iir_cases as IC

FS = IC.FS


@pytest.fixture(scope="module")
def consts():
    from sygnals_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ops.sosfilt_constants()


def test_scipy_reference_against_long_double(consts):
    """A condition on the reference, not a measurement: 1e-9 of the row's peak (y) and of the state's peak (zf).
    Observed: 6.3e-13 (y), 4.8e-11 (zf)."""
    worst_y = worst_z = 0.0
    for c in sum(IC.sweep_cases(consts).values(), []):
        x, zi = IC.make_input(c)
        ey, ez = IC.reference_error(IC.DESIGNS[c.design], x, zi)
        assert ey <= 1e-9 and ez <= 1e-9, (IC.case_id(c), ey, ez)
        worst_y, worst_z = max(worst_y, ey), max(worst_z, ez)
    for name, x, zi in IC.special_inputs():
        ey, ez = IC.reference_error(IC.DESIGNS[name], x, zi)
        assert ey <= 1e-9 and ez <= 1e-9, (name, x.shape, ey, ez)
        worst_y, worst_z = max(worst_y, ey), max(worst_z, ez)
    print(f"scipy vs long double: y {worst_y:.2e}, zf {worst_z:.2e}")


def test_design_table():
    radius = {k: max(np.abs(np.roots(sec[3:])).max() for sec in sos) for k, sos in IC.DESIGNS.items()}
    for name, r in (("bessel4_lp", 0.842), ("cheby1_5_lp", 0.966), ("cheby2_6_hp", 0.983), ("butter4_bp", 0.987),
                    ("ellip8_bp", 0.9994), ("ellip10_bs", 0.9997), ("eq10", 0.998)):
        assert abs(radius[name] - r) < 6e-4, (name, radius[name])
    assert all(r < 1.0 for r in radius.values())
    # splitting a cascade at 8 sections changes nothing in float64 (the kernels' group rule rests on it)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(4000)
    for name in ("ellip10_bs", "cat17", "cat32"):
        sos = IC.DESIGNS[name]
        y = x
        for s0 in range(0, sos.shape[0], 8):
            y = signal.sosfilt(sos[s0:s0 + 8], y)
        assert np.array_equal(y, signal.sosfilt(sos, x))


WN = {"lowpass": 3000.0, "highpass": 500.0, "bandpass": (300.0, 3400.0), "bandstop": (1000.0, 2000.0)}


@pytest.mark.parametrize("family,rp,rs", [("butter", None, None), ("cheby1", 1.0, None), ("cheby2", None, 40.0), ("ellip", 0.5, 60.0),
                                          ("bessel", None, None)])
def test_design_iir_sos_is_iirfilter(family, rp, rs):
    from sygnals_amd.core import filters as F
    for btype, cut in WN.items():
        for order in (1, 4, 5, 8):
            wn = cut / (FS / 2) if not isinstance(cut, tuple) else (cut[0] / (FS / 2), cut[1] / (FS / 2))
            want = signal.iirfilter(order, wn, rp=rp, rs=rs, btype=btype, ftype=family, output="sos")
            got = F.design_iir_sos(cut, FS, order, btype, family=family, rp=rp, rs=rs)
            assert got.dtype == np.float64 and np.array_equal(got, want)
            if family == "butter":
                assert np.array_equal(got, F.design_butterworth_sos(cut, FS, order, btype))
    if family == "bessel":
        for norm in ("phase", "delay", "mag"):
            assert np.array_equal(F.design_iir_sos(2000.0, FS, 4, "lowpass", family="bessel", norm=norm),
                                  signal.bessel(4, 2000.0 / (FS / 2), "lowpass", output="sos", norm=norm))


def test_design_iir_sos_refusals():
    from sygnals_amd.core import filters as F
    served = "served: 'butter', 'cheby1' (with rp > 0), 'cheby2' (with rs > 0), 'ellip' (with rp > 0 and rs > 0), 'bessel'"
    with pytest.raises(ValueError) as e:
        F.design_iir_sos(1000.0, FS, 4, "lowpass", family="chebyshev")
    assert "Unknown filter family 'chebyshev'" in str(e.value) and served in str(e.value)
    for family, kw, name in (("cheby1", {}, "rp"), ("cheby1", {"rp": 0.0}, "rp"), ("cheby1", {"rp": -1.0, "rs": 40.0}, "rp"),
                             ("cheby2", {}, "rs"), ("cheby2", {"rp": 1.0}, "rs"), ("cheby2", {"rs": -3.0}, "rs"),
                             ("ellip", {"rs": 40.0}, "rp"), ("ellip", {"rp": 1.0}, "rs"), ("ellip", {"rp": 1.0, "rs": 0.0}, "rs"),
                             ("ellip", {"rp": float("nan"), "rs": 40.0}, "rp")):
        with pytest.raises(ValueError) as e:
            F.design_iir_sos(1000.0, FS, 4, "lowpass", family=family, **kw)
        assert f"Family {family!r} needs {name} > 0 dB" in str(e.value) and served in str(e.value)
    with pytest.raises(ValueError, match="Unknown Bessel norm 'energy'"):
        F.design_iir_sos(1000.0, FS, 4, "lowpass", family="bessel", norm="energy")
    # the cutoff checks and messages of design_butterworth_sos
    for family, kw in (("butter", {}), ("ellip", {"rp": 1.0, "rs": 40.0})):
        with pytest.raises(ValueError, match=r"Cutoff frequency \(24000.0 Hz\) must be strictly between 0 and Nyquist \(24000.0 Hz\)"):
            F.design_iir_sos(24000.0, FS, 4, "lowpass", family=family, **kw)
        with pytest.raises(ValueError, match=r"Low cutoff \(3400.0 Hz\) must be less than high cutoff \(300.0 Hz\)"):
            F.design_iir_sos((3400.0, 300.0), FS, 4, "bandpass", family=family, **kw)
        with pytest.raises(ValueError, match="Both low"):
            F.design_iir_sos((0.0, 300.0), FS, 4, "bandpass", family=family, **kw)
        with pytest.raises(TypeError, match="cutoff must be a float"):
            F.design_iir_sos([300.0, 3400.0], FS, 4, "bandpass", family=family, **kw)


def test_sosfilt_zi_and_fir_design():
    from sygnals_amd.core import filters as F
    for name, sos in IC.DESIGNS.items():
        want = signal.sosfilt_zi(sos)
        got = F.sosfilt_zi(sos)
        # both solve, per section, a system whose condition is 1 / |1 + a1 + a2| (1.7e-5 for the 31 Hz EQ band), and
        # the sections' gains multiply along the cascade: 4 eps per section over that, of the largest state
        tol = 4 * sos.shape[0] * 2.0 ** -52 / np.min(np.abs(1.0 + sos[:, 4] + sos[:, 5]))
        assert got.shape == want.shape and np.abs(got - want).max() <= tol * np.abs(want).max(), name
    with pytest.raises(ValueError, match=r"shape \(n_sections, 6\)"):
        F.sosfilt_zi(np.zeros((2, 5)))
    for args, kw in (((101, 3000.0), {}), ((64, (300.0, 3400.0)), {"pass_zero": False, "window": ("kaiser", 6.0)}),
                     ((31, 8000.0), {"pass_zero": False, "window": "hann"})):
        cut = args[1]
        assert np.array_equal(F.design_fir(args[0], list(cut) if isinstance(cut, tuple) else cut, FS, **kw),
                              signal.firwin(args[0], cut, fs=FS, **kw))
    with pytest.raises(ValueError):
        F.design_fir(64, 8000.0, FS, pass_zero=False)                  # an even number of taps cannot pass Nyquist


def _gain_db(sos, freq, fs=FS):
    w = 2.0 * np.pi * freq / fs
    z = np.exp(-1j * w * np.arange(3))
    return 20.0 * np.log10(abs(np.dot(sos[0, :3], z) / np.dot(sos[0, 3:], z)))


def test_eq_biquads_by_construction():
    """Asserted to 1e-8 dB (observed within 2e-10 dB); the inverse pair to 1e-15."""
    from sygnals_amd.core.audio.effects import design_eq_sos
    worst = 0.0
    for freq in (31.25, 1000.0, 16000.0):
        for g in (-12.0, -6.0, 0.5, 6.0, 12.0):
            for q in (0.5, 1.0, 1.414, 8.0):
                pk = design_eq_sos("peak", FS, freq, g, q)
                assert pk.shape == (1, 6) and pk.dtype == np.float64 and pk[0, 3] == 1.0
                errs = [_gain_db(pk, freq) - g, _gain_db(pk, 0.0), _gain_db(pk, FS / 2)]
                inv = design_eq_sos("peak", FS, freq, -g, q)
                assert np.allclose(pk[0, :3] / pk[0, 0], inv[0, 3:], rtol=0, atol=1e-15)
                assert np.allclose(pk[0, 3:], inv[0, :3] / inv[0, 0], rtol=0, atol=1e-15)
                lo, hi = design_eq_sos("low_shelf", FS, freq, g, q), design_eq_sos("high_shelf", FS, freq, g, q)
                errs += [_gain_db(lo, 0.0) - g, _gain_db(lo, FS / 2), _gain_db(lo, freq) - g / 2,
                         _gain_db(hi, FS / 2) - g, _gain_db(hi, 0.0), _gain_db(hi, freq) - g / 2]
                worst = max(worst, max(abs(e) for e in errs))
                assert max(abs(e) for e in errs) <= 1e-8, (freq, g, q, errs)
                for sos in (pk, lo, hi):
                    assert np.abs(np.roots(sos[0, 3:])).max() < 1.0
    print(f"EQ gains by construction: worst {worst:.2e} dB")
    # defaults: Q 1 for the peak, 1 / sqrt(2) for the shelves
    assert np.array_equal(design_eq_sos("peak", FS, 1000.0, 3.0), design_eq_sos("peak", FS, 1000.0, 3.0, 1.0))
    assert np.array_equal(design_eq_sos("low_shelf", FS, 200.0, 3.0), design_eq_sos("low_shelf", FS, 200.0, 3.0, 1 / np.sqrt(2.0)))
    for freq, q in ((50.0, 30.0), (1000.0, 2.0)):
        b, a = signal.iirnotch(freq, q, FS)
        got = design_eq_sos("notch", FS, freq, 0.0, q)
        assert np.array_equal(got, np.concatenate([b, a])[None]) and np.abs(np.roots(got[0, 3:])).max() < 1.0
    # the package's peak equals the cookbook form the test cases write out themselves
    assert np.allclose(design_eq_sos("peak", FS, 250.0, -6.0, 1.414)[0], IC.eq_peak(250.0, -6.0, 1.414), rtol=1e-15, atol=0)


def test_eq_validation_and_stacking():
    from sygnals_amd.core.audio.effects import equalizer as EQ
    for freq in (0.0, -5.0, 24000.0, 30000.0):
        with pytest.raises(ValueError) as e:
            EQ.design_eq_sos("peak", FS, freq, 3.0)
        assert str(e.value) == f"EQ frequency ({freq} Hz) must be between 0 and Nyquist (24000.0 Hz)."
    for kind in ("peak", "notch", "low_shelf"):
        for q in (0.0, -1.0):
            with pytest.raises(ValueError, match="Q factor must be positive for peak/notch filters."):
                EQ.design_eq_sos(kind, FS, 1000.0, 3.0, q)
    with pytest.raises(ValueError, match="Unknown EQ filter type 'bell'"):
        EQ.design_eq_sos("bell", FS, 1000.0, 3.0)
    for kind in ("peak", "low_shelf", "high_shelf"):
        for g in (0.0, 0.09, -0.099):
            assert EQ.design_eq_sos(kind, FS, 1000.0, g) is None
        assert EQ.design_eq_sos(kind, FS, 1000.0, 0.1) is not None
    g10 = EQ.graphic_eq_sos(FS, IC.GRAPHIC_BANDS, IC.GRAPHIC_Q)
    assert g10.shape == (10, 6) and np.allclose(g10, IC.DESIGNS["eq10"], rtol=1e-15, atol=0)
    assert EQ.graphic_eq_sos(FS, [(100.0, 0.05), (1000.0, 3.0)]).shape == (1, 6)
    assert EQ.graphic_eq_sos(FS, [(100.0, 0.05)]).shape == (0, 6) and EQ.graphic_eq_sos(FS, []).shape == (0, 6)
    with pytest.raises(ValueError, match="band_gains must be a list"):
        EQ.graphic_eq_sos(FS, [(100.0, 1.0, 2.0)])
    with pytest.raises(ValueError, match="q_factor must be positive."):
        EQ.graphic_eq_sos(FS, [(100.0, 1.0)], 0.0)
    params = [{"type": "Peak", "freq": 1000.0, "gain_db": 4.0, "q": 2.0}, {"type": "low_shelf", "freq": 120.0, "gain_db": -3.0},
              {"type": "high_shelf", "freq": 8000.0, "gain_db": 0.01}, {"type": "notch", "freq": 50.0, "q": 30.0}]
    sos = EQ.parametric_eq_sos(FS, params)
    assert sos.shape == (3, 6)                                         # the 0.01 dB shelf is skipped
    assert np.array_equal(sos[0:1], EQ.design_eq_sos("peak", FS, 1000.0, 4.0, 2.0))
    assert np.array_equal(sos[1:2], EQ.design_eq_sos("low_shelf", FS, 120.0, -3.0))
    assert np.array_equal(sos[2:3], EQ.design_eq_sos("notch", FS, 50.0, 0.0, 30.0))
    with pytest.raises(ValueError, match="EQ stage 1 missing required 'type' or 'freq' parameter."):
        EQ.parametric_eq_sos(FS, [{"type": "peak", "freq": 100.0}, {"type": "peak"}])
    with pytest.raises(ValueError, match="params must be a list of dictionaries"):
        EQ.parametric_eq_sos(FS, ({"type": "peak", "freq": 100.0},))
    with pytest.raises(ValueError, match="must be between 0 and Nyquist"):
        EQ.parametric_eq_sos(FS, [{"type": "peak", "freq": 24000.0, "gain_db": 3.0}])
    # no stage left: a copy, and no device is needed for it
    x = np.linspace(-1.0, 1.0, 50)
    for y in (EQ.apply_graphic_eq(x, 48000, [(100.0, 0.05)]), EQ.apply_parametric_eq(x, 48000, [])):
        assert y.dtype == np.float64 and np.array_equal(y, x) and y is not x
    with pytest.raises(ValueError, match="Input audio data must be a 1D array."):
        EQ.apply_graphic_eq(np.zeros((2, 8)), 48000, [(100.0, 3.0)])
