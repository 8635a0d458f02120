"""The audio-effect entries of the C ABI are declared, bound and exported, and reject bad arguments before device work."""
import ctypes as C
import os

import pytest

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_fx_delay_chunk", "syg_fx_delay_work_bytes", "syg_fx_delay_f32", "syg_spectral_gate_f32", "syg_fx_mix_f32",
       "syg_fx_tremolo_f32", "syg_fx_compress_f32", "syg_fx_midside_f32"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_float * 64)()
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)


def _delay(h, p, x=True, B=2, L=1000, ldx=1000, D=100, fb=0.4, dry=1.0, wet=0.5, out=True, ldo=1000, work=None):
    return h.syg_fx_delay_f32(p if x else None, B, L, ldx, D, fb, dry, wet, p if out else None, ldo, work, None)


def test_delay_rejects(h, p):
    assert _delay(h, p, x=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _delay(h, p, out=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _delay(h, p, B=0) == -1 and b"bad B / L" in h.syg_last_error()
    assert _delay(h, p, L=0) == -1 and b"bad B / L" in h.syg_last_error()
    assert _delay(h, p, ldx=999) == -1 and b"bad ldx / ldo" in h.syg_last_error()
    assert _delay(h, p, ldo=999) == -1 and b"bad ldx / ldo" in h.syg_last_error()
    for D in (0, -5):
        assert _delay(h, p, D=D) == -1 and b"delay_samples" in h.syg_last_error()
    for fb in (-0.1, 1.0, 1.5, NAN, INF, 1.0 - 1e-12):           # the last rounds to 1 in float32
        assert _delay(h, p, fb=fb) == -1 and b"feedback" in h.syg_last_error()
    assert _delay(h, p, dry=NAN) == -1 and b"dry / wet" in h.syg_last_error()
    assert _delay(h, p, wet=INF) == -1 and b"dry / wet" in h.syg_last_error()
    # one long row with a short delay takes the chunked form, which needs its workspace
    assert _delay(h, p, B=1, L=1 << 20, ldx=1 << 20, ldo=1 << 20, D=7) == -1 and b"needs `work`" in h.syg_last_error()


def test_delay_plan(h):
    K = h.syg_fx_delay_chunk()
    assert K >= 16
    assert h.syg_fx_delay_work_bytes(1024, 22050, 11025) == 0            # a batch with a long delay: chains of two steps
    assert h.syg_fx_delay_work_bytes(1, 4 * K * 7 - 7, 7) == 0           # a chain one step short of four chunks
    assert h.syg_fx_delay_work_bytes(1, 4 * K * 7, 7) == 4 * 4 * 7       # four chunks of seven residues, carries plain
    big = h.syg_fx_delay_work_bytes(1, 1 << 24, 7)
    n1 = -(-(-(-(1 << 24) // 7)) // K)                                   # chunks of the first level
    assert big >= 4 * n1 * 7 and big <= 4 * n1 * 7 * 1.02               # the deeper levels are a small addition
    assert h.syg_fx_delay_work_bytes(0, 100, 7) == -1 and h.syg_fx_delay_work_bytes(1, 100, 0) == -1
    assert h.syg_set_option(5, 2) == -1 and b"fx_delay_form" in h.syg_last_error()
    assert h.syg_get_option(5) == -1
    try:
        assert h.syg_set_option(5, 1) == 0 and h.syg_fx_delay_work_bytes(2, 1000, 100) == 4 * 2 * 100
        assert h.syg_set_option(5, 0) == 0 and h.syg_fx_delay_work_bytes(1, 1 << 24, 7) == 0
    finally:
        assert h.syg_set_option(5, -1) == 0


def _gate(h, p, D=True, B=2, T=44, Dn=True, Tn=22, a=1.0, G=True, N=True):
    return h.syg_spectral_gate_f32(p if D else None, B, T, p if Dn else None, Tn, a, p if G else None, p if N else None, None)


def test_gate_rejects(h, p):
    for kw in ({"D": False}, {"Dn": False}, {"G": False}, {"N": False}):
        assert _gate(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"T": 0}, {"Tn": 0}, {"T": -1}):
        assert _gate(h, p, **kw) == -1 and b"bad B / T / Tn" in h.syg_last_error()
    for a in (-0.5, NAN, INF):
        assert _gate(h, p, a=a) == -1 and b"reduction amount" in h.syg_last_error()


def test_mix_rejects(h, p):
    f = h.syg_fx_mix_f32
    assert f(None, 10, 10, p, 10, 10, 1, 10, 1.0, 1.0, p, 10, None) == -1 and b"null pointer" in h.syg_last_error()
    assert f(p, 10, 10, None, 0, 0, 1, 10, 1.0, 1.0, None, 10, None) == -1 and b"null pointer" in h.syg_last_error()
    assert f(p, 10, 10, None, 0, 0, 0, 10, 1.0, 1.0, p, 10, None) == -1 and b"bad B / L" in h.syg_last_error()
    assert f(p, 10, 10, None, 0, 0, 1, 0, 1.0, 1.0, p, 10, None) == -1 and b"bad B / L" in h.syg_last_error()
    assert f(p, 10, 10, None, 0, 0, 1, 10, 1.0, 1.0, p, 9, None) == -1 and b"bad B / L" in h.syg_last_error()
    assert f(p, 10, 9, None, 0, 0, 1, 10, 1.0, 1.0, p, 10, None) == -1 and b"bad Lx" in h.syg_last_error()
    assert f(p, 10, 10, p, 20, 10, 1, 30, 1.0, 1.0, p, 30, None) == -1 and b"bad Ly" in h.syg_last_error()
    assert f(p, 10, 10, p, 10, 10, 1, 10, NAN, 1.0, p, 10, None) == -1 and b"finite" in h.syg_last_error()


def _trem(h, p, x=True, B=1, L=50, ldx=50, sr=8000.0, rate=5.0, depth=0.5, shape=0, n0=0, out=True, ldo=50):
    return h.syg_fx_tremolo_f32(p if x else None, B, L, ldx, sr, rate, depth, shape, n0, p if out else None, ldo, None)


def test_tremolo_rejects(h, p):
    assert _trem(h, p, x=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _trem(h, p, out=False) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"L": 0}, {"ldx": 49}, {"ldo": 49}):
        assert _trem(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for rate in (0.0, -1.0, NAN):
        assert _trem(h, p, rate=rate) == -1 and b"rate must be positive" in h.syg_last_error()
    for depth in (-0.01, 1.01, NAN):
        assert _trem(h, p, depth=depth) == -1 and b"depth" in h.syg_last_error()
    for shape in (-1, 3):
        assert _trem(h, p, shape=shape) == -1 and b"unknown LFO shape" in h.syg_last_error()
    assert _trem(h, p, sr=0.0) == -1 and b"sr must be positive" in h.syg_last_error()
    assert _trem(h, p, n0=-1) == -1 and b"first sample" in h.syg_last_error()


def test_compress_and_midside_reject(h, p):
    c, m = h.syg_fx_compress_f32, h.syg_fx_midside_f32
    assert c(None, 1, 50, 50, 0.8, 4.0, p, 50, None) == -1 and b"null pointer" in h.syg_last_error()
    assert c(p, 0, 50, 50, 0.8, 4.0, p, 50, None) == -1 and b"bad B / L" in h.syg_last_error()
    assert c(p, 1, 0, 50, 0.8, 4.0, p, 50, None) == -1 and b"bad B / L" in h.syg_last_error()
    for ratio in (0.99, 0.0, NAN):
        assert c(p, 1, 50, 50, 0.8, ratio, p, 50, None) == -1 and b"ratio must be >= 1" in h.syg_last_error()
    for thr in (-0.1, NAN):
        assert c(p, 1, 50, 50, thr, 4.0, p, 50, None) == -1 and b"threshold" in h.syg_last_error()
    assert m(p, 1, 20, 20, 1.5, None, 20, None) == -1 and b"null pointer" in h.syg_last_error()
    assert m(p, 1, 0, 20, 1.5, p, 20, None) == -1 and b"bad B / L" in h.syg_last_error()
    for wd in (-1.0, NAN):
        assert m(p, 1, 20, 20, wd, p, 20, None) == -1 and b"width" in h.syg_last_error()


def test_public_functions_importable():
    import sygnals_amd.core.audio.effects as E
    for name in ("apply_delay", "apply_tremolo", "simple_dynamic_range_compression", "apply_reverb", "adjust_gain",
                 "stereo_widening_midside", "noise_reduction_spectral", "transient_shaping_hpss"):
        assert callable(getattr(E, name)) and callable(getattr(E, name + "_batch"))
    from sygnals_amd.core.audio.effects import compression, delay, reverb, tremolo, utility  # noqa: F401
    from sygnals_amd.ops import fx_compress, fx_delay, fx_midside, fx_mix, fx_tremolo, spectral_gate  # noqa: F401


def test_mirrors_validate_like_the_reference():
    """Every raise of the reference's effect files, with its type and text; all fire before any device work."""
    import numpy as np
    import sygnals_amd.core.audio.effects as E
    y, y2 = np.zeros(100), np.zeros((2, 100))

    def raises(text, fn, *a, **k):
        with pytest.raises(ValueError) as e:
            fn(*a, **k)
        assert str(e.value) == text

    one_d = "Input audio data must be a 1D array."
    raises(one_d, E.apply_delay, y2, 8000)
    raises("delay_time must be non-negative.", E.apply_delay, y, 8000, delay_time=-0.1)
    for fb in (-0.1, 1.0):
        raises("feedback gain must be between 0.0 and < 1.0.", E.apply_delay, y, 8000, feedback=fb)
    raises("wet_level must be between 0.0 and 1.0.", E.apply_delay, y, 8000, wet_level=1.1)
    raises("dry_level must be between 0.0 and 1.0.", E.apply_delay, y, 8000, dry_level=-0.1)
    raises(one_d, E.apply_tremolo, y2, 8000)
    raises("Tremolo depth must be between 0.0 and 1.0.", E.apply_tremolo, y, 8000, depth=1.5)
    raises("Tremolo rate must be positive.", E.apply_tremolo, y, 8000, rate=0.0)
    raises("LFO shape must be 'sine', 'triangle', or 'square'.", E.apply_tremolo, y, 8000, shape="saw")
    raises(one_d, E.simple_dynamic_range_compression, y2)
    raises("Threshold must be between 0.0 and 1.0.", E.simple_dynamic_range_compression, y, threshold=1.2)
    raises("Compression ratio must be >= 1.0.", E.simple_dynamic_range_compression, y, ratio=0.5)
    raises(one_d, E.apply_reverb, y2, 8000)
    raises("wet_level must be between 0.0 and 1.0.", E.apply_reverb, y, 8000, wet_level=2.0)
    raises("dry_level must be between 0.0 and 1.0.", E.apply_reverb, y, 8000, dry_level=2.0)
    raises("decay_time must be non-negative.", E.reverb._generate_basic_ir, 8000, -1.0)
    raises("Input audio data must be a NumPy array.", E.adjust_gain, [0.0, 1.0], 3.0)
    raises("Input audio 'y' must be 1D for spectral noise reduction.", E.noise_reduction_spectral, y2, 8000)
    for dur in (0.0, -1.0, 1.0):                                      # 1 s at 8 kHz is longer than the clip
        raises("Invalid noise_profile_duration.", E.noise_reduction_spectral, y, 8000, noise_profile_duration=dur)
    raises("reduction_amount must be non-negative.", E.noise_reduction_spectral, y, 8000, 0.01, reduction_amount=-1.0)
    raises("Input audio 'y' must be 1D for HPSS transient shaping.", E.transient_shaping_hpss, y2, 8000)
    stereo = "Input audio 'y' must be a 2-channel NumPy array with shape (2, n_samples) for stereo widening."
    raises(stereo, E.stereo_widening_midside, y)
    raises(stereo, E.stereo_widening_midside, np.zeros((3, 100)))
    raises("width_factor must be non-negative.", E.stereo_widening_midside, y2, -0.5)
    # what the device path does not serve is refused, with what is served in the message
    for kw in ({"n_fft": 1024}, {"hop_length": 256}):
        with pytest.raises(ValueError, match="only n_fft=2048 with hop_length 512"):
            E.noise_reduction_spectral(y, 8000, 0.01, **kw)
    with pytest.raises(ValueError, match="holds no sample"):
        E.noise_reduction_spectral(y, 8000, 0.0001)
    # the seeded impulse response is the reference's
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_effects.npz"))
    for i, (dec, _, _) in enumerate(g["reverb_params"]):
        assert np.array_equal(E.reverb._generate_basic_ir(8000, dec, seed=7), g[f"reverb_ir_{i}"])
