"""The onset entries of the C ABI are declared, bound and exported, and reject bad arguments before device work."""
import ctypes as C
import os

import pytest

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_onset_strength_work_bytes", "syg_onset_strength_f32", "syg_onset_peaks_f32", "syg_clip_metrics_f32"]


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


def _strength(h, p, mel=True, B=2, M=128, T=94, amin=1e-10, top_db=80.0, lag=1, max_size=1, pad=3, T_out=94,
              detrend=0, env=True, work=None):
    return h.syg_onset_strength_f32(p if mel else None, B, M, T, amin, top_db, lag, max_size, pad, T_out, detrend,
                                    p if env else None, work, None)


def test_strength_rejects(h, p):
    assert _strength(h, p, mel=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _strength(h, p, env=False) == -1 and b"null pointer" in h.syg_last_error()
    for kw in (dict(B=0), dict(T=0), dict(M=0), dict(B=-1), dict(T=-5)):
        assert _strength(h, p, **kw) == -1 and b"bad B / M / T" in h.syg_last_error()
    for amin in (0.0, -1e-10, float("nan"), float("inf")):
        assert _strength(h, p, amin=amin) == -1 and b"amin must be strictly positive" in h.syg_last_error()
    assert _strength(h, p, top_db=float("nan")) == -1 and b"top_db" in h.syg_last_error()
    for lag in (0, -1):
        assert _strength(h, p, lag=lag) == -1 and b"lag must be a positive integer" in h.syg_last_error()
    for lag, T in ((94, 94), (95, 94), (1, 1)):
        assert _strength(h, p, lag=lag, T=T) == -1 and b"needs more than" in h.syg_last_error()
    assert _strength(h, p, max_size=0) == -1 and b"max_size must be a positive integer" in h.syg_last_error()
    for kw in (dict(pad=-1), dict(T_out=0), dict(T_out=98)):
        assert _strength(h, p, **kw) == -1 and b"bad pad / T_out" in h.syg_last_error()
    # a clip of more than 2048 frames is split over workgroups and needs the workspace
    assert h.syg_onset_strength_work_bytes(1024, 128, 94) == 0 and h.syg_onset_strength_work_bytes(3, 128, 2048) == 0
    assert h.syg_onset_strength_work_bytes(1, 128, 337501) == 330 * 4
    assert h.syg_onset_strength_work_bytes(2, 128, 2049) == 2 * 3 * 4
    assert h.syg_onset_strength_work_bytes(0, 128, 94) == -1 and h.syg_onset_strength_work_bytes(1, 0, 94) == -1
    assert _strength(h, p, B=1, T=337501, T_out=337501) == -1 and b"workspace" in h.syg_last_error()


def _peaks(h, p, env=True, B=2, T=94, ld=94, pre_max=1, post_max=1, pre_avg=4, post_avg=5, delta=0.07, wait=1,
           normalize=1, backtrack=0, frames=True, count=True):
    return h.syg_onset_peaks_f32(p if env else None, B, T, ld, pre_max, post_max, pre_avg, post_avg, delta, wait,
                                 normalize, backtrack, None, p if frames else None, p if count else None, None)


def test_peaks_reject(h, p):
    for kw in (dict(env=False), dict(frames=False), dict(count=False)):
        assert _peaks(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in (dict(B=0), dict(T=0), dict(ld=93), dict(T=-1)):
        assert _peaks(h, p, **kw) == -1 and b"bad B / T / ld" in h.syg_last_error()
    for kw in (dict(pre_max=-1), dict(post_max=-1), dict(pre_avg=-2), dict(post_avg=-1), dict(wait=-1)):
        assert _peaks(h, p, **kw) == -1 and b"must be non-negative" in h.syg_last_error()
    assert _peaks(h, p, pre_max=0, post_max=0) == -1 and b"pre_max + post_max must be at least 1" in h.syg_last_error()
    assert _peaks(h, p, pre_avg=0, post_avg=0) == -1 and b"pre_avg + post_avg must be at least 1" in h.syg_last_error()
    assert _peaks(h, p, pre_max=3, post_max=0) == -1 and b"must be positive" in h.syg_last_error()
    assert _peaks(h, p, pre_avg=3, post_avg=0) == -1 and b"must be positive" in h.syg_last_error()
    for d in (float("nan"), float("inf"), float("-inf"), -0.01):
        assert _peaks(h, p, delta=d) == -1 and b"delta must be finite" in h.syg_last_error()


def test_clip_metrics_rejects(h, p):
    assert h.syg_clip_metrics_f32(None, 1, 100, 100, p, None) == -1 and b"null pointer" in h.syg_last_error()
    assert h.syg_clip_metrics_f32(p, 1, 100, 100, None, None) == -1 and b"null pointer" in h.syg_last_error()
    for B, L, ld in ((0, 100, 100), (1, 0, 100), (1, 100, 99)):
        assert h.syg_clip_metrics_f32(p, B, L, ld, p, None) == -1 and b"bad B / L / ldy" in h.syg_last_error()


def test_public_functions_importable():
    from sygnals_amd.core.audio.features import (detect_onsets, detect_onsets_batch, get_basic_audio_metrics,  # noqa: F401
                                                 onset_strength_batch)
    from sygnals_amd.core.segmentation import (segment_by_event, segment_by_onsets, segment_by_silence,  # noqa: F401
                                               segment_fixed_length)
    from sygnals_amd.ops import clip_metrics, onset_peaks, onset_strength  # noqa: F401
