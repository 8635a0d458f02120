"""The pitch entries of the C ABI are declared, bound and exported, and reject bad arguments before device work."""
import ctypes as C
import os

import pytest

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_pitch_frames_f32", "syg_pyin_viterbi_f32", "syg_pyin_work_bytes"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)


def _frames(h, p, frame_length=2048, win=1024, min_p=22, max_p=734, y=True, K=358, work=True):
    return h.syg_pitch_frames_f32(p if y else None, 1, 48000, 48000, frame_length, win, 512, 1, 94, 48000.0, min_p, max_p,
                                  1, 0.1, 65.4, 601, p, K, p, None, p, p, p, p, None, None)


def test_frame_stage_rejects(h):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert _frames(h, p, frame_length=4096) == -3 and b"only 2048" in h.syg_last_error()
    assert _frames(h, p, min_p=734, max_p=734) == -1 and b"min_period < max_period" in h.syg_last_error()
    assert _frames(h, p, max_p=1100) == -1 and b"max_period" in h.syg_last_error()
    assert _frames(h, p, y=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _frames(h, p, K=100) == -1 and b"K must be" in h.syg_last_error()
    rc = h.syg_pitch_frames_f32(p, 1, 48000, 48000, 2048, 1024, 512, 1, 94, 48000.0, 22, 734, 0, 0.1, 65.4, 601, None, 0,
                                p, None, None, None, None, None, None, None)
    assert rc == -1 and b"f0_out" in h.syg_last_error()


def test_viterbi_rejects(h):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    lc = (C.c_double * 3)()
    need = h.syg_pyin_work_bytes(4, 94, 601)
    assert need == 4 * 94 * 1202 * 2 and h.syg_pyin_work_bytes(1, 1, 40000) == -1
    rc = h.syg_pyin_viterbi_f32(p, p, p, p, 4, 94, 358, 601, 25, p, 51, C.cast(lc, C.c_void_p), 65.4, p, need - 1, p, p,
                                None, None)
    assert rc == -1 and b"workspace" in h.syg_last_error()
    rc = h.syg_pyin_viterbi_f32(None, p, p, p, 4, 94, 358, 601, 25, p, 51, C.cast(lc, C.c_void_p), 65.4, p, need, p, p,
                                None, None)
    assert rc == -1 and b"null pointer" in h.syg_last_error()
    rc = h.syg_pyin_viterbi_f32(p, p, p, p, 4, 94, 358, 601, 25, p, 50, C.cast(lc, C.c_void_p), 65.4, p, need, p, p,
                                None, None)
    assert rc == -1 and b"rows" in h.syg_last_error()


def test_public_functions_importable():
    from sygnals_amd.core.audio.features import (fundamental_frequency, fundamental_frequency_batch, jitter,  # noqa: F401
                                                 shimmer)
