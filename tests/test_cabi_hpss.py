"""The HPSS entries of the C ABI are declared, bound and exported, and reject bad arguments before device work."""
import ctypes as C
import os

import pytest

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_hpss_masks_f32", "syg_istft2048_f32", "syg_hnr_rows_f32"]


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


def _masks(h, p, D=True, B=2, T=94, kh=31, kp=31, power=2.0, mh=1.0, mp=1.0, out=True):
    return h.syg_hpss_masks_f32(p if D else None, B, T, kh, kp, power, mh, mp, p if out else None, p, None, None, None)


def test_masks_reject(h, p):
    assert _masks(h, p, D=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _masks(h, p, out=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _masks(h, p, T=0) == -1 and b"bad B / T" in h.syg_last_error()
    assert _masks(h, p, B=0) == -1 and b"bad B / T" in h.syg_last_error()
    for kh, kp in ((0, 31), (31, 64), (64, 1), (31, -1)):
        assert _masks(h, p, kh=kh, kp=kp) == -1 and b"median windows" in h.syg_last_error()
    for pw in (0.0, -1.0, float("nan"), float("-inf")):
        assert _masks(h, p, power=pw) == -1 and b"power" in h.syg_last_error()
    for mh, mp in ((0.5, 1.0), (1.0, 0.99), (float("nan"), 1.0), (1.0, float("inf"))):
        assert _masks(h, p, mh=mh, mp=mp) == -1 and b"margins" in h.syg_last_error()


def _istft(h, p, D=True, B=1, T=94, hop=512, center=1, length=48000, win=True, tw=True, ma=None, ya=True, mb=None,
           yb=None, ldy=48000):
    return h.syg_istft2048_f32(p if D else None, B, T, hop, center, length, p if win else None, p if tw else None, ma,
                               p if ya else None, mb, yb, ldy, None)


def test_istft_rejects(h, p):
    assert _istft(h, p, hop=256) == -3 and b"only hop 512" in h.syg_last_error()
    assert _istft(h, p, center=0) == -3 and b"only hop 512" in h.syg_last_error()
    assert _istft(h, p, D=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _istft(h, p, win=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _istft(h, p, tw=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _istft(h, p, ya=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _istft(h, p, mb=p) == -1 and b"go together" in h.syg_last_error()
    assert _istft(h, p, mb=p, yb=p) == -1 and b"needs mask_a" in h.syg_last_error()
    assert _istft(h, p, length=0) == -1 and b"bad B / T" in h.syg_last_error()
    assert _istft(h, p, ldy=47999) == -1 and b"bad B / T" in h.syg_last_error()
    assert _istft(h, p, T=0) == -1 and b"bad B / T" in h.syg_last_error()


def _hnr(h, p, yh=True, yp=True, B=1, L=22050, ldy=22050, fl=1024, hop=256, center=1, T=87, out=True):
    return h.syg_hnr_rows_f32(p if yh else None, p if yp else None, B, L, ldy, fl, hop, center, T, p if out else None,
                              None, None, None)


def test_hnr_rows_reject(h, p):
    assert _hnr(h, p, yh=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _hnr(h, p, yp=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _hnr(h, p, out=False) == -1 and b"null pointer" in h.syg_last_error()
    assert _hnr(h, p, L=0) == -1 and b"bad B / L" in h.syg_last_error()
    assert _hnr(h, p, ldy=100) == -1 and b"bad B / L" in h.syg_last_error()
    assert _hnr(h, p, hop=0) == -1 and b"frame_length / hop" in h.syg_last_error()
    assert _hnr(h, p, fl=0) == -1 and b"frame_length / hop" in h.syg_last_error()
    assert _hnr(h, p, center=2) == -1 and b"frame_length / hop" in h.syg_last_error()
    assert _hnr(h, p, T=88) == -1 and b"framing rule" in h.syg_last_error()


def test_public_functions_importable():
    from sygnals_amd.core.audio.features import harmonic_to_noise_ratio, harmonic_to_noise_ratio_batch  # noqa: F401
    from sygnals_amd.ops import hnr_rows, hpss, hpss_masks, istft2048  # noqa: F401
