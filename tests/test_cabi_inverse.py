"""The feature-inversion entries of the C ABI are declared, bound and exported, size their workspace, and refuse bad
arguments before device work; the operators and the mirrors refuse what is not served without a device; the host tables
are the restatement's; the plugin registers the public functions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import inverse_ref as R
from tests.test_cabi_symbols import declared_functions

NEW = ["syg_gl_project_work_bytes", "syg_gl_project_f32", "syg_inv_dense_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 4096)()                     # never dereferenced: every call is refused
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)


def test_work_bytes(h):
    wb = h.syg_gl_project_work_bytes
    assert wb(1, 1) == 16 and wb(3, 2) == 3 * 2 * 16            # ceil(2 * 1025 / 2048) = 2 workgroups a clip
    assert wb(2, 65) == 2 * 33 * 16 and wb(1, 1 << 15) == 1024 * 16    # capped at 1024 workgroups a clip
    assert wb(0, 5) == -1 and wb(5, 0) == -1 and b"bad B / T" in h.syg_last_error()


def test_entries_refuse_before_device_work(h, p):
    err = h.syg_last_error
    assert h.syg_gl_project_f32(None, None, p, 1, 2, 0.0, p, None, None, None) == -1 and b"null pointer" in err()
    assert h.syg_gl_project_f32(p, None, None, 1, 2, 0.0, p, None, None, None) == -1 and b"null pointer" in err()
    assert h.syg_gl_project_f32(p, None, p, 1, 2, 0.0, None, None, None, None) == -1 and b"null pointer" in err()
    assert h.syg_gl_project_f32(p, None, p, 1, 2, 0.0, p, p, None, None) == -1 and b"sums needs the workspace" in err()
    assert h.syg_gl_project_f32(p, None, p, 0, 2, 0.0, p, None, None, None) == -1 and b"bad B / T" in err()
    assert h.syg_gl_project_f32(p, None, p, 1, 0, 0.0, p, None, None, None) == -1 and b"bad B / T" in err()
    for alpha in (0.5, -0.01, float("nan")):
        assert h.syg_gl_project_f32(p, p, p, 1, 2, alpha, p, None, None, None) == -1 and b"alpha" in err()
    d = h.syg_inv_dense_f32
    assert d(None, 1, 4, 4, p, 4, 0, 1.0, 0, 1.0, p, 0, None) == -1 and b"null pointer" in err()
    assert d(p, 1, 4, 4, None, 4, 0, 1.0, 0, 1.0, p, 0, None) == -1 and b"null pointer" in err()
    assert d(p, 1, 4, 4, p, 4, 0, 1.0, 0, 1.0, None, 0, None) == -1 and b"null pointer" in err()
    for B, M, T, F in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 4097, 4, 4), (1, 4, 4, 65537)):
        assert d(p, B, M, T, p, F, 0, 1.0, 0, 1.0, p, 0, None) == -1 and b"bad B / M / T / F" in err()
    assert d(p, 1, 4, 4, p, 4, 2, 1.0, 0, 1.0, p, 0, None) == -1 and b"pre is 0 or 1" in err()
    assert d(p, 1, 4, 4, p, 4, 0, 1.0, 3, 1.0, p, 0, None) == -1 and b"post 0, 1 or 2" in err()
    assert d(p, 1, 4, 4, p, 4, 0, 1.0, 0, 1.0, p, 2, None) == -1 and b"out_mel_major 0 or 1" in err()
    assert d(p, 1, 4, 4, p, 4, 1, 0.0, 0, 1.0, p, 0, None) == -1 and b"pre_ref must be positive" in err()
    assert d(p, 1, 4, 4, p, 4, 0, 1.0, 1, float("inf"), p, 0, None) == -1 and b"post_arg" in err()
    assert d(p, 1, 4, 4, p, 4, 0, 1.0, 2, -1.0, p, 0, None) == -1 and b"post_arg" in err()


def test_griffinlim_refuses_without_a_device():
    from sygnals_amd import ops
    S = torch.ones(2, 5, 1025)
    for momentum in (1.0, -0.1, 1.5, float("nan"), None):
        with pytest.raises(ValueError, match="momentum must be in \\[0, 1\\)"):
            ops.griffinlim(S, momentum=momentum)
    for n_iter in (-1, 2.5, True):
        with pytest.raises(ValueError, match="n_iter must be a non-negative integer"):
            ops.griffinlim(S, n_iter=n_iter)
    with pytest.raises(ValueError, match="init must be 'random' or None"):
        ops.griffinlim(S, init="zeros")
    with pytest.raises(ValueError, match="T=1 frames give the default length"):
        ops.griffinlim(torch.ones(2, 1, 1025))
    with pytest.raises(ValueError, match="length=100 frames to 1 frames, S has 5"):
        ops.griffinlim(S, length=100)
    with pytest.raises(ValueError, match="length=0 "):
        ops.griffinlim(torch.ones(2, 1, 1025), length=0)
    for bad in (torch.ones(2, 5, 1024), torch.ones(5, 1025), torch.ones(2, 5, 1025, dtype=torch.float64), np.ones((2, 5, 1025))):
        with pytest.raises(ValueError, match="S must be a float32 tensor \\[B, T, 1025\\]"):
            ops.griffinlim(bad)
    with pytest.raises(ValueError, match="empty input"):
        ops.griffinlim(torch.ones(0, 5, 1025))
    with pytest.raises(ValueError, match="angles must be a float32 tensor \\[2, 5, 1025, 2\\]"):
        ops.griffinlim(S, angles=torch.ones(2, 5, 1025))
    with pytest.raises(ValueError, match="angles must be a float32 tensor \\[2, 5, 1025, 2\\]"):
        ops.griffinlim(S, angles=torch.ones(3, 5, 1025, 2))
    for chunk in (0, -1, 1.5):
        with pytest.raises(ValueError, match="chunk must be a positive integer or None"):
            ops.griffinlim(S, chunk=chunk)
    with pytest.raises(ValueError):
        ops.griffinlim(S, seed=-1)


def test_projection_refuses_without_a_device():
    from sygnals_amd import ops
    S, Rr = torch.ones(2, 5, 1025), torch.ones(2, 5, 1025, 2)
    f = ops.gl_project
    with pytest.raises(ValueError, match="alpha"):
        f(Rr, S, None, 0.5)
    with pytest.raises(ValueError, match="R must be a float32 tensor"):
        f(None, S)
    with pytest.raises(ValueError, match="R must be a float32 tensor \\[2, 5, 1025, 2\\]"):
        f(torch.ones(2, 4, 1025, 2), S)
    with pytest.raises(ValueError, match="P must be a float32 tensor \\[2, 5, 1025, 2\\]"):
        f(Rr, S, torch.ones(1, 5, 1025, 2))
    with pytest.raises(ValueError, match="S must be a float32 tensor \\[B, T, 1025\\]"):
        f(Rr, torch.ones(2, 5, 1025, 2))
    assert ops.gl_alpha(0.99) == R.alpha_of(0.99) == float(np.float32(0.99 / 1.99)) and ops.gl_alpha(0) == 0.0


def test_inversions_refuse_without_a_device():
    from sygnals_amd import ops
    mel, mfcc = torch.ones(2, 128, 5), torch.ones(2, 13, 5)
    for kw in (dict(n_fft=1024), dict(n_fft=4096)):
        with pytest.raises(ValueError, match="only n_fft=2048, window='hann', win_length=2048, hop_length=512 and center=True"):
            ops.mel_to_stft(mel, **kw)
    for power in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="power must be positive and finite"):
            ops.mel_to_stft(mel, power=power)
    with pytest.raises(ValueError, match="mel must be a float32 tensor \\[B, n_mels, T\\]"):
        ops.mel_to_stft(torch.ones(128, 5))
    with pytest.raises(ValueError, match="n_mels=1026 must be in \\[1, 1025\\]"):
        ops.mel_to_stft(torch.ones(1, 1026, 2))
    with pytest.raises(ValueError, match="n_mfcc=13 must be in \\[1, n_mels=12\\]"):
        ops.mfcc_to_mel(mfcc, n_mels=12)
    for kw in (dict(norm=None), dict(dct_type=1), dict(dct_type=4)):
        with pytest.raises(ValueError, match="only norm='ortho' with dct_type 2 or 3 is served"):
            ops.mfcc_to_mel(mfcc, **kw)
    with pytest.raises(ValueError, match="ref must be positive and finite"):
        ops.mfcc_to_mel(mfcc, ref=0.0)
    with pytest.raises(ValueError, match="lifter=-1"):
        ops.mfcc_to_mel(mfcc, lifter=-1)
    # 1 + (lifter / 2) sin(pi n / lifter) = 0 at n = 3 lifter / 2 once lifter = 2: a weight that cannot be divided out
    assert 1.0 + (2.0 / 2.0) * np.sin(np.pi * 3 / 2.0) == 0.0
    with pytest.raises(ValueError, match="lifter=2.0 has a zero weight"):
        ops.mfcc_to_mel(mfcc, lifter=2.0)
    with pytest.raises(ValueError, match="post must be None, 'root' or 'db'"):
        ops.inv_dense(mel, torch.ones(4, 128), post="sqrt")
    with pytest.raises(ValueError, match="pre_ref must be positive and finite"):
        ops.inv_dense(mel, torch.ones(4, 128), pre_ref=0.0)


def test_mirrors_refuse_without_a_device():
    from sygnals_amd.core.features import inverse as IV
    S = np.ones((1025, 5))
    for kw in (dict(n_fft=1024), dict(hop_length=256), dict(win_length=1024), dict(window="hamming"), dict(center=False)):
        with pytest.raises(ValueError, match="only n_fft=2048, window='hann', win_length=2048, hop_length=512 and center=True"):
            IV.griffinlim(S, **kw)
        with pytest.raises(ValueError, match="only n_fft=2048"):
            IV.griffinlim_batch(torch.ones(1, 5, 1025), **kw)
    with pytest.raises(ValueError, match="S must be a real matrix \\[1025, T\\]"):
        IV.griffinlim(np.ones((5, 1025)))
    with pytest.raises(ValueError, match="S must be a real matrix"):
        IV.griffinlim(np.ones((1025, 5), dtype=np.complex64))
    with pytest.raises(ValueError, match="momentum must be in"):
        IV.griffinlim(S, momentum=1.0)
    with pytest.raises(ValueError, match="M must be a real matrix"):
        IV.mel_to_stft(np.ones(5))
    with pytest.raises(ValueError, match="only n_fft=2048"):
        IV.mel_to_audio(np.ones((128, 5)), n_fft=512)
    with pytest.raises(ValueError, match="only norm='ortho'"):
        IV.mfcc_to_mel(np.ones((13, 5)), norm=None)
    with pytest.raises(ValueError, match="zero weight"):
        IV.mfcc_to_audio(np.ones((13, 5)), lifter=2.0)


def test_host_tables_are_the_restatements():
    from sygnals_amd import _tables as T, ops
    W = ops.mel_pinv_table(22050, 2048, 128)
    B = T.mel_filterbank(22050, 2048, 128).astype(np.float64)
    assert W.shape == (1025, 128) and W.dtype == np.float32
    assert np.allclose(W, R.mel_pinv(B), atol=2e-6)
    assert np.allclose(B @ W.astype(np.float64), np.eye(128), atol=1e-5)          # full row rank: B B+ = I
    # mixed signs, the largest entry far above 1: why the bound of the device test is absolute (sum |W| |x|), not relative
    assert (W < 0).mean() > 0.3 and 10.0 < np.abs(W).max() < 30.0
    assert np.allclose(ops.idct_lifter_table(13, 128, 2, "ortho", 22), R.idct_matrix(13, 128, 2, 22), atol=2e-7)
    assert ops.idct_lifter_table(128, 128).shape == (128, 128)


def test_plugin_registers_the_inversions():
    from sygnals_amd.core.features import inverse as IV
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.f = {}

        def add_feature(self, name, fn):
            self.f[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_feature_extractors(r)
    for name in ("griffinlim", "mel_to_stft", "mel_to_audio", "mfcc_to_mel", "mfcc_to_audio"):
        assert r.f[name] is getattr(IV, name)
    assert "integrated_loudness" in r.f and "mfcc" in r.f
    assert set(IV.__all__) == {n + s for n in ("griffinlim", "mel_to_stft", "mel_to_audio", "mfcc_to_mel", "mfcc_to_audio")
                               for s in ("", "_batch")}
