"""The NMF entries of the C ABI are declared, bound and exported, size their workspace, and refuse bad arguments before
device work; the operators and core.decompose refuse what is not served without a device; the plugin registers the public
functions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_nmf_constants", "syg_nmf_work_bytes", "syg_nmf_f32", "syg_nmf_divergence_f32", "syg_nmf_masks_f32"]


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


def test_constants_and_work_bytes(h):
    from sygnals_amd import ops
    k = ops.nmf_constants()
    assert k == dict(max_components=64, max_bins=2049, max_groups=64, a_tile_frames=16, a_chunk_bins=64, c_tile_bins=64,
                     c_chunk_frames=32, sums_chunk=64, mfma_min_components=k["mfma_min_components"], eps=float(np.finfo(np.float32).eps))
    assert 1 <= k["mfma_min_components"] <= 65                   # 65: the MFMA form is never taken by default
    assert h.syg_nmf_constants(9) == -1 and h.syg_nmf_constants(-1) == -1
    wb = h.syg_nmf_work_bytes
    assert wb(1, 1, 1, 1) == 8                                   # (K K + K) floats, or one float64 partial
    assert wb(3, 65, 1025, 2) == 3 * 9 * 8                       # ceil(65 * 1025 / 8192) = 9 partials beat 6 floats
    assert wb(3, 65, 1025, 8) == 3 * 72 * 4
    assert wb(3, 5, 33, 64) == 3 * (64 * 64 + 64) * 4
    assert wb(1, 10000, 2049, 2) == 256 * 8                      # capped at 256 workgroups a clip
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 2050, 1), (1, 1, 1, 65), (1 << 30, 1 << 20, 2, 1)):
        assert wb(*bad) == -1 and b"served are" in h.syg_last_error()


def test_entries_refuse_before_device_work(h, p):
    err = h.syg_last_error
    f = h.syg_nmf_f32
    for args in ((None, 1, 2, 3, 2, p, p, 0, 1, 0, 1, 1, -1, p), (p, 1, 2, 3, 2, None, p, 0, 1, 0, 1, 1, -1, p),
                 (p, 1, 2, 3, 2, p, None, 0, 1, 0, 1, 1, -1, p), (p, 1, 2, 3, 2, p, p, 0, 1, 0, 1, 1, -1, None)):
        assert f(*args, None) == -1 and b"null pointer" in err()
    for B, T, F, K in ((0, 2, 3, 2), (1, 0, 3, 2), (1, 2, 0, 2), (1, 2, 3, 0), (1, 2, 2050, 2), (1, 2, 3, 65)):
        assert f(p, B, T, F, K, p, p, 0, 1, 0, 1, 1, -1, p, None) == -1 and b"served are" in err()
    for loss in (-1, 2, 3):
        assert f(p, 1, 2, 3, 2, p, p, 0, 1, loss, 1, 1, -1, p, None) == -1 and b"Itakura-Saito and other beta are not served" in err()
    assert f(p, 1, 2, 3, 2, p, p, 0, -1, 0, 1, 1, -1, p, None) == -1 and b"n_iter" in err()
    assert f(p, 1, 2, 3, 2, p, p, 0, 1, 0, 2, 1, -1, p, None) == -1 and b"are 0 or 1" in err()
    assert f(p, 3, 2, 3, 2, p, p, 1, 1, 0, 1, 1, -1, p, None) == -1 and b"shared dictionary" in err()
    for form in (-2, 2):
        assert f(p, 1, 2, 3, 2, p, p, 0, 1, 0, 1, 1, form, p, None) == -1 and b"form must be" in err()
    d = h.syg_nmf_divergence_f32
    assert d(p, p, p, 0, 1, 2, 3, 2, 0, None, p, None) == -1 and b"null pointer" in err()
    assert d(p, p, p, 0, 1, 2, 3, 2, 0, p, None, None) == -1 and b"null pointer" in err()
    assert d(p, p, p, 0, 1, 2, 3, 65, 0, p, p, None) == -1 and b"served are" in err()
    assert d(p, p, p, 0, 1, 2, 3, 2, 2, p, p, None) == -1 and b"loss" in err()
    m = h.syg_nmf_masks_f32
    assert m(p, p, p, 0, None, 1, 2, 3, 2, 1, p, None) == -1 and b"null pointer" in err()
    assert m(p, p, p, 0, p, 1, 2, 3, 2, 1, None, None) == -1 and b"null pointer" in err()
    assert m(p, p, p, 0, p, 1, 2, 2050, 2, 1, p, None) == -1 and b"served are" in err()
    for ng in (0, 65):
        assert m(p, p, p, 0, p, 1, 2, 3, 2, ng, p, None) == -1 and b"n_groups must be in [1, 64]" in err()


def test_nmf_refuses_without_a_device():
    from sygnals_amd import ops
    V = torch.ones(2, 5, 33)
    for beta in ("itakura-saito", 0, 0.5, 3, None, True):
        with pytest.raises(ValueError, match="is not served .*served: beta_loss 'frobenius' \\(2\\) or 'kullback-leibler' \\(1\\)"):
            ops.nmf(V, 3, beta_loss=beta)
    with pytest.raises(ValueError, match="solver='cd' is not served \\(coordinate descent is sequential"):
        ops.nmf(V, 3, solver="cd")
    for init in ("nndsvd", "nndsvda", "nndsvdar"):
        with pytest.raises(ValueError, match="need an SVD"):
            ops.nmf(V, 3, init=init)
    for n_iter in (-1, 2.5, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="n_iter must be a non-negative integer"):
            ops.nmf(V, 3, n_iter=n_iter)
    for K in (0, 65, -1, 2.0):
        with pytest.raises(ValueError, match="must be an integer in \\[1, 64\\]"):
            ops.nmf(V, K)
    for form in ("auto", 1, "MFMA"):
        with pytest.raises(ValueError, match="form must be None, 'fma' or 'mfma'"):
            ops.nmf(V, 3, form=form)
    with pytest.raises(ValueError, match="n_components is needed"):
        ops.nmf(V)
    for bad in (torch.ones(5, 33), torch.ones(2, 5, 33, dtype=torch.float64), np.ones((2, 5, 33), np.float32)):
        with pytest.raises(ValueError, match="V must be a float32 tensor \\[B, T, F\\]"):
            ops.nmf(bad, 3)
    for empty in (torch.ones(0, 5, 33), torch.ones(2, 0, 33), torch.ones(2, 5, 0)):
        with pytest.raises(ValueError, match="empty input"):
            ops.nmf(empty, 3)
    with pytest.raises(ValueError, match="F=2050 bins must be in \\[1, 2049\\]"):
        ops.nmf(torch.ones(1, 2, 2050), 3)
    with pytest.raises(ValueError, match="A must be a float32 tensor \\[2, 5, 3\\]"):
        ops.nmf(V, 3, A0=torch.ones(2, 4, 3))
    with pytest.raises(ValueError, match="A must be a float32 tensor \\[2, 5, 3\\]"):
        ops.nmf(V, 3, A0=torch.ones(1, 5, 3))
    with pytest.raises(ValueError, match="C must be a float32 tensor \\[2, 3, 33\\] or \\[1, 3, 33\\]"):
        ops.nmf(V, 3, C0=torch.ones(2, 3, 32))
    with pytest.raises(ValueError, match="C must be a float32 tensor"):
        ops.nmf(V, A0=torch.ones(2, 5, 3), C0=torch.ones(2, 4, 33))
    with pytest.raises(ValueError, match="shared dictionary C0 \\[1, 3, 33\\] cannot be updated"):
        ops.nmf(V, C0=torch.ones(1, 3, 33))
    with pytest.raises(ValueError):
        ops.nmf(V, 3, seed=-1)
    with pytest.raises(ValueError, match="is not served"):
        ops.nmf_divergence(V, torch.ones(2, 5, 3), torch.ones(2, 3, 33), "itakura-saito")
    with pytest.raises(ValueError, match="A must be a float32 tensor \\[2, 5, 3\\]"):
        ops.nmf_divergence(V, torch.ones(2, 5, 3, 1), torch.ones(2, 3, 33))
    D = torch.ones(2, 5, 33, 2)
    with pytest.raises(ValueError, match="D must be a float32 tensor \\[B, T, F, 2\\]"):
        ops.nmf_masks(V, torch.ones(2, 5, 3), torch.ones(2, 3, 33))
    with pytest.raises(ValueError, match="G must be a float32 tensor \\[n_groups, 3\\]"):
        ops.nmf_masks(D, torch.ones(2, 5, 3), torch.ones(2, 3, 33), torch.ones(2, 4))
    with pytest.raises(ValueError, match="n_groups=65 must be in \\[1, 64\\]"):
        ops.nmf_masks(D, torch.ones(2, 5, 3), torch.ones(2, 3, 33), torch.ones(65, 3))


def test_decompose_refuses_without_a_device():
    from sygnals_amd.core import decompose as DC
    S = np.ones((33, 5))
    with pytest.raises(ValueError, match="S must be a real non-negative matrix \\[F, T\\]"):
        DC.decompose(np.ones(5), 2)
    with pytest.raises(ValueError, match="S must be a real non-negative matrix"):
        DC.decompose(np.ones((33, 5), dtype=np.complex64), 2)
    with pytest.raises(ValueError, match="non-negative and finite"):
        DC.decompose(-S, 2)
    with pytest.raises(ValueError, match="is not served"):
        DC.decompose(S, 2, beta_loss="itakura-saito")
    with pytest.raises(ValueError, match="must be an integer in \\[1, 64\\]"):
        DC.decompose(S, 65)
    with pytest.raises(ValueError, match="must be an integer in \\[1, 64\\]"):
        DC.decompose(S)
    with pytest.raises(ValueError, match="n_iter must be a non-negative integer"):
        DC.decompose(S, 2, n_iter=-3)
    with pytest.raises(ValueError, match="fit=False needs components"):
        DC.decompose(S, 2, fit=False)
    with pytest.raises(ValueError, match="components must be a real matrix \\[33, K\\]"):
        DC.decompose(S, 2, components=np.ones((32, 2)))
    with pytest.raises(ValueError, match="sort=True reorders learned components"):
        DC.decompose(S, 2, fit=False, components=np.ones((33, 2)), sort=True)
    with pytest.raises(ValueError, match="fit=False needs components"):
        DC.decompose_batch(torch.ones(1, 5, 33), 2, fit=False)
    with pytest.raises(ValueError, match="y must be one real clip"):
        DC.separate_components(np.ones((2, 100)), 22050, 2)
    with pytest.raises(ValueError, match="n_components=0 must be an integer in \\[1, 64\\]"):
        DC.separate_components(np.ones(100), 22050, 0)
    with pytest.raises(ValueError, match="y must be a float32 tensor \\[B, L\\]"):
        DC.separate_components_batch(torch.ones(100), 2)
    with pytest.raises(ValueError, match="is not served"):
        DC.separate_components_batch(torch.ones(1, 100), 2, beta_loss=0)


def test_plugin_registers_the_decomposition():
    from sygnals_amd.core import decompose as DC
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.f = {}

        def add_feature(self, name, fn):
            self.f[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_feature_extractors(r)
    assert r.f["decompose"] is DC.decompose and r.f["separate_components"] is DC.separate_components
    assert "griffinlim" in r.f and "mfcc" in r.f
    assert set(DC.__all__) == {"decompose", "decompose_batch", "separate_components", "separate_components_batch"}
