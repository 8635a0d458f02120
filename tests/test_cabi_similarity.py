"""The self-similarity entries of the C ABI are declared, bound and exported, size their workspace, and refuse bad
arguments before device work; the operators, core.similarity and core.decompose refuse what is not served without a
device; the plugin registers the public functions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_sim_k_max", "syg_sim_knn_work_bytes", "syg_sim_knn_f32", "syg_sim_dense_f32", "syg_nn_filter_f32", "syg_repet_masks_f32"]


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
    assert h.syg_sim_k_max() == 256 == ops.K_MAX
    k = ops.similarity_constants()
    assert k == dict(k_max=256, metrics=("euclidean", "sqeuclidean", "cosine"), modes=("connectivity", "distance", "affinity"),
                     aggregates=("mean", "average", "median"))
    wb = h.syg_sim_knn_work_bytes
    assert wb(1, 1, 1, 0) == 8                                   # one float, rounded up to 8 bytes
    assert wb(3, 65, 40, 0) == 784                               # the squared norms of X alone: 780 bytes, rounded up
    assert wb(3, 65, 40, 1) == 1264                              # and of Y: 3 (65 + 40) floats, rounded up
    assert wb(1, 7750, 7750, 0) == 7750 * 4
    for bad in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 1), (1, 1, 1, 2), (1, (1 << 30) + 1, 1, 0), (1 << 20, 1 << 30, 1, 0)):
        assert wb(*bad) == -1 and b"served are" in h.syg_last_error()


def knn_args(p, **kw):
    a = dict(X=p, Y=None, B=1, T=5, Ty=5, D=3, ldx=3, ldy=3, bsx=15, bsy=15, x_len=None, y_len=None, k=2, width=1, metric=0,
             idx=p, dist=p, count=p, work=p)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_knn_refuses_before_device_work(h, p):
    err, f = h.syg_last_error, h.syg_sim_knn_f32
    for name in ("X", "idx", "dist", "count", "work"):
        assert f(*knn_args(p, **{name: None})) == -1 and b"null pointer" in err()
    for kw in (dict(B=0), dict(T=0), dict(D=0), dict(Y=p, Ty=0), dict(T=(1 << 30) + 1)):
        assert f(*knn_args(p, **kw)) == -1 and b"served are" in err()
    for k in (0, 257, -1):
        assert f(*knn_args(p, k=k)) == -1 and b"k must be in [1, 256]" in err()
    for w in (0, -3):
        assert f(*knn_args(p, width=w)) == -1 and b"width must be in" in err()
    assert f(*knn_args(p, Y=p, width=2)) == -1 and b"with Y it must be 1" in err()
    for m in (-1, 3, 7):
        assert f(*knn_args(p, metric=m)) == -1 and b"cityblock has no contraction form" in err()
    assert f(*knn_args(p, ldx=2)) == -1 and b"row stride is smaller than D=3" in err()
    assert f(*knn_args(p, Y=p, ldy=2)) == -1 and b"row stride is smaller than D=3" in err()
    assert f(*knn_args(p, bsx=-1)) == -1 and b"negative batch stride" in err()
    assert f(*knn_args(p, y_len=p)) == -1 and b"y_len needs Y" in err()


def test_dense_filter_and_masks_refuse_before_device_work(h, p):
    err = h.syg_last_error
    d = h.syg_sim_dense_f32                    # idx, dist, count, B, T, Ty, k, mode, sym, self, bandwidth, out, rowmax
    assert d(None, p, p, 1, 4, 4, 2, 0, 0, 0, None, p, None, None) == -1 and b"null pointer" in err()
    assert d(p, p, p, 1, 4, 4, 2, 0, 0, 0, None, None, None, None) == -1 and b"null pointer" in err()
    assert d(p, p, p, 1, 0, 4, 2, 0, 0, 0, None, p, None, None) == -1 and b"served are" in err()
    for k in (0, 257):
        assert d(p, p, p, 1, 4, 4, k, 0, 0, 0, None, p, None, None) == -1 and b"k must be in [1, 256]" in err()
    for mode in (-1, 3):
        assert d(p, p, p, 1, 4, 4, 2, mode, 0, 0, None, p, None, None) == -1 and b"mode must be" in err()
    assert d(p, p, p, 1, 4, 4, 2, 0, 2, 0, None, p, None, None) == -1 and b"are 0 or 1" in err()
    assert d(p, p, p, 1, 4, 5, 2, 0, 1, 0, None, p, None, None) == -1 and b"square matrix" in err()
    assert d(p, p, p, 1, 4, 5, 2, 0, 0, 1, None, p, None, None) == -1 and b"square matrix" in err()
    assert d(p, p, p, 1, 4, 4, 2, 2, 0, 0, None, p, None, None) == -1 and b"needs bandwidth" in err()
    n = h.syg_nn_filter_f32                    # S, B, T, F, lds, bss, idx, count, k, weights, bandwidth, aggregate, out
    assert n(None, 1, 4, 3, 3, 12, p, p, 2, None, None, 0, p, None) == -1 and b"null pointer" in err()
    assert n(p, 1, 4, 3, 3, 12, p, p, 2, None, None, 0, None, None) == -1 and b"null pointer" in err()
    assert n(p, 1, 4, 0, 3, 12, p, p, 2, None, None, 0, p, None) == -1 and b"served are" in err()
    assert n(p, 1, 4, 3, 3, 12, p, p, 257, None, None, 0, p, None) == -1 and b"k must be in [1, 256]" in err()
    for agg in (-1, 3):
        assert n(p, 1, 4, 3, 3, 12, p, p, 2, None, None, agg, p, None) == -1 and b"aggregate must be" in err()
    assert n(p, 1, 4, 3, 3, 12, p, p, 2, None, None, 1, p, None) == -1 and b"needs weights" in err()
    assert n(p, 1, 4, 3, 2, 12, p, p, 2, None, None, 0, p, None) == -1 and b"row stride is smaller than F=3" in err()
    r = h.syg_repet_masks_f32                  # S, Sf, n, margin_b, margin_f, power, mask_f, mask_b
    assert r(p, None, 4, 2.0, 10.0, 2.0, p, p, None) == -1 and b"null pointer" in err()
    assert r(p, p, 0, 2.0, 10.0, 2.0, p, p, None) == -1 and b"n must be in" in err()
    for bad in ((0.0, 10.0, 2.0), (2.0, -1.0, 2.0), (2.0, 10.0, 0.0), (2.0, 10.0, float("inf")), (float("nan"), 10.0, 2.0)):
        assert r(p, p, 4, *bad, p, p, None) == -1 and b"must be positive and finite" in err()


def test_operators_refuse_without_a_device():
    from sygnals_amd import ops
    X = torch.ones(2, 9, 4)
    for metric in ("cityblock", "manhattan", "chebyshev", None, 2):
        with pytest.raises(ValueError, match="is not served .*served: 'euclidean', 'sqeuclidean', 'cosine'"):
            ops.sim_knn(X, metric=metric)
    for k in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="k=.* must be an integer in \\[1, 256\\]"):
            ops.sim_knn(X, k=k)
    for w in (0, -1, 1.5):
        with pytest.raises(ValueError, match="width=.* must be an integer in"):
            ops.sim_knn(X, width=w)
    with pytest.raises(ValueError, match="with Y every frame is a candidate"):
        ops.sim_knn(X, torch.ones(2, 5, 4), width=2)
    with pytest.raises(ValueError, match="Y \\[2, 5, 3\\] must be \\[2, T', 4\\] or \\[1, T', 4\\]"):
        ops.sim_knn(X, torch.ones(2, 5, 3))
    with pytest.raises(ValueError, match="must be \\[2, T', 4\\]"):
        ops.sim_knn(X, torch.ones(3, 5, 4))
    with pytest.raises(ValueError, match="y_len needs Y"):
        ops.sim_knn(X, y_len=[1, 2])
    for bad in (torch.ones(9, 4), torch.ones(2, 9, 4, dtype=torch.float64), np.ones((2, 9, 4), np.float32)):
        with pytest.raises(ValueError, match="X must be a float32 tensor \\[B, T, D\\]"):
            ops.sim_knn(bad)
    with pytest.raises(ValueError, match="empty input"):
        ops.sim_knn(torch.ones(2, 0, 4))
    with pytest.raises(ValueError, match="mode='sparse' is not served"):
        ops.recurrence_matrix(X, mode="sparse")
    with pytest.raises(ValueError, match="sym and self apply to self-similarity"):
        ops.recurrence_matrix(X, torch.ones(2, 5, 4), sym=True)
    with pytest.raises(ValueError, match="bandwidth applies to mode='affinity'"):
        ops.recurrence_matrix(X, bandwidth=1.0)
    idx, count = torch.zeros(2, 9, 3, dtype=torch.int32), torch.ones(2, 9, dtype=torch.int32)
    for agg in ("max", "min", None, np.mean):
        with pytest.raises(ValueError, match="aggregate=.* is not served; served: 'mean', 'average', 'median'"):
            ops.nn_filter(X, idx, count, aggregate=agg)
    with pytest.raises(ValueError, match="idx must be an int32 tensor \\[B, T, k\\]"):
        ops.nn_filter(X, idx.long(), count)
    with pytest.raises(ValueError, match="must be \\[2, 9, k\\]"):
        ops.nn_filter(X, idx[:, :8], count[:, :8])
    with pytest.raises(ValueError, match="count must be an int32 tensor \\[2, 9\\]"):
        ops.nn_filter(X, idx, count[:1])
    with pytest.raises(ValueError, match="aggregate='average' needs weights"):
        ops.nn_filter(X, idx, count, aggregate="average")
    with pytest.raises(ValueError, match="weights must be a float32 tensor \\[2, 9, 3\\]"):
        ops.nn_filter(X, idx, count, torch.ones(2, 9, 2), "average")
    with pytest.raises(ValueError, match="apply to aggregate='average'"):
        ops.nn_filter(X, idx, count, torch.ones(2, 9, 3), "median")
    with pytest.raises(ValueError, match="k in \\[1, 256\\]"):
        ops.nn_filter(X, torch.zeros(2, 9, 257, dtype=torch.int32), count)
    for kw in (dict(margin_b=0), dict(margin_f=-1.0), dict(power=0.0), dict(power=float("inf")), dict(margin_b=None)):
        with pytest.raises(ValueError, match="must be a positive finite number"):
            ops.repet_masks(X, X, **kw)
    with pytest.raises(ValueError, match="Sf must be a float32 tensor \\[2, 9, 4\\]"):
        ops.repet_masks(X, torch.ones(2, 9, 5))


def test_core_functions_refuse_without_a_device():
    from sygnals_amd.core import decompose as DC
    from sygnals_amd.core import similarity as SM
    data = np.ones((4, 9))
    with pytest.raises(ValueError, match="data must be a real matrix \\[d, t\\]"):
        SM.recurrence_matrix(np.ones(9))
    with pytest.raises(ValueError, match="metric='cityblock' is not served"):
        SM.recurrence_matrix(data, metric="cityblock")
    with pytest.raises(ValueError, match="sparse outputs are not served"):
        SM.recurrence_matrix(data, sparse=True)
    with pytest.raises(ValueError, match="k=300 must be an integer in \\[1, 256\\]"):
        SM.recurrence_matrix(data, k=300)
    with pytest.raises(ValueError, match="width=0 must be an integer"):
        SM.recurrence_matrix(data, width=0)
    with pytest.raises(ValueError, match="mode='lag' is not served"):
        SM.cross_similarity(data, data, mode="lag")
    with pytest.raises(ValueError, match="same number of features"):
        SM.cross_similarity(data, np.ones((5, 9)))
    with pytest.raises(ValueError, match="S must be a real matrix \\[F, T\\]"):
        DC.nn_filter(np.ones(9))
    with pytest.raises(ValueError, match="aggregate=.* is not served"):
        DC.nn_filter(data, aggregate=np.max)
    with pytest.raises(ValueError, match="recurrence arguments served are k, width, metric and bandwidth"):
        DC.nn_filter(data, sym=True)
    with pytest.raises(ValueError, match="rec must be a real matrix \\[9, 9\\]"):
        DC.nn_filter(data, rec=np.ones((4, 4)))
    with pytest.raises(ValueError, match="y must be one real clip"):
        DC.separate_repeating(np.ones((2, 100)))
    for kw in (dict(width_seconds=0), dict(margin_background=-1), dict(margin_foreground=0), dict(power=0)):
        with pytest.raises(ValueError, match="must be a positive finite number"):
            DC.separate_repeating(np.ones(100), 22050, **kw)
    with pytest.raises(ValueError, match="metric='cityblock' is not served"):
        DC.separate_repeating(np.ones(100), 22050, metric="cityblock")
    with pytest.raises(ValueError, match="y must be a float32 tensor \\[B, L\\]"):
        DC.separate_repeating_batch(torch.ones(100))
    with pytest.raises(ValueError, match="width=0 must be an integer"):
        DC.separate_repeating_batch(torch.ones(1, 100), width=0)


def test_plugin_registers_the_similarity_functions():
    from sygnals_amd.core import decompose as DC
    from sygnals_amd.core import similarity as SM
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.f = {}

        def add_feature(self, name, fn):
            self.f[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_feature_extractors(r)
    assert r.f["nn_filter"] is DC.nn_filter and r.f["separate_repeating"] is DC.separate_repeating
    assert r.f["recurrence_matrix"] is SM.recurrence_matrix and r.f["decompose"] is DC.decompose
    assert set(SM.__all__) == {"recurrence_matrix", "recurrence_matrix_batch", "cross_similarity", "cross_similarity_batch"}
