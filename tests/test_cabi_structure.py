"""The structure entries of the C ABI are declared, bound and exported, publish their constants, size their workspace and
refuse bad arguments before device work; the operators and core.structure refuse what is not served without a device;
the plugin registers the public functions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_structure_constants", "syg_lag_shear_f32", "syg_path_enhance_f32", "syg_diag_median_f32", "syg_agglomerative_work_bytes",
       "syg_agglomerative_f32", "syg_segment_sync_f32"]


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
    k = ops.structure_constants()
    assert k["agg_t_max"] == 8192 >= 7750 and k["median_w_max"] == 63 and (k["path_tile_rows"], k["path_tile_cols"]) == (16, 64)
    assert k["path_span_max"] == 160 and k["shear_t_max"] == 32768
    assert k["modes"] == ("reflect", "mirror", "nearest", "wrap", "grid-wrap", "constant", "grid-constant")
    assert k["aggregates"] == ("mean", "max", "min")
    assert h.syg_structure_constants(6) == -1 and h.syg_structure_constants(-1) == -1
    wb = h.syg_agglomerative_work_bytes
    assert wb(1, 1, 1) == 8 and wb(64, 431, 12) == 64 * 431 * 12 * 8 and wb(1, 7750, 12) == 7750 * 96
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 20, 1 << 20, 1), (1, 1, (1 << 20) + 1), (1 << 10, 1 << 20, 1 << 10)):
        assert wb(*bad) == -1 and b"served are" in h.syg_last_error()


def test_shear_and_median_refuse_before_device_work(h, p):
    err, f = h.syg_last_error, h.syg_lag_shear_f32        # in, B, t, ldi, bsi, inverse, axis, pad, out
    assert f(None, 1, 4, 4, 16, 0, 1, 1, p, None) == -1 and b"null pointer" in err()
    assert f(p, 1, 4, 4, 16, 0, 1, 1, None, None) == -1 and b"null pointer" in err()
    for B, t in ((0, 4), (1, 0), (1, 32769), (1 << 30, 4096)):
        assert f(p, B, t, t, t * t, 0, 1, 1, p, None) == -1 and b"served are" in err()
    for flags in ((2, 1, 1), (0, -1, 1), (0, 1, 3)):
        assert f(p, 1, 4, 4, 16, *flags, p, None) == -1 and b"are 0 or 1" in err()
    assert f(p, 1, 4, 3, 16, 0, 1, 1, p, None) == -1 and b"row stride is smaller" in err()
    assert f(p, 1, 4, 4, 16, 1, 0, 1, p, None) == -1 and b"row stride is smaller" in err()      # the padded rows are 8 long
    assert f(p, 1, 4, 4, -1, 0, 1, 1, p, None) == -1 and b"batch stride negative" in err()
    m = h.syg_diag_median_f32                               # R, B, t, ldr, bsr, w, axis, pad, mode, cval, out
    assert m(None, 1, 4, 4, 16, 3, 1, 1, 0, 0.0, p, None) == -1 and b"null pointer" in err()
    assert m(p, 1, 0, 4, 16, 3, 1, 1, 0, 0.0, p, None) == -1 and b"served are" in err()
    for w in (0, 2, 64, 65, -3):
        assert m(p, 1, 4, 4, 16, w, 1, 1, 0, 0.0, p, None) == -1 and b"w must be odd and in [1, 63]" in err()
    assert m(p, 1, 4, 4, 16, 3, 2, 1, 0, 0.0, p, None) == -1 and b"are 0 or 1" in err()
    for mode in (-1, 5):
        assert m(p, 1, 4, 4, 16, 3, 1, 1, mode, 0.0, p, None) == -1 and b"mode must be SYG_BOUNDARY_REFLECT" in err()
    assert m(p, 1, 4, 4, 16, 3, 1, 1, 4, float("nan"), p, None) == -1 and b"cval must be finite" in err()
    assert m(p, 1, 4, 3, 16, 3, 1, 1, 0, 0.0, p, None) == -1 and b"row stride is smaller than t=4" in err()


def path_args(p, **kw):
    a = dict(R=p, B=1, T=5, Tc=4, ldr=4, bsr=20, taps=p, n_taps=9, fstart=p, n_filters=1, dr_min=-1, dr_max=1, dc_min=-1, dc_max=1,
             mode=0, cval=0.0, clip=1, out=p)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_path_enhance_refuses_before_device_work(h, p):
    err, f = h.syg_last_error, h.syg_path_enhance_f32
    for name in ("R", "taps", "fstart", "out"):
        assert f(*path_args(p, **{name: None})) == -1 and b"null pointer" in err()
    for kw in (dict(B=0), dict(T=0), dict(Tc=0), dict(T=(1 << 20) + 1)):
        assert f(*path_args(p, **kw)) == -1 and b"served are" in err()
    for kw in (dict(n_filters=0), dict(n_filters=4097), dict(n_taps=0)):
        assert f(*path_args(p, **kw)) == -1 and b"n_filters must be in" in err()
    for kw in (dict(dr_min=2), dict(dc_min=-80, dc_max=81), dict(dr_min=-100, dr_max=61)):
        assert f(*path_args(p, **kw)) == -1 and b"span at most 160" in err()
    assert f(*path_args(p, mode=5)) == -1 and b"mode must be" in err()
    assert f(*path_args(p, clip=2)) == -1 and b"clip is 0 or 1" in err()
    assert f(*path_args(p, cval=float("inf"))) == -1 and b"cval finite" in err()
    assert f(*path_args(p, ldr=3)) == -1 and b"row stride is smaller than T'=4" in err()


def agg_args(p, **kw):
    a = dict(X=p, B=2, T=9, D=3, ldx=3, bsx=27, offset=p, length=p, k=p, n_spans=2, max_len=9, k_max=4, bounds=p, count=p, work=p,
             work_bytes=2 * 9 * 3 * 8)
    a.update(kw)
    return tuple(a.values()) + (None,)


def test_agglomerative_and_sync_refuse_before_device_work(h, p):
    err, f = h.syg_last_error, h.syg_agglomerative_f32
    for name in ("X", "offset", "length", "k", "bounds", "count", "work"):
        assert f(*agg_args(p, **{name: None})) == -1 and b"null pointer" in err()
    for kw in (dict(B=0), dict(T=0), dict(D=0)):
        assert f(*agg_args(p, **kw)) == -1 and b"served are" in err()
    for n in (0, 19):
        assert f(*agg_args(p, n_spans=n)) == -1 and b"n_spans must be in" in err()
    for kw in (dict(max_len=0), dict(max_len=10), dict(T=9000, max_len=8193, work_bytes=1 << 40)):
        assert f(*agg_args(p, **kw)) == -1 and b"a span holds 1 to 8192 frames" in err()
    for km in (0, 10):
        assert f(*agg_args(p, k_max=km)) == -1 and b"k_max must be in" in err()
    assert f(*agg_args(p, ldx=2)) == -1 and b"frame stride is smaller than D=3" in err()
    assert f(*agg_args(p, work_bytes=431)) == -1 and b"workspace is too small" in err()
    s = h.syg_segment_sync_f32                   # X, B, T, D, ldx, bsx, edges, n_seg, edge_bs, aggregate, out
    assert s(None, 1, 9, 3, 3, 27, p, 2, 0, 0, p, None) == -1 and b"null pointer" in err()
    assert s(p, 1, 0, 3, 3, 27, p, 2, 0, 0, p, None) == -1 and b"served are" in err()
    for n in (0, 10):
        assert s(p, 1, 9, 3, 3, 27, p, n, 0, 0, p, None) == -1 and b"n_seg must be in" in err()
    assert s(p, 1, 9, 3, 3, 27, p, 2, 2, 0, p, None) == -1 and b"batch stride of edges" in err()
    for agg in (-1, 3):
        assert s(p, 1, 9, 3, 3, 27, p, 2, 0, agg, p, None) == -1 and b"median is not served" in err()
    assert s(p, 1, 9, 3, 2, 27, p, 2, 0, 0, p, None) == -1 and b"frame stride is smaller" in err()


def test_operators_refuse_without_a_device():
    from sygnals_amd import ops
    sq, rect, X = torch.ones(2, 6, 6), torch.ones(2, 6, 5), torch.ones(2, 9, 4)
    with pytest.raises(ValueError, match="rec must be square"):
        ops.recurrence_to_lag(rect)
    for bad in (torch.ones(6, 6), sq.double(), np.ones((1, 6, 6), np.float32)):
        with pytest.raises(ValueError, match="must be a float32 tensor \\[B, T, T'\\]"):
            ops.recurrence_to_lag(bad)
    for axis in (2, -2, None, True):
        with pytest.raises(ValueError, match="axis=.* must be -1"):
            ops.recurrence_to_lag(sq, axis=axis)
    with pytest.raises(ValueError, match="lag must be \\[t, t\\] or padded"):
        ops.lag_to_recurrence(torch.ones(1, 7, 3))
    with pytest.raises(ValueError, match="lag must be \\[t, t\\] or padded"):
        ops.lag_to_recurrence(torch.ones(1, 12, 6), axis=0)
    with pytest.raises(ValueError, match="empty input"):
        ops.path_enhance(torch.ones(1, 0, 4), 7)
    with pytest.raises(ValueError, match="mode='spline' is not served; served: 'reflect', 'mirror'"):
        ops.path_enhance(rect, 7, mode="spline")
    with pytest.raises(ValueError, match="min_ratio=3.0 cannot exceed max_ratio=2.0"):
        ops.path_enhance(rect, 7, min_ratio=3.0)
    with pytest.raises(ValueError, match="cval=.* must be a finite number"):
        ops.path_enhance(rect, 7, mode="constant", cval=float("nan"))
    with pytest.raises(ValueError, match="n=0 must be a positive integer"):
        ops.path_enhance(rect, 0)
    for w in (0, 2, 65, 3.0, True):
        with pytest.raises(ValueError, match="w=.* must be an odd integer in \\[1, 63\\]"):
            ops.diag_median(sq, w)
    with pytest.raises(ValueError, match="R must be square"):
        ops.diag_median(rect, 3)
    for k in (0, 10, [1, 10]):
        with pytest.raises(ValueError, match="k must be in \\[1, frames of the span\\]"):
            ops.agglomerative(X, k)
    with pytest.raises(ValueError, match="k must be an integer or a one-dimensional array of integers \\[2\\]"):
        ops.agglomerative(X, 2.5)
    with pytest.raises(ValueError, match="offset and length come together"):
        ops.agglomerative(X, 2, offset=[0])
    with pytest.raises(ValueError, match="lie inside one clip of 9 frames"):
        ops.agglomerative(X, 1, offset=[5], length=[5])
    with pytest.raises(ValueError, match="spans must not overlap"):
        ops.agglomerative(X, 1, offset=[0, 3], length=[4, 2])
    with pytest.raises(ValueError, match="a span of 9000 frames is above the served 8192 frames"):
        ops.agglomerative(torch.ones(1, 9000, 1), 2)
    with pytest.raises(ValueError, match="n_segments=0 must be an integer >= 1"):
        ops.subsegment(X, [3], 0)
    with pytest.raises(ValueError, match="negative frame index"):
        ops.subsegment(X, [3, -2])
    for agg in ("median", np.median):
        with pytest.raises(ValueError, match="aggregate='median' is not served; served: 'mean', 'max', 'min'"):
            ops.segment_sync(X, [0, 4, 9], agg)
    with pytest.raises(ValueError, match="aggregate='sum' is not served"):
        ops.segment_sync(X, [0, 4, 9], "sum")
    for e in ([0, 4, 10], [4, 0], [[0, 4, 9]], [0.0, 4.0]):
        with pytest.raises(ValueError, match="edges"):
            ops.segment_sync(X, e)


def test_core_functions_refuse_without_a_device():
    import scipy.sparse

    from sygnals_amd.core import structure as S
    data, rec = np.ones((4, 9)), np.ones((6, 6))
    with pytest.raises(ValueError, match="rec must be square"):
        S.recurrence_to_lag(np.ones((6, 5)))
    with pytest.raises(ValueError, match="sparse matrices are not served"):
        S.recurrence_to_lag(scipy.sparse.csr_matrix(rec))
    with pytest.raises(ValueError, match="sparse matrices are not served"):
        S.path_enhance(scipy.sparse.eye(6), 3)
    with pytest.raises(ValueError, match="lag must be \\[t, t\\] or padded"):
        S.lag_to_recurrence(np.ones((7, 3)))
    with pytest.raises(ValueError, match="axis=2 must be -1"):
        S.timelag_filter(np.mean, axis=2)
    with pytest.raises(ValueError, match="arguments served are mode and cval"):
        S.path_enhance(rec, 3, origin=1)
    with pytest.raises(ValueError, match="mode='spline' is not served"):
        S.path_enhance(rec, 3, mode="spline")
    with pytest.raises(ValueError, match="min_ratio=3.0 cannot exceed"):
        S.path_enhance(rec, 3, min_ratio=3.0)
    for fn, args in ((S.agglomerative, (data, 2)), (S.subsegment, (data, [3]))):
        with pytest.raises(ValueError, match="clusterer= callables are not served"):
            fn(*args, clusterer=object())
    for k in (0, 10):
        with pytest.raises(ValueError, match="k"):
            S.agglomerative(data, k)
    with pytest.raises(ValueError, match="9000 frames are above the served 8192"):
        S.agglomerative(np.ones((2, 9000)), 3)
    with pytest.raises(ValueError, match="axis=5 is not an axis"):
        S.agglomerative(data, 2, axis=5)
    with pytest.raises(ValueError, match="n_segments=0"):
        S.subsegment(data, [3], 0)
    with pytest.raises(ValueError, match="aggregate='median' is not served"):
        S.sync(data, [3], aggregate=np.median)
    with pytest.raises(ValueError, match="is not served"):
        S.sync(data, [3], aggregate=np.sum)
    with pytest.raises(ValueError, match="idx leaves no segment"):
        S.sync(data, [3], pad=False)
    with pytest.raises(ValueError, match="y must be one real clip"):
        S.structure_segments(np.ones((2, 100)), 22050, 2)
    with pytest.raises(ValueError, match="feature='cqt' is not served"):
        S.structure_segments(np.ones(4096), 22050, 2, feature="cqt")
    with pytest.raises(ValueError, match="the clip has 9 frames"):
        S.structure_segments(np.ones(4096), 22050, 10)


def test_plugin_registers_the_structure_functions():
    from sygnals_amd.core import similarity as SM
    from sygnals_amd.core import structure as S
    from sygnals_amd.plugins import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.f = {}

        def add_feature(self, name, fn):
            self.f[name] = fn
    r = Reg()
    SygnalsAmdPlugin().register_feature_extractors(r)
    assert r.f["path_enhance"] is S.path_enhance and r.f["agglomerative"] is S.agglomerative and r.f["subsegment"] is S.subsegment
    assert r.f["recurrence_matrix"] is SM.recurrence_matrix
    assert {"recurrence_to_lag", "lag_to_recurrence", "timelag_filter", "path_enhance", "agglomerative", "subsegment", "sync"} <= set(S.__all__)
    assert all(n + "_batch" in S.__all__ for n in ("recurrence_to_lag", "lag_to_recurrence", "timelag_filter", "path_enhance",
                                                   "agglomerative", "subsegment", "sync"))
