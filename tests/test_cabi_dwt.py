"""The wavelet entries of the C ABI are declared, bound and exported, and reject bad arguments before device work."""
import ctypes as C
import os

import pytest

from tests import dwt_ref as R
from tests.test_cabi_symbols import declared_functions

NEW = ["syg_dwt_lengths", "syg_dwt_fits", "syg_dwt_work_bytes", "syg_dwt_f32", "syg_idwt_length", "syg_idwt_work_bytes",
       "syg_idwt_f32"]
ZERO, CONSTANT, SYMMETRIC, REFLECT, PERIODIC = range(5)
LDS_FLOATS = 160 * 1024 // 4


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


def _lens(*v):
    arr = (C.c_int64 * len(v))(*v)
    return C.cast(arr, C.c_void_p), arr


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "sygnals_hip.h")).read()
    for i, name in enumerate(("ZERO", "CONSTANT", "SYMMETRIC", "REFLECT", "PERIODIC")):
        assert f"#define SYG_DWT_{name} {i}\n" in src
    assert h.syg_abi_version() == 1


def test_lengths_against_the_restatement(h):
    import numpy as np
    triples = [(1, 2, 1), (1, 20, 3), (2, 2, 1), (7, 4, 2), (8, 2, 3), (17, 20, 4), (255, 8, 5), (256, 8, 5), (257, 16, 7),
               (1000, 8, 3), (4097, 4, 12), (32768, 8, 12), (200001, 20, 14), (1 << 24, 8, 21)]
    for L, F, levels in triples:
        name = "db%d" % (F // 2)
        arr = (C.c_int64 * (levels + 1))()
        total = h.syg_dwt_lengths(L, F, levels, C.cast(arr, C.c_void_p))
        if L <= 5000:
            want = [c.size for c in R.wavedec(np.zeros(L), name, level=levels)]
        else:
            n, ls = L, []
            for _ in range(levels):
                n = R.dwt_coeff_len(n, F)
                ls.append(n)
            want = [ls[-1]] + ls[::-1]
        assert list(arr) == want and total == sum(want), (L, F, levels)
        assert h.syg_idwt_length(C.cast(arr, C.c_void_p), levels, F) in (L, L + 1)
    arr = (C.c_int64 * 8)()
    q = C.cast(arr, C.c_void_p)
    assert h.syg_dwt_lengths(100, 8, 3, None) == -1 and b"null pointer" in h.syg_last_error()
    for L, F, levels in ((0, 8, 3), (100, 8, 0), (-4, 8, 1), (100, 8, 65)):
        assert h.syg_dwt_lengths(L, F, levels, q) == -1 and b"bad L / levels" in h.syg_last_error()
    for F in (0, 1, 3, 7, 22, -2):
        assert h.syg_dwt_lengths(100, F, 3, q) == -1 and b"F must be even and in 2 ... 20" in h.syg_last_error()


def test_fit_rule_and_workspace(h):
    # the first two approximations (the first rounded up to even) fit 160 KiB of LDS
    def fits(L, F):
        n1 = (L + F - 1) // 2
        n2 = (n1 + F - 1) // 2
        return n1 + (n1 & 1) + n2 <= LDS_FLOATS
    for F in (2, 8, 20):
        lim = max(L for L in range(54000, 54700) if fits(L, F))
        assert not fits(lim + 1, F)
        assert h.syg_dwt_fits(lim, F, 5) == 1 and h.syg_dwt_fits(lim + 1, F, 5) == 0
        assert h.syg_dwt_work_bytes(3, lim, F, 5) == 0
        n1 = (lim + 1 + F - 1) // 2
        n2 = (n1 + F - 1) // 2
        assert h.syg_dwt_work_bytes(3, lim + 1, F, 5) == 3 * (n1 + (n1 & 1) + n2) * 4
        assert h.syg_dwt_work_bytes(3, lim + 1, F, 1) == 0                 # one level: cA goes straight to the row
    assert h.syg_dwt_fits(32768, 8, 12) == 1 and h.syg_dwt_fits(48000, 8, 12) == 1 and h.syg_dwt_fits(1 << 24, 8, 21) == 0
    assert h.syg_dwt_fits(0, 8, 1) == 0 and h.syg_dwt_fits(100, 7, 1) == 0 and h.syg_dwt_fits(100, 8, 0) == 0
    for B, L, F, levels in ((0, 100, 8, 1), (1, 0, 8, 1), (1, 100, 9, 1), (1, 100, 8, 0), (1, 100, 22, 1)):
        assert h.syg_dwt_work_bytes(B, L, F, levels) == -1
    # the switch to one launch per level
    assert h.syg_set_option(4, 0) == 0
    try:
        assert h.syg_dwt_fits(1000, 8, 3) == 0 and h.syg_dwt_work_bytes(2, 1000, 8, 3) == 2 * (504 + 255) * 4
        assert h.syg_dwt_work_bytes(1, 3, 20, 5) == (20 + 19) * 4       # shorter than the filter: lengths rise to F - 1
        q, _k = _lens(131, 131, 255, 503)
        assert h.syg_idwt_work_bytes(2, q, 3, 8) == 2 * (256 + 504) * 4
    finally:
        assert h.syg_set_option(4, 1) == 0
    assert h.syg_set_option(4, 2) == -1 and b"dwt_form must be 0 or 1" in h.syg_last_error()
    q, _k = _lens(131, 131, 255, 503)
    assert h.syg_idwt_work_bytes(2, q, 3, 8) == 0


def _dwt(h, p, x=True, B=2, L=1000, ldx=1000, lo=True, hi=True, F=8, mode=SYMMETRIC, levels=3, out=True, ldout=1020,
         work=None):
    return h.syg_dwt_f32(p if x else None, B, L, ldx, p if lo else None, p if hi else None, F, mode, levels,
                         p if out else None, ldout, work, None)


def test_dwt_rejects(h, p):
    for kw in (dict(x=False), dict(lo=False), dict(hi=False), dict(out=False)):
        assert _dwt(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in (dict(B=0), dict(L=0), dict(B=-1), dict(L=-7)):
        assert _dwt(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for levels in (0, -1, 65):
        assert _dwt(h, p, levels=levels) == -1 and b"levels must be 1 ... 64" in h.syg_last_error()
    for F in (0, 1, 3, 7, 21, 22, -8):
        assert _dwt(h, p, F=F) == -1 and b"F must be even and in 2 ... 20" in h.syg_last_error()
    for mode in (-1, 5, 99):
        assert _dwt(h, p, mode=mode) == -1 and b"unknown mode" in h.syg_last_error()
    assert _dwt(h, p, ldx=999) == -1 and b"ldx = 999 is smaller than the row" in h.syg_last_error()
    assert _dwt(h, p, ldout=1019) == -1 and b"ldout = 1019 is smaller than the packed row (1020)" in h.syg_last_error()
    L = 200000
    total = h.syg_dwt_lengths(L, 8, 3, _lens(0, 0, 0, 0)[0])
    assert h.syg_dwt_work_bytes(1, L, 8, 3) > 0
    assert _dwt(h, p, B=1, L=L, ldx=L, ldout=total) == -1 and b"need a workspace" in h.syg_last_error()


def _idwt(h, p, lens=(131, 131, 255, 503), coeffs=True, B=2, ldc=1020, levels=3, lo=True, hi=True, F=8, y=True, ldy=1000,
          work=None, lens_null=False):
    q, _keep = _lens(*lens)
    return h.syg_idwt_f32(p if coeffs else None, B, ldc, None if lens_null else q, levels, p if lo else None,
                          p if hi else None, F, p if y else None, ldy, work, None)


def test_idwt_rejects(h, p):
    for kw in (dict(coeffs=False), dict(lo=False), dict(hi=False), dict(y=False), dict(lens_null=True)):
        assert _idwt(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for B in (0, -3):
        assert _idwt(h, p, B=B) == -1 and b"bad B" in h.syg_last_error()
    for levels in (0, -1, 65):
        assert _idwt(h, p, levels=levels) == -1 and b"levels must be 1 ... 64" in h.syg_last_error()
    for F in (0, 3, 22):
        assert _idwt(h, p, F=F) == -1 and b"F must be even and in 2 ... 20" in h.syg_last_error()
    assert _idwt(h, p, ldc=1019) == -1 and b"ldc = 1019 is smaller than the packed row (1020)" in h.syg_last_error()
    assert _idwt(h, p, ldy=999) == -1 and b"ldy = 999 is smaller than the row (1000)" in h.syg_last_error()
    for lens in ((131, 130, 255, 503), (133, 131, 255, 503), (131, 131, 254, 503), (131, 131, 255, 505), (0, 131, 255, 503),
                 (3, 3, 255, 503)):
        assert _idwt(h, p, lens=lens) == -1 and b"inconsistent lens" in h.syg_last_error(), lens
        q, _k = _lens(*lens)
        assert h.syg_idwt_length(q, 3, 8) == -1 and h.syg_idwt_work_bytes(2, q, 3, 8) == -1
    # an approximation one longer than its detail is trimmed, not refused
    q, _k = _lens(132, 131, 255, 503)
    assert h.syg_idwt_length(q, 3, 8) == 1000
    q, _k = _lens(131, 131, 255, 503)
    assert h.syg_idwt_length(q, 3, 8) == 1000 and h.syg_idwt_length(None, 3, 8) == -1
    # a long row's fine levels run through the workspace
    lens = (25006, 25006, 50005, 100003)
    q, _k = _lens(*lens)
    assert h.syg_idwt_work_bytes(1, q, 3, 8) == (100004 + 50006) * 4
    assert _idwt(h, p, lens=lens, B=1, ldc=sum(lens), ldy=200000) == -1 and b"need a workspace" in h.syg_last_error()


def test_public_functions_importable():
    from sygnals_amd.core.transforms import (discrete_wavelet_transform, dwt_batch, idwt_batch,  # noqa: F401
                                             inverse_discrete_wavelet_transform)
    from sygnals_amd.ops import dwt, dwt_fits, idwt  # noqa: F401
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin

    class Reg:
        def __init__(self):
            self.names = []

        def add_transform(self, name, fn):
            self.names.append(name)
    r = Reg()
    SygnalsAmdPlugin().register_transforms(r)
    assert {"discrete_wavelet_transform", "inverse_discrete_wavelet_transform", "hilbert_transform"} <= set(r.names)
