"""Host side of the free-running form of syg_stft2048_mfcc_tri_f32: the predicate that says where it can load its frames
and the option that selects it.  Both answer before any device call."""
import ctypes as C
import os

import pytest

from tests.test_cabi_symbols import declared_functions

OPT = 6      # SYG_OPT_STFT_FREERUN


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_symbol_declared_bound_exported(h):
    from sygnals_amd import _lib, ops
    raw = C.CDLL(_lib.LIB_PATH)
    name = "syg_stft2048_mfcc_tri_freerun"
    assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert ops._LIB_OPTIONS["stft_freerun"] == OPT


@pytest.mark.parametrize("hop,L,ldy,addr,want", [
    (512, 48000, 48000, 0x1000, 1),              # the headline shape
    (160, 5000, 5000, 0x1008, 1),                # 8-byte aligned is enough
    (2, 2, 2, 0x1000, 1),
    (1024, 48000, 48000, 0x1000, 1),             # no stage buffer: the hop is not bounded by it
    (511, 6144, 6144, 0x1000, 0),                # odd hop
    (128, 4001, 4002, 0x1000, 0),                # odd L
    (128, 4000, 4001, 0x1000, 0),                # odd row stride
    (128, 4000, 4000, 0x1004, 0),                # clips start between two pairs
    (128, 4000, 4000, 0x1002, 0),
    (512, (1 << 28) - 2, 1 << 28, 0x1000, 1),    # byte offsets inside a clip in 32 bits, as for the staged tiles
    (512, 1 << 28, 1 << 28, 0x1000, 0),
    (512, 1 << 30, 1 << 30, 0x1000, 0),
])
def test_freerun_predicate(h, hop, L, ldy, addr, want):
    assert h.syg_stft2048_mfcc_tri_freerun(hop, L, ldy, C.c_void_p(addr)) == want


def test_freerun_option(h):
    from sygnals_amd import ops
    assert h.syg_get_option(OPT) == -1 and ops.get_option("stft_freerun") == -1
    try:
        for v in (0, 1, -1):
            assert h.syg_set_option(OPT, v) == 0 and h.syg_get_option(OPT) == v
        for bad in (2, -2):
            assert h.syg_set_option(OPT, bad) == -1 and b"stft_freerun must be -1 (default), 0 or 1" in h.syg_last_error()
            assert h.syg_get_option(OPT) == -1
        with ops.override(stft_freerun=1):
            assert ops.get_option("stft_freerun") == 1
            assert ops.get_option("stft_load") == -1          # its own option: the load path keeps its meaning and range
        assert ops.get_option("stft_freerun") == -1
    finally:
        assert h.syg_set_option(OPT, -1) == 0
