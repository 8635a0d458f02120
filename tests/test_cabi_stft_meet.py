"""Host side of SYG_OPT_STFT_MEET: how the free-running form of syg_stft2048_mfcc_tri_f32 hands a clip over (0: counters in
LDS, no workgroup barrier inside the tile loop; 1: one barrier per clip; -1: the library decides).  Answers before any
device call."""
import os
import re

import pytest

OPT = 7      # SYG_OPT_STFT_MEET
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_key_is_declared_documented_and_named(h):
    from sygnals_amd import ops
    hdr = open(os.path.join(ROOT, "include", "sygnals_hip.h")).read()
    assert re.search(r"#define\s+SYG_OPT_STFT_MEET\s+7\b", hdr) and re.search(r"#define\s+SYG_OPT_COUNT\s+8\b", hdr)
    assert re.search(r"#define\s+SYG_ABI_VERSION\s+1\b", hdr) and h.syg_abi_version() == 1
    assert re.search(r"\*\s+SYG_OPT_STFT_MEET\s+-1 \(default", hdr), "the option is documented in the header's option list"
    assert ops._LIB_OPTIONS["stft_meet"] == OPT
    assert ops._LIB_OPTIONS["stft_freerun"] == 6


def test_default_range_and_error_text(h):
    from sygnals_amd import ops
    assert h.syg_get_option(OPT) == -1 and ops.get_option("stft_meet") == -1
    try:
        for v in (0, 1, -1):
            assert h.syg_set_option(OPT, v) == 0 and h.syg_get_option(OPT) == v
        for bad in (2, -2, 3):
            assert h.syg_set_option(OPT, bad) == -1 and b"stft_meet must be -1 (default), 0 or 1" in h.syg_last_error()
            assert h.syg_get_option(OPT) == -1
        assert h.syg_set_option(OPT + 1, 0) == -1 and b"unknown option 8" in h.syg_last_error()
    finally:
        assert h.syg_set_option(OPT, -1) == 0


def test_override_sets_and_restores(h):
    from sygnals_amd import ops
    with ops.override(stft_meet=0):
        assert ops.get_option("stft_meet") == 0
        assert ops.get_option("stft_freerun") == -1 and ops.get_option("stft_load") == -1      # options of their own
        with ops.override(stft_meet=1, stft_freerun=1):
            assert ops.get_option("stft_meet") == 1 and ops.get_option("stft_freerun") == 1
        assert ops.get_option("stft_meet") == 0 and ops.get_option("stft_freerun") == -1
    assert ops.get_option("stft_meet") == -1
