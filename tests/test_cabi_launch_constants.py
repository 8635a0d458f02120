"""The launch caps of the C ABI (syg_launch_constants): declared, bound and exported; the grid's y limit is the one number the
host plans restate; the workgroups a CU of the persistent grids are pinned, so that a retune has to come here and with
that re-derive the cases of tests/launch_cap_cases.py.  No device."""
import ctypes as C
import os

import pytest

from tests.test_cabi_symbols import declared_functions

KEYS = ("max_grid_y", "lpc_frames_wgs_per_cu", "lpc_envelope_wgs_per_cu", "pitch_frames_wgs_per_cu", "noise_wgs_per_cu")


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_symbol_declared_bound_exported(h):
    from sygnals_amd import _lib
    name = "syg_launch_constants"
    assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), name)


def test_exactly_the_named_keys(h):
    from sygnals_amd import ops
    k = ops.launch_constants()
    assert tuple(k) == KEYS
    assert [h.syg_launch_constants(i) for i in range(len(KEYS))] == [k[name] for name in KEYS]


def test_one_grid_y_limit(h):
    from sygnals_amd import _fftplan, ops
    k = ops.launch_constants()
    assert k["max_grid_y"] == 65535 == ops.MAX_ROWS == _fftplan.MAX_ROWS
    assert ops.TREMOLO_MAX_ROWS == 8 * k["max_grid_y"]


def test_workgroups_a_cu_are_pinned(h):
    from sygnals_amd import ops
    k = ops.launch_constants()
    assert (k["lpc_frames_wgs_per_cu"], k["lpc_envelope_wgs_per_cu"], k["pitch_frames_wgs_per_cu"], k["noise_wgs_per_cu"]) == (8, 32, 16, 8)


def test_the_case_table_reads_them(h):
    from tests import launch_cap_cases as LC
    k = LC.constants()
    assert set(LC.LAUNCH_NAMES.values()) == set(KEYS)
    for name, key in LC.LAUNCH_NAMES.items():
        assert name not in vars(LC) and getattr(LC, name) == k["launch"][key]


@pytest.mark.parametrize("which", [-1, len(KEYS), 1 << 20])
def test_unknown_key_is_refused(h, which):
    assert h.syg_launch_constants(which) < 0
    assert b"launch_constants: unknown key" in h.syg_last_error()
