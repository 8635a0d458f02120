"""The augmentation entries of the C ABI are declared, bound and exported, and reject bad arguments before device work;
the vocoder's step table is numpy's own arange."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_phase_vocoder_chunk", "syg_phase_vocoder_work_bytes", "syg_phase_vocoder_f32", "syg_fx_add_noise_resident_max",
       "syg_fx_add_noise_work_bytes", "syg_fx_add_noise_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 64)()                       # 16-byte aligned or not, never dereferenced: every call is rejected
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)


def _pv(h, p, D=True, B=2, T=10, col=True, alpha=True, To=13, out=True, work=None, form=0):
    return h.syg_phase_vocoder_f32(p if D else None, B, T, p if col else None, p if alpha else None, To,
                                   p if out else None, work, form, None)


def test_vocoder_rejects(h, p):
    for kw in ({"D": False}, {"col": False}, {"alpha": False}, {"out": False}):
        assert _pv(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"T": 0}, {"To": 0}, {"To": -3}, {"B": 1 << 40}):
        assert _pv(h, p, **kw) == -1 and b"bad B / T / T_out" in h.syg_last_error()
    for form in (-2, 2):
        assert _pv(h, p, form=form) == -1 and b"form must be" in h.syg_last_error()
    assert _pv(h, p, form=1) == -1 and b"needs `work`" in h.syg_last_error()
    K = h.syg_phase_vocoder_chunk()
    assert _pv(h, p, B=1, To=4 * K, form=-1) == -1 and b"needs `work`" in h.syg_last_error()   # the rule: one long row


def test_vocoder_plan(h):
    K = h.syg_phase_vocoder_chunk()
    assert K >= 8
    wb = h.syg_phase_vocoder_work_bytes
    assert wb(1024, 81, -1) == 0                                        # a batch: one chain per (clip, bin) fills the device
    assert wb(1, 4 * K - 1, -1) == 0                                    # one step short of four chunks
    assert wb(1, 4 * K, -1) == 16 * 4 * 1025                            # four chunk-start phasors (two float64) per bin
    assert wb(3, 4 * K + 1, -1) == 16 * 3 * 5 * 1025
    assert wb(1, 4 * K, 0) == 0 and wb(1024, 5, 1) == 16 * 1024 * 1025  # the explicit forms
    assert wb(0, 10, -1) == -1 and wb(1, 0, -1) == -1 and wb(1, 10, 2) == -1


def _an(h, p, y=True, B=2, L=100, ldy=100, nz=True, ldn=100, snr=True, out=True, ldo=100, work=None):
    return h.syg_fx_add_noise_f32(p if y else None, B, L, ldy, p if nz else None, ldn, p if snr else None,
                                  p if out else None, ldo, work, None)


def test_add_noise_rejects_and_plan(h, p):
    for kw in ({"y": False}, {"nz": False}, {"snr": False}, {"out": False}):
        assert _an(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"L": 0}, {"L": -1}):
        assert _an(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for kw in ({"ldy": 99}, {"ldn": 99}, {"ldo": 99}):
        assert _an(h, p, **kw) == -1 and b"bad ldy / ldn / ldo" in h.syg_last_error()
    R = h.syg_fx_add_noise_resident_max()
    assert R >= 4096
    assert _an(h, p, L=R + 1, ldy=R + 1, ldn=R + 1, ldo=R + 1) == -1 and b"needs `work`" in h.syg_last_error()
    wb = h.syg_fx_add_noise_work_bytes
    assert wb(1024, R) == 0 and wb(1, 1) == 0                           # resident: one launch, no workspace
    assert wb(1024, R + 1) == 16 * 1024 * 2                             # two slices of a row that is just too long
    assert wb(1, 1 << 24) == 16 * 64                                    # one long row: the most slices
    assert wb(0, 10) == -1 and wb(1, 0) == -1


@pytest.mark.parametrize("T", [1, 2, 3, 65, 1000])
@pytest.mark.parametrize("rate", [0.25, 0.37, 0.5, 0.8, 1.0, 1.25, 2.0, 3.7, 1e-3 + 2000.0])
def test_step_table_is_numpys_arange(T, rate):
    from sygnals_amd import _tables
    col, alpha = _tables.vocoder_steps(T, rate)
    steps = np.arange(0, T, rate, dtype=np.float64)
    assert col.dtype == np.int32 and alpha.dtype == np.float64
    assert len(col) == len(steps) == int(np.ceil(T / rate))
    assert np.array_equal(col, [int(s) for s in steps]) and np.array_equal(alpha, np.mod(steps, 1.0))
    assert col.min() >= 0 and col.max() <= T - 1 and alpha.min() >= 0 and alpha.max() < 1


def test_step_table_rejects():
    from sygnals_amd import _tables
    for T, rate in ((0, 1.0), (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf")), (1 << 20, 1e-6)):
        with pytest.raises(ValueError):
            _tables.vocoder_steps(T, rate)


def test_mirrors_keep_the_reference_signatures_and_messages():
    import sygnals_amd.core.audio.effects as E
    import sygnals_amd.core.augment as A
    from sygnals_amd.ops import fx_add_noise, phase_vocoder, time_stretch  # noqa: F401
    assert list(inspect.signature(E.time_stretch).parameters) == ["y", "rate"]
    assert list(inspect.signature(A.time_stretch).parameters) == ["y", "rate"]
    sig = inspect.signature(A.add_noise)
    assert list(sig.parameters) == ["y", "snr_db", "noise_type", "seed"]
    assert sig.parameters["noise_type"].default == "gaussian" and sig.parameters["seed"].default is None
    assert list(inspect.signature(A.add_noise_batch).parameters) == ["y", "snr_db", "noise_type", "seed", "noise"]
    assert not hasattr(A, "pitch_shift") and not hasattr(E, "pitch_shift")
    y, y2 = np.zeros(100), np.zeros((2, 100))

    def raises(text, fn, *a, **k):
        with pytest.raises(ValueError) as e:
            fn(*a, **k)
        assert str(e.value) == text

    for fn in (E.time_stretch, A.time_stretch):
        raises("Input audio data must be a 1D array.", fn, y2, 1.5)
        for rate in (0.0, -2.0):
            raises("Time stretch rate must be positive.", fn, y, rate)
    raises("Input audio data must be a 1D array for noise addition.", A.add_noise, y2, 10.0)
    raises("Invalid noise_type: 'violet'. Choose 'gaussian', 'white', 'pink', or 'brown'.", A.add_noise, y, 10.0, "violet")


def test_cli_rate_must_be_positive(tmp_path):
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    np.savez(tmp_path / "x.npz", data=np.zeros(100), sr=np.array(8000))
    for rate in ("0", "-1.5"):
        r = CliRunner().invoke(cli, ["augment", "time-stretch", str(tmp_path / "x.npz"), "-o", str(tmp_path / "y.npz"),
                                     "--rate", rate])
        assert r.exit_code == 2 and "Stretch rate must be positive." in r.output
    r = CliRunner().invoke(cli, ["augment", "--help"])
    assert r.exit_code == 0 and "add-noise" in r.output and "time-stretch" in r.output and "pitch-shift" not in r.output
