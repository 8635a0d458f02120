"""The noise-generation entries of the C ABI are declared, bound and exported, and reject bad arguments before device
work; the host-side stream ids are the library's; the CLI's new options are checked; the mirrors keep their parameters."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_rng_constants", "syg_rng_philox_u32", "syg_rng_normal_f32", "syg_rng_normal_pairs_c64", "syg_rng_power_gain_c64",
       "syg_rng_unpack_pairs_f32", "syg_fx_add_noise_gen_work_bytes", "syg_fx_add_noise_gen_f32"]
ROWS = 1 << 31


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 64)()                       # aligned, never dereferenced: every call is rejected
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert h.syg_abi_version() == 1


def test_constants_are_the_host_sides(h):
    from sygnals_amd import _rng
    k = h.syg_rng_constants
    assert k(0) == _rng.ROUNDS == 10 and k(1) == _rng.STREAM_NOISE == 0 and k(2) == _rng.STREAM_ROW == 1
    assert k(3) == _rng.ROW_LIMIT == ROWS and k(4) == 1 << 26
    assert k(5) == -1 and k(-1) == -1


def test_philox_rejects(h, p):
    f = h.syg_rng_philox_u32
    for args in ((None, p, 4, p), (p, None, 4, p), (p, p, 4, None)):
        assert f(*args, None) == -1 and b"null pointer" in h.syg_last_error()
    for n in (0, -1):
        assert f(p, p, n, p, None) == -1 and b"bad n" in h.syg_last_error()
    odd = C.c_void_p(p.value + 4)
    assert f(odd, p, 4, p, None) == -1 and b"aligned" in h.syg_last_error()


def _nf(h, p, out=True, B=2, L=100, ld=100, seed=1, first_row=0, offset=0):
    return h.syg_rng_normal_f32(p if out else None, B, L, ld, seed, first_row, offset, None)


def test_normal_rejects(h, p):
    assert _nf(h, p, out=False) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"B": -2}, {"L": 0}, {"L": -1}, {"L": 1 << 39}):
        assert _nf(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    assert _nf(h, p, ld=99) == -1 and b"bad row stride" in h.syg_last_error()
    for kw in ({"first_row": -1}, {"first_row": ROWS - 1}, {"first_row": ROWS}, {"B": ROWS + 1, "ld": 100}):
        assert _nf(h, p, **kw) == -1 and b"must lie in [0, 2^31)" in h.syg_last_error()
    for off in (-1, 1 << 62):
        assert _nf(h, p, offset=off) == -1 and b"offset must be in" in h.syg_last_error()


def test_coloured_steps_reject(h, p):
    pairs, gain, unpack = h.syg_rng_normal_pairs_c64, h.syg_rng_power_gain_c64, h.syg_rng_unpack_pairs_f32
    assert pairs(None, 1, 8, 1, 0, None) == -1 and b"null pointer" in h.syg_last_error()
    for P, M in ((0, 8), (1, 0), (1, (1 << 26) + 1)):
        assert pairs(p, P, M, 1, 0, None) == -1 and b"bad P / M" in h.syg_last_error()
    for first_row, P in ((1, 1), (-2, 1), (ROWS - 2, 2)):
        assert pairs(p, P, 8, 1, first_row, None) == -1 and b"first_row must be even" in h.syg_last_error()
    assert gain(None, 1, 8, 1.0, None) == -1 and b"null pointer" in h.syg_last_error()
    for rows, M in ((0, 8), (1, 1), (1, 12), (1, 1 << 27)):
        assert gain(p, rows, M, 1.0, None) == -1 and b"bad rows / M" in h.syg_last_error()
    for alpha in (-0.5, 2.5, float("nan")):
        assert gain(p, 1, 8, alpha, None) == -1 and b"exponent must be in [0, 2]" in h.syg_last_error()
    assert unpack(None, 8, 0, p, 1, 8, 8, None) == -1 and b"null pointer" in h.syg_last_error()
    assert unpack(p, 8, 0, None, 1, 8, 8, None) == -1 and b"null pointer" in h.syg_last_error()
    assert unpack(p, 8, 0, p, 0, 8, 8, None) == -1 and b"bad B / L" in h.syg_last_error()
    assert unpack(p, 8, 0, p, 1, 8, 7, None) == -1 and b"bad row stride" in h.syg_last_error()
    assert unpack(p, 8, ROWS, p, 1, 8, 8, None) == -1 and b"must lie in [0, 2^31)" in h.syg_last_error()
    assert unpack(p, 4, 0, p, 1, 8, 8, None) == -1 and b"bad M" in h.syg_last_error()


def _ang(h, p, y=True, B=2, L=100, ldy=100, seed=1, first_row=0, snr=True, out=True, ldo=100, work=None):
    return h.syg_fx_add_noise_gen_f32(p if y else None, B, L, ldy, seed, first_row, p if snr else None, p if out else None, ldo,
                                      work, None)


def test_add_noise_gen_rejects_and_plan(h, p):
    for kw in ({"y": False}, {"snr": False}, {"out": False}):
        assert _ang(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"L": 0}, {"L": -1}):
        assert _ang(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for kw in ({"ldy": 99}, {"ldo": 99}):
        assert _ang(h, p, **kw) == -1 and b"bad ldy / ldo" in h.syg_last_error()
    for kw in ({"first_row": -1}, {"first_row": ROWS - 1}):
        assert _ang(h, p, **kw) == -1 and b"must lie in [0, 2^31)" in h.syg_last_error()
    R = h.syg_fx_add_noise_resident_max()
    assert _ang(h, p, L=R + 1, ldy=R + 1, ldo=R + 1) == -1 and b"needs `work`" in h.syg_last_error()
    wb = h.syg_fx_add_noise_gen_work_bytes
    assert wb(1024, R) == 0 and wb(1, 1) == 0                           # resident: one launch, no workspace
    # slice sums and one scale factor a row, 16 bytes each
    assert wb(1024, R + 1) == 16 * 1024 * (2 + 1)                       # two slices of a row that is just too long
    assert wb(1, 1 << 24) == 16 * (2048 + 1)                            # one long row: slices that fill the device
    assert wb(3, 1 << 24) == 16 * 3 * (683 + 1)                         # ceil(2048 / 3) slices of whole segments
    assert wb(4096, 1 << 20) == 16 * 4096 * (1 + 1)                     # a batch that fills it already: one slice
    assert wb(0, 10) == -1 and wb(1, 0) == -1


def test_python_refusals_need_no_device():
    """What ops checks before it asks for a GPU: seeds, rows, offsets, exponents, the coloured offset."""
    from sygnals_amd import ops
    from sygnals_amd.core.augment import noise as N
    for fn, args in ((ops.randn, (1, 8, -1)), (ops.randn, (1, 8, 1 << 64)), (ops.randn, (0, 8, 1)), (ops.randn, (1, 0, 1)),
                     (ops.randn, (1, 8, 1, -1)), (ops.randn, (2, 8, 1, (1 << 31) - 1)), (ops.randn, (1, 8, 1, 0, -1)),
                     (ops.colored_noise, (1, 8, 1, 2.5)), (ops.colored_noise, (1, 8, 1, -0.1)),
                     (ops.colored_noise, (1, 8, 1, float("nan"))), (ops.colored_noise, (1, 8, 1, 1.0, -1))):
        with pytest.raises(ValueError):
            fn(*args)
    assert "offset" not in inspect.signature(ops.colored_noise).parameters      # M depends on L: no offset for coloured noise
    assert ops.colored_noise_fft_len(1) == 2 and ops.colored_noise_fft_len(2) == 2 and ops.colored_noise_fft_len(3) == 4
    assert ops.colored_noise_fft_len(1024) == 1024 and ops.colored_noise_fft_len(1025) == 2048
    with pytest.raises(ValueError, match="Invalid noise_type: 'violet'. Choose 'gaussian', 'white', 'pink', or 'brown'."):
        N.generate_noise_batch(1, 8, "violet", seed=1)
    with pytest.raises(ValueError, match="exponent must be in"):
        N.generate_noise_batch(1, 8, "pink", seed=1, exponent=3.0)
    with pytest.raises(ValueError, match="Invalid noise_type: 'violet'"):
        N.add_noise_device(np.zeros(8), 10.0, "violet")
    with pytest.raises(ValueError, match="1D array for noise addition"):
        N.add_noise_device(np.zeros((2, 8)), 10.0)
    assert N.add_noise_device(np.zeros(0), 10.0, "pink", seed=1).shape == (0,)


def test_signatures():
    import sygnals_amd.core.augment as A
    assert list(inspect.signature(A.add_noise).parameters) == ["y", "snr_db", "noise_type", "seed"]
    assert list(inspect.signature(A.add_noise_batch).parameters) == ["y", "snr_db", "noise_type", "seed", "noise"]
    sig = inspect.signature(A.generate_noise_batch)
    assert list(sig.parameters) == ["B", "L", "noise_type", "seed", "exponent", "first_row", "device"]
    assert sig.parameters["noise_type"].default == "gaussian" and sig.parameters["first_row"].default == 0
    assert list(inspect.signature(A.add_noise_device_batch).parameters)[:6] == ["y", "snr_db", "noise_type", "seed", "exponent",
                                                                                 "first_row"]
    assert list(inspect.signature(A.add_noise_device).parameters)[:4] == ["y", "snr_db", "noise_type", "seed"]
    for name in ("add_noise_device", "add_noise_device_batch", "generate_noise_batch"):
        assert name in A.__all__


def test_cli_usage_errors(tmp_path):
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    np.savez(tmp_path / "x.npz", data=np.zeros(100), sr=np.array(8000))
    base = ["augment", "add-noise", str(tmp_path / "x.npz"), "-o", str(tmp_path / "y.npz"), "--snr", "10"]
    r = CliRunner().invoke(cli, base + ["--generator", "host", "--exponent", "1"])
    assert r.exit_code == 2 and "--exponent needs --generator device" in r.output
    r = CliRunner().invoke(cli, base + ["--exponent", "1"])                       # the default generator is the host's
    assert r.exit_code == 2 and "--exponent needs --generator device" in r.output
    for bad in ("2.5", "-1"):
        r = CliRunner().invoke(cli, base + ["--generator", "device", "--exponent", bad])
        assert r.exit_code == 2 and "--exponent must be in [0, 2]" in r.output
    r = CliRunner().invoke(cli, base + ["--generator", "cloud"])
    assert r.exit_code == 2
    r = CliRunner().invoke(cli, ["augment", "add-noise", "--help"])
    assert r.exit_code == 0 and "--generator" in r.output and "--exponent" in r.output
    assert not (tmp_path / "y.npz").exists()
