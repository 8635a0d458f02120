"""The resampling entries of the C ABI are declared, bound and exported and reject bad arguments before device work; the
mirrors keep their signatures; what is not served is refused without a device; the CLI reports its usage errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from sygnals_amd import _resample as RS
from tests.test_cabi_symbols import declared_functions

NEW = ["syg_resample_tile", "syg_resample_table_lds_rule", "syg_resample_table_lds_max", "syg_resample_table_max", "syg_resample_span_max",
       "syg_resample_rate_max", "syg_resample_poly_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 64)()                       # never dereferenced: every call is rejected
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)
    assert h.syg_abi_version() == 1


def test_constants(h):
    from sygnals_amd import ops
    k = ops.resample_constants()
    assert k == dict(tile=h.syg_resample_tile(), table_lds_rule=h.syg_resample_table_lds_rule(),
                     table_lds_max=h.syg_resample_table_lds_max(), table_max=h.syg_resample_table_max(),
                     span_max=h.syg_resample_span_max(), rate_max=h.syg_resample_rate_max())
    assert k["tile"] % 256 == 0 and 256 <= k["tile"] <= 4096
    # the staged span (one pad word per 32 at most), the table and a tile of results fit the 160 KiB of LDS together
    assert 4 * (k["span_max"] * 33 // 32 + 1) + k["table_lds_max"] + 4 * k["tile"] <= 160 * 1024
    assert 0 < k["table_lds_rule"] <= k["table_lds_max"] < k["table_max"] <= 64 << 20
    assert k["rate_max"] + k["tile"] * k["rate_max"] <= 1 << 31          # p0 + i down in 32 bits
    # the tables of the audio rates, as the default filter makes them, may all be forced into LDS; the rule keeps the
    # small ones there
    for up, down in ((160, 441), (320, 441), (147, 160), (160, 147), (441, 160), (1, 3), (3, 1)):
        pl = RS.resample_plan(up, down, 32768)
        assert ops.resample_table_fits_lds(pl.up, pl.Kp) and pl.table.nbytes <= k["table_max"]
        assert ops.resample_table_in_lds(pl.up, pl.Kp) == (pl.table.nbytes <= k["table_lds_rule"]) == (max(up, down) <= 3)
    assert not ops.resample_table_fits_lds(441, 200)


def _rs(h, p, x=True, B=2, L=100, ldx=100, up=3, down=2, npr=10, Kp=21, table=True, pad=0, cval=0.0, form=-1, n_out=150, y=True,
        ldy=150):
    a = lambda on: p if on else None                                 # noqa: E731
    return h.syg_resample_poly_f32(a(x), B, L, ldx, up, down, npr, Kp, a(table), pad, cval, form, n_out, a(y), ldy, None)


def test_rejects(h, p):
    for kw in ({"x": False}, {"table": False}, {"y": False}):
        assert _rs(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"up": 0}, {"down": 0}, {"up": -3}, {"down": -1}, {"up": (1 << 20) + 1}, {"down": 1 << 21}):
        assert _rs(h, p, **kw) == -1 and b"must be in [1, 1048576]" in h.syg_last_error()
    for kw in ({"B": 0}, {"B": -1}, {"B": 65536}, {"L": 0, "n_out": 0}, {"L": -4}, {"L": 1 << 40, "ldx": 1 << 40}):
        assert _rs(h, p, **kw) == -1 and b"bad B / L" in h.syg_last_error()
    for n_out in (149, 151, 0):
        assert _rs(h, p, n_out=n_out) == -1 and b"is not ceil(L up / down) = 150" in h.syg_last_error()
    assert _rs(h, p, L=5, ldx=5, up=2, down=3, n_out=3) == -1 and b"= 4" in h.syg_last_error()      # ceil, not floor
    assert _rs(h, p, ldx=99) == -1 and b"ldx=99 is less than L=100" in h.syg_last_error()
    assert _rs(h, p, ldy=149) == -1 and b"ldy=149 is less than n_out=150" in h.syg_last_error()
    for pad in (-1, 5, 99):
        assert _rs(h, p, pad=pad) == -1 and b"unknown pad code" in h.syg_last_error()
    assert _rs(h, p, L=1, ldx=1, n_out=2, pad=4) == -1 and b"reflect pad rule needs at least two samples" in h.syg_last_error()
    for kw in ({"Kp": 0}, {"Kp": -2}, {"npr": -1}):
        assert _rs(h, p, **kw) == -1 and b"bad Kp / n_pre_remove" in h.syg_last_error()
    big = h.syg_resample_table_max() // 4 // 3 + 1                   # up Kp 4 just over the bound
    assert _rs(h, p, Kp=big) == -1
    msg = h.syg_last_error()
    assert b"up=3, down=2" in msg and b"above the bound of %d" % h.syg_resample_table_max() in msg
    for form in (-2, 2):
        assert _rs(h, p, form=form) == -1 and b"form must be" in h.syg_last_error()
    over = h.syg_resample_table_lds_max() // 4 // 3 + 1              # too large for LDS, fine for global memory
    assert _rs(h, p, Kp=over | 1, form=0) == -1 and b"form 0 needs a table of at most" in h.syg_last_error()


def test_mirror_signatures():
    import sygnals_amd.core.dsp as D
    from sygnals_amd import ops
    from sygnals_amd.core.audio import io as AIO
    from sygnals_amd.pipeline import mfcc_from_files
    W = ("kaiser", 5.0)
    sig = inspect.signature(D.resample)
    assert list(sig.parameters) == ["data", "orig_sr", "target_sr", "window", "padtype", "cval"]
    assert (sig.parameters["window"].default, sig.parameters["padtype"].default, sig.parameters["cval"].default) == (W, "constant", None)
    assert list(inspect.signature(D.resample_batch).parameters) == ["y", "orig_sr", "target_sr", "window", "padtype", "cval"]
    assert list(inspect.signature(D.resample_poly_batch).parameters) == ["y", "up", "down", "window", "padtype", "cval"]
    sig = inspect.signature(ops.resample_poly)
    assert list(sig.parameters) == ["y", "up", "down", "window", "padtype", "cval", "form", "out"]
    assert [sig.parameters[k].default for k in ("window", "padtype", "cval", "form", "out")] == [W, "constant", None, None, None]
    assert list(inspect.signature(ops.resample_plan).parameters) == ["up", "down", "L", "window"]
    sig = inspect.signature(AIO.load_audio)
    assert list(sig.parameters) == ["file_path", "sr", "mono", "offset", "duration", "res_type"]
    assert [sig.parameters[k].default for k in ("sr", "mono", "offset", "duration", "res_type")] == [None, True, 0.0, None, "poly"]
    assert inspect.signature(mfcc_from_files).parameters["target_sr"].default is None


def test_load_audio_messages_and_res_type(tmp_path):
    from scipy.io import wavfile
    from sygnals_amd.core.audio.io import load_audio
    with pytest.raises(FileNotFoundError) as e:
        load_audio(tmp_path / "nope.wav")
    assert str(e.value) == f"Audio input file not found: {tmp_path / 'nope.wav'}"
    with pytest.raises(ValueError) as e:
        load_audio(tmp_path)
    assert str(e.value) == f"Input path is not a file: {tmp_path}"
    pcm = (np.arange(2000).reshape(1000, 2) % 200 - 100).astype(np.int16) * 100
    wavfile.write(tmp_path / "a.wav", 8000, pcm)
    for res_type in ("kaiser_best", "kaiser_fast", "soxr_hq"):
        with pytest.raises(ValueError) as e:
            load_audio(tmp_path / "a.wav", sr=16000, res_type=res_type)
        assert "resampy" in str(e.value) and "kaiser_best" in str(e.value)
    # the native rate needs no device: decode, mix down, cut
    y, sr = load_audio(tmp_path / "a.wav")
    assert sr == 8000 and y.dtype == np.float64 and np.array_equal(y, (pcm / 32768.0).mean(axis=1))
    y, sr = load_audio(str(tmp_path / "a.wav"), sr=8000, mono=False, offset=0.05, duration=0.025)
    assert sr == 8000 and y.shape == (2, 200) and np.array_equal(y, pcm.T[:, 400:600] / 32768.0)


def test_refusals_need_no_device():
    import sygnals_amd.core.dsp as D
    from sygnals_amd import ops
    y = torch.zeros((2, 40), dtype=torch.float32)                   # a host tensor: anything that got further would fail on it
    for pad in RS.REFUSED_PADS + ("nonsense",):
        for call in (lambda: ops.resample_poly(y, 3, 2, padtype=pad), lambda: D.resample_poly_batch(y, 3, 2, padtype=pad),
                     lambda: D.resample(np.zeros(40), 8000, 16000, padtype=pad)):
            with pytest.raises(ValueError) as e:
                call()
            assert "not served" in str(e.value) and all(s in str(e.value) for s in RS.SERVED_PADS)
    with pytest.raises(ValueError) as e:
        ops.resample_poly(torch.zeros((3, 1), dtype=torch.float32), 3, 2, padtype="reflect")
    assert "at least two samples" in str(e.value)
    with pytest.raises(ValueError):
        D.resample(np.zeros(1), 8000, 16000, padtype="reflect")
    for a, b in ((44100.5, 16000), (44100, 16000.25), (0, 16000), (44100, -1), ("x", 16000), (float("nan"), 8000), (float("inf"), 8000)):
        for call in (lambda: D.resample(np.zeros(8), a, b), lambda: D.resample_batch(y, a, b)):
            with pytest.raises(ValueError) as e:
                call()
            assert "integer-valued" in str(e.value)
    for call in (lambda: ops.resample_poly(y, 1.5, 2), lambda: ops.resample_poly(y, 0, 2), lambda: ops.resample_plan(2, 0, 10)):
        with pytest.raises(ValueError):
            call()
    k = ops.resample_constants()
    down = k["table_max"] // 80 + 7                                  # 20 down + 1 taps of 4 bytes: just over the bound
    with pytest.raises(ValueError) as e:
        ops.resample_poly(y, 1, down)
    assert f"up=1, down={down}" in str(e.value) and str(k["table_max"]) in str(e.value)
    with pytest.raises(ValueError) as e:
        ops.resample_poly(y, 3, 2, window=np.ones(k["table_max"] // 4 + 8))
    assert "up=3, down=2" in str(e.value)
    with pytest.raises(ValueError):
        ops.resample_poly(y, 3, 2, form="registers")
    with pytest.raises(ValueError):
        ops.resample_poly(y, 3, 2, padtype="edge", cval=1.0)
    with pytest.raises(ValueError):
        D.resample(np.zeros((2, 2)), 8000, 16000)
    assert D.resample(np.zeros(0), 8000, 16000).shape == (0,)


def test_plugin_registers_the_transform():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    names = []

    class Reg:
        def add_transform(self, name, fn):
            names.append(name)
    SygnalsAmdPlugin().register_transforms(Reg())
    assert "resample" in names and "hilbert_transform" in names


def test_cli_usage_errors(tmp_path):
    import click
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli, parse_window_spec
    assert parse_window_spec("kaiser:5.0") == ("kaiser", 5.0) and parse_window_spec("hann") == "hann"
    assert parse_window_spec(" kaiser : 8 ") == ("kaiser", 8.0)
    for bad in ("kaiser:abc", "", ":5"):
        with pytest.raises(click.UsageError):
            parse_window_spec(bad)
    pd.DataFrame({"value": np.arange(8.0)}).to_csv(tmp_path / "x.csv", index=False)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", "resample", str(tmp_path / "x.csv"), "-o", str(tmp_path / "y.csv"), *a])   # noqa: E731
    r = run("--target-sr", "16000")
    assert r.exit_code == 2 and "--fs is required" in r.output
    for v in ("0", "-8000"):
        r = run("--target-sr", v, "--fs", "8000")
        assert r.exit_code == 2 and "--target-sr must be a positive" in r.output
    r = run("--fs", "8000")
    assert r.exit_code == 2 and "--target-sr" in r.output
    r = run("--target-sr", "16000", "--fs", "0")
    assert r.exit_code == 2 and "--fs must be a positive" in r.output
    r = run("--target-sr", "16000", "--fs", "8000", "--padtype", "median")
    assert r.exit_code == 2 and "not served" in r.output
    r = run("--target-sr", "16000", "--fs", "8000", "--window", "kaiser:x")
    assert r.exit_code == 2 and "--window" in r.output
    r = CliRunner().invoke(cli, ["dsp", "--help"])
    assert r.exit_code == 0 and "resample" in r.output
