"""The LPC entries of the C ABI are declared, bound and exported and reject bad arguments before device work; the
constants are what the Python side reports; what is not served is refused with a ValueError that says what is, without
a device; the plugin registers lpc; the CLI reports its usage errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_lpc_constants", "syg_lpc_frames_f32", "syg_lpc_rows_work_bytes", "syg_lpc_rows_f32", "syg_lpc_envelope_f32"]
KEYS = ("max_frame", "max_order", "waves", "tile_frames", "span_max", "stage_chunk", "acorr_chunk")


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
    from sygnals_amd import _lpc, ops
    k = ops.lpc_constants()
    assert k == {name: h.syg_lpc_constants(i) for i, name in enumerate(KEYS)}
    assert k["max_frame"] == _lpc.MAX_FRAME == 2048 and k["max_order"] == _lpc.MAX_ORDER == 64
    assert 1 <= k["waves"] <= 16 and 64 % k["tile_frames"] == 0 and k["tile_frames"] >= k["waves"]
    # the staged span and the tile's results fit 64 KiB of LDS, so two workgroups fit a CU
    assert 4 * (k["span_max"] + k["tile_frames"] * (2 * 64 + 3)) <= 64 * 1024
    assert (k["tile_frames"] - 1) * 512 + 2048 <= k["span_max"]                  # the 2048 / 512 shape is staged
    assert k["stage_chunk"] % 256 == 0 and 8 * k["stage_chunk"] <= 48 * 1024 and k["acorr_chunk"] % 256 == 0
    assert h.syg_lpc_constants(7) == -1 and b"unknown key" in h.syg_last_error()
    assert h.syg_lpc_constants(-1) == -1
    nb = -(-100000 // k["stage_chunk"])
    assert h.syg_lpc_rows_work_bytes(3, 100000, 16, 0) == 8 * (2 * 3 * 100000 + 2 * 3 * nb * 5 + 3 * 64)
    assert h.syg_lpc_rows_work_bytes(3, 100000, 16, 1) == 8 * 3 * -(-100000 // k["acorr_chunk"]) * 65
    for bad in ((0, 100, 4, 0), (1, 2, 1, 0), (1, (1 << 26) + 1, 4, 0), (1 << 20, 1 << 12, 4, 0), (1, 100, 0, 0), (1, 100, 65, 1), (1, 100, 4, 2)):
        assert h.syg_lpc_rows_work_bytes(*bad) == -1 and b"bad B / L / order / method" in h.syg_last_error()


def _frames(h, p, y=True, B=2, L=6000, ldy=6000, frame=2048, hop=512, center=1, T=12, win=True, order=16, method=0, a=True, k=True,
            err=True):
    s = lambda on: p if on else None                                 # noqa: E731
    return h.syg_lpc_frames_f32(s(y), B, L, ldy, frame, hop, center, T, s(win), order, method, s(a), s(k), s(err), None)


def test_frames_rejects(h, p):
    for kw in ({"y": False}, {"a": False}):
        assert _frames(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for frame in (2049, 4096, 2, 0, -5):
        assert _frames(h, p, frame=frame) != 0 and b"is not served by the frame kernel" in h.syg_last_error()
    for method in (-1, 2):
        assert _frames(h, p, method=method) == -1 and b"neither SYG_LPC_BURG" in h.syg_last_error()
    for order in (0, -1, 65):
        assert _frames(h, p, order=order) == -1 and b"is outside 1 ... min(64, N - 2) = 64" in h.syg_last_error()
    assert _frames(h, p, frame=40, order=39, T=151) == -1 and b"min(64, N - 2) = 38 for N = 40" in h.syg_last_error()
    for kw in ({"B": 0}, {"L": 0, "T": 1}, {"ldy": 5999}):
        assert _frames(h, p, **kw) == -1 and b"bad B / L / ldy" in h.syg_last_error()
    for kw in ({"hop": 0}, {"center": 2}):
        assert _frames(h, p, **kw) == -1 and b"bad hop / center" in h.syg_last_error()
    for T in (11, 13, 0):
        assert _frames(h, p, T=T) == -1 and b"framing rule" in h.syg_last_error()
    assert _frames(h, p, center=0, T=12) == -1 and b"framing rule (8)" in h.syg_last_error()
    # another frame length than a power of two follows the padded rule: 1 + (6000 + 2 * 200 - 400) / 160 = 38
    assert _frames(h, p, frame=400, hop=160, T=39) == -1 and b"framing rule (38)" in h.syg_last_error()
    assert _frames(h, p, B=1 << 21, order=64, hop=1, T=6001) == -1 and b"above 2^31" in h.syg_last_error()


def test_rows_and_envelope_reject(h, p):
    rows = lambda y=p, B=2, L=5000, ldy=5000, win=None, order=16, method=0, work=p, wb=1 << 30, a=p: \
        h.syg_lpc_rows_f32(y, B, L, ldy, win, order, method, work, wb, a, None, None, None)      # noqa: E731
    assert rows(y=None) == -1 and b"null pointer" in h.syg_last_error() and rows(a=None) == -1
    assert rows(method=3) == -1 and b"neither SYG_LPC_BURG" in h.syg_last_error()
    for kw in ({"B": 0}, {"L": 2}, {"L": (1 << 26) + 1, "ldy": 1 << 27}, {"ldy": 4999}):
        assert rows(**kw) == -1 and b"bad B / L / ldy" in h.syg_last_error()
    for order in (0, 65):
        assert rows(order=order) == -1 and b"is outside 1 ... min(64, N - 2)" in h.syg_last_error()
    need = h.syg_lpc_rows_work_bytes(2, 5000, 16, 0)
    for kw in ({"work": None}, {"wb": need - 1}):
        assert rows(**kw) == -1 and f"workspace of {need} bytes needed".encode() in h.syg_last_error()
    env = lambda a=p, err=p, B=2, order=16, T=5, n_fft=512, ph=p, db=0, amin=1e-10, out=p: \
        h.syg_lpc_envelope_f32(a, err, B, order, T, n_fft, ph, db, amin, out, None)               # noqa: E731
    for kw in ({"a": None}, {"err": None}, {"ph": None}, {"out": None}):
        assert env(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for order in (0, 65):
        assert env(order=order) == -1 and b"is outside 1 ... 64" in h.syg_last_error()
    for n_fft in (0, 1, 513, (1 << 24) + 2):
        assert env(n_fft=n_fft) == -1 and b"must be even and in [2, 2^24]" in h.syg_last_error()
    assert env(db=2) == -1 and b"db must be 0 or 1" in h.syg_last_error()
    for amin in (-1.0, float("nan"), float("inf")):
        assert env(amin=amin) == -1 and b"amin must be finite" in h.syg_last_error()
    for kw in ({"B": 0}, {"T": 0}, {"B": 1 << 20, "T": 1 << 20}):
        assert env(**kw) == -1 and b"bad B / T" in h.syg_last_error()


def test_signatures():
    from sygnals_amd import ops
    from sygnals_amd.core.features import cepstral as CF
    assert list(inspect.signature(CF.lpc).parameters) == ["y", "order", "method", "window"]
    sig = inspect.signature(CF.lpc_batch)
    assert list(sig.parameters) == ["y", "order", "frame_length", "hop_length", "center", "method", "window", "return_reflection",
                                    "return_error"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [2048, 512, True, "burg", None, False, False]
    assert list(inspect.signature(ops.lpc_frames).parameters)[:7] == ["y", "order", "frame_length", "hop", "center", "method", "window"]
    assert "form" in inspect.signature(ops.lpc_rows).parameters and "db" in inspect.signature(ops.lpc_envelope).parameters
    assert CF.CEPSTRAL_FEATURES["lpc"] is CF.lpc and "mfcc" in CF.CEPSTRAL_FEATURES


def test_refusals_need_no_device():
    from sygnals_amd import ops
    from sygnals_amd.core.features import cepstral as CF
    y = torch.zeros((2, 6000), dtype=torch.float32)                 # a host tensor: anything that got further would fail on it
    x = np.zeros(6000)
    # the order: outside [1, min(64, N - 2)], with the bound named
    for order in (0, -2, 65, 1.5, True):
        for call in (lambda: ops.lpc_frames(y, order), lambda: ops.lpc_rows(y, order), lambda: CF.lpc(x, order),
                     lambda: CF.lpc_batch(y, order), lambda: CF.lpc_batch(np.zeros((2, 6000)), order)):
            with pytest.raises(ValueError) as e:
                call()
            assert "order" in str(e.value) and ("min(64, N - 2) = 64" in str(e.value) or "integer" in str(e.value))
    with pytest.raises(ValueError, match=r"order=39 is outside 1 ... min\(64, N - 2\) = 38 for N = 40"):
        ops.lpc_frames(y, 39, 40, 10)
    with pytest.raises(ValueError, match=r"min\(64, N - 2\) = 6 for N = 8"):
        CF.lpc(np.zeros(8), 7)
    with pytest.raises(ValueError, match=r"min\(64, N - 2\) = 1 for N = 3"):
        ops.lpc_rows(y[:, :3], 2)
    # frames above 2048 in the frame form, with what serves longer rows
    for call in (lambda: ops.lpc_frames(y, 16, 2049), lambda: ops.lpc_frames(y, 16, 4096, 1024), lambda: CF.lpc_batch(y, 16, 4096)):
        with pytest.raises(ValueError) as e:
            call()
        assert "is above 2048" in str(e.value) and "lpc_rows" in str(e.value)
    with pytest.raises(ValueError, match="the frame form serves rows of at most 2048 samples"):
        ops.lpc_rows(y, 16, form="frame")
    with pytest.raises(ValueError, match="form must be None, 'frame' or 'stage'"):
        ops.lpc_rows(y, 16, form="fused")
    for kw in ({"frame_length": 2}, {"hop": 0}, {"hop": 1.5}, {"frame_length": 400.5}):
        with pytest.raises(ValueError):
            ops.lpc_frames(y, 1, **kw)
    # another method name
    for call in (lambda: ops.lpc_frames(y, 16, method="covariance"), lambda: ops.lpc_rows(y, 16, method="yule"),
                 lambda: CF.lpc(x, 16, method="cov"), lambda: CF.lpc_batch(y, 16, method=None)):
        with pytest.raises(ValueError) as e:
            call()
        assert "'burg'" in str(e.value) and "'autocorr'" in str(e.value)
    # empty and malformed inputs
    for bad in (torch.zeros((0, 800)), torch.zeros((2, 0)), torch.zeros(800), torch.zeros((2, 800), dtype=torch.float64), x):
        for call in (lambda: ops.lpc_frames(bad, 4, 400, 160), lambda: ops.lpc_rows(bad, 4)):
            with pytest.raises(ValueError):
                call()
    for bad in (np.zeros(0), np.zeros((2, 800))):
        with pytest.raises(ValueError):
            CF.lpc(bad, 4)
    for bad in (np.zeros((0, 800)), np.zeros((2, 0)), np.zeros(800)):
        with pytest.raises(ValueError):
            CF.lpc_batch(bad, 4, 400, 160)
    with pytest.raises(ValueError, match="too short"):
        ops.lpc_frames(y[:, :100], 4, 400, 160, center=False)
    # results above 2^31 elements are refused by name and size.  (Expanded views: no memory.)
    big = torch.zeros((1, 1), dtype=torch.float32).expand(40000, 65536)
    with pytest.raises(ValueError) as e:
        ops.lpc_frames(big, 64, 2048, 64)
    assert "lpc_frames" in str(e.value) and str(40000 * 65 * 1025) in str(e.value) and "2^31" in str(e.value)
    with pytest.raises(ValueError) as e:
        ops.lpc_rows(big, 16)
    assert "lpc_rows" in str(e.value) and str(40000 * 65536) in str(e.value) and "2^31" in str(e.value)
    with pytest.raises(ValueError, match="2\\^26"):
        ops.lpc_rows(torch.zeros((1, 1), dtype=torch.float32).expand(1, (1 << 26) + 1), 16)
    # the envelope
    a, err = torch.zeros((2, 17, 5), dtype=torch.float32), torch.zeros((2, 5), dtype=torch.float32)
    for n_fft in (0, 1, 513, 2048.5):
        with pytest.raises(ValueError, match="n_fft"):
            ops.lpc_envelope(a, err, n_fft)
    with pytest.raises(ValueError, match="amin must be finite"):
        ops.lpc_envelope(a, err, amin=-1.0)
    for bad_a, bad_e in ((a[:, :1], err), (torch.zeros((2, 66, 5)), err), (a, err[:, :4]), (a[0], err), (a.double(), err)):
        with pytest.raises(ValueError):
            ops.lpc_envelope(bad_a, bad_e)
    with pytest.raises(ValueError) as e:
        ops.lpc_envelope(torch.zeros((1, 1, 1), dtype=torch.float32).expand(4000, 17, 1000), torch.zeros((1, 1)).expand(4000, 1000), 4096)
    assert "lpc_envelope" in str(e.value) and "2^31" in str(e.value)


def test_plugin_registers_lpc():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    got = {}

    class Reg:
        def add_transform(self, name, fn):
            got[name] = fn
    SygnalsAmdPlugin().register_transforms(Reg())
    from sygnals_amd.core.features import cepstral as CF
    assert got["lpc"] is CF.lpc and "real_cepstrum" in got


def test_cli_usage_errors(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    pd.DataFrame({"value": np.arange(8.0)}).to_csv(tmp_path / "x.csv", index=False)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", "lpc", str(tmp_path / "x.csv"), "-o", str(tmp_path / "y.npz"), *a])   # noqa: E731
    r = run("--order", "7")
    assert r.exit_code == 2 and "min(64, N - 2) = 6 for N = 8" in r.output
    r = run("--order", "0")
    assert r.exit_code == 2 and "order=0 is outside 1 ..." in r.output
    r = run("--order", "65", "--frames")
    assert r.exit_code == 2 and "min(64, N - 2) = 64 for N = 2048" in r.output
    r = run("--order", "16", "--frames", "--frame-length", "17")
    assert r.exit_code == 2 and "min(64, N - 2) = 15 for N = 17" in r.output
    r = run("--order", "4", "--frames", "--frame-length", "4096")
    assert r.exit_code == 2 and "is above 2048" in r.output
    r = run("--order", "4", "--frames", "--hop", "0")
    assert r.exit_code == 2 and "hop_length must be at least 1" in r.output
    r = run("--order", "4", "--envelope", "--n-fft", "513")
    assert r.exit_code == 2 and "n_fft=513 must be even" in r.output
    r = run("--order", "4", "--method", "covariance")
    assert r.exit_code == 2
    r = run()
    assert r.exit_code == 2 and "--order" in r.output
    r = CliRunner().invoke(cli, ["dsp", "--help"])
    assert r.exit_code == 0 and "lpc" in r.output
