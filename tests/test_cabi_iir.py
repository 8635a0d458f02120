"""The causal SOS entries of the C ABI are declared, bound and exported and reject bad arguments before device work; the
work-size formula; the Python side refuses without a device; the plugin registers the new filters; the CLI's options,
usage errors and --band parsing, and `filter apply` without the new options calls exactly what it called before."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_sosfilt_constants", "syg_sosfilt_work_bytes", "syg_sosfilt_f32"]
IDENT = [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]


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


def test_constants_and_work_bytes(h):
    from sygnals_amd import ops
    k = ops.sosfilt_constants()
    assert k == {name: h.syg_sosfilt_constants(i) for i, name in enumerate(ops.SOSFILT_KEYS)}
    assert k["tile"] * 8 == k["chunk"] and k["chunks_per_wave"] == 64 and k["group_sections"] == 8 and k["max_sections"] == 32
    assert k["chunk"] % 4 == 0 and k["scan_ahead"] >= 1 and k["two_level_chunks"] >= 2 * k["scan_ahead"]
    assert h.syg_sosfilt_constants(7) == -1 and b"unknown key" in h.syg_last_error() and h.syg_sosfilt_constants(-1) == -1
    for B, L, S in ((1, 1, 1), (3, 256, 4), (3, 257, 4), (1024, 32768, 10), (7, 100000, 32), (1, 1 << 24, 8), (70000, 300, 2)):
        n = -(-L // k["chunk"])
        want = 2 * min(B, 65535) * (n + -(-n // k["scan_ahead"])) * 2 * min(S, 8) * 8
        assert h.syg_sosfilt_work_bytes(B, L, S) == want
    for bad in ((0, 100, 4), (1, 0, 4), (1, 100, 0), (1, 100, 33), (-1, 100, 4), (1, -5, 4)):
        assert h.syg_sosfilt_work_bytes(*bad) == -1
    # the zero-phase entry is as it was: at most 8 sections
    assert h.syg_sosfiltfilt_work_bytes(1, 100, 9, 9) == -1 and h.syg_sosfiltfilt_work_bytes(1, 100, 9, 8) >= 0


def test_rejects_before_device_work(h, p):
    sos = (C.c_double * (6 * 33))(*(IDENT * 33))
    sp = C.cast(sos, C.c_void_p)
    call = lambda x=p, B=2, L=1000, ldx=1000, s=sp, S=4, zi=None, y=p, ldy=1000, zf=None, work=p: \
        h.syg_sosfilt_f32(x, B, L, ldx, s, S, zi, y, ldy, zf, work, None)                        # noqa: E731
    for kw in ({"x": None}, {"y": None}, {"s": None}):
        assert call(**kw) == -1 and b"null pointer" in h.syg_last_error()
    assert call(S=0) == -1 and b"n_sections must be in [1, 32] (got 0)" in h.syg_last_error()
    assert call(S=33) == -1 and b"n_sections must be in [1, 32] (got 33)" in h.syg_last_error()
    assert call(S=-2) == -1 and b"n_sections must be in [1, 32]" in h.syg_last_error()
    assert call(L=0, ldx=0, ldy=0) == -1 and b"L must be at least 1 (got 0)" in h.syg_last_error()
    for kw in ({"B": 0}, {"ldx": 999}, {"ldy": 999}):
        assert call(**kw) == -1 and b"bad B / ldx / ldy" in h.syg_last_error()
    bad = (C.c_double * 18)(*(IDENT * 3))
    bad[6 * 2 + 3] = 0.0
    assert call(s=C.cast(bad, C.c_void_p), S=3) == -1 and b"a0 of section 2 is zero" in h.syg_last_error()
    assert call(work=None) == -1 and b"need the work buffer of syg_sosfilt_work_bytes" in h.syg_last_error()


def test_python_refusals_need_no_device():
    from sygnals_amd import ops
    from sygnals_amd.core import filters as F
    x = torch.zeros((2, 100), dtype=torch.float32)          # a host tensor: anything that got further would fail on it
    sos = np.array([IDENT] * 2)
    with pytest.raises(ValueError, match=r"shape \(n_sections, 6\)"):
        ops.sosfilt(x, np.zeros((2, 5)))
    for n in (0, 33):
        with pytest.raises(ValueError, match=f"{n} sections; the causal kernels serve 1 to 32"):
            ops.sosfilt(x, np.array([IDENT] * n).reshape(n, 6))
    z = sos.copy()
    z[1, 3] = 0.0
    with pytest.raises(ValueError, match="a0 of a section is zero"):
        ops.sosfilt(x, z)
    for bad in (torch.zeros(100), torch.zeros((2, 100), dtype=torch.float64), torch.zeros((0, 100)), torch.zeros((2, 0)),
                np.zeros((2, 100), dtype=np.float32)):
        with pytest.raises(ValueError, match="sosfilt: x must"):
            ops.sosfilt(bad, sos)
    for zi in (torch.zeros((2, 2, 2)), torch.zeros((2, 3, 2), dtype=torch.float64), torch.zeros((1, 2, 2), dtype=torch.float64),
               np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"zi must be a float64 tensor of shape \[B, n_sections, 2\] = \[2, 2, 2\]"):
            ops.sosfilt(x, sos, zi=zi)
    for out in (torch.zeros((2, 99)), torch.zeros((2, 100), dtype=torch.float64), torch.zeros((2, 200))[:, ::2]):
        with pytest.raises(ValueError, match="out must be a float32 tensor"):
            ops.sosfilt(x, sos, out=out)
    assert list(inspect.signature(ops.sosfilt).parameters) == ["x", "sos", "zi", "return_state", "out"]
    assert list(inspect.signature(F.design_iir_sos).parameters) == ["cutoff", "fs", "order", "filter_type", "family", "rp", "rs", "norm"]
    assert list(inspect.signature(F.apply_sos_filter_causal_batch).parameters) == ["sos", "data", "zi", "return_state"]
    assert list(inspect.signature(F.design_fir).parameters) == ["numtaps", "cutoff", "fs", "window", "pass_zero"]
    with pytest.raises(ValueError, match="must be a 1D array"):
        F.apply_sos_filter_causal(sos, np.zeros((2, 8)))
    with pytest.raises(ValueError, match=r"shape \(n_sections, 6\)"):
        F.apply_sos_filter_causal(np.zeros(6), np.zeros(8))
    with pytest.raises(ValueError, match="taps must be a non-empty 1D array"):
        F.apply_fir_filter_batch(np.zeros((2, 3)), x)


def test_plugin_registers_filters_and_effects_export():
    from sygnals_amd.core import filters as F
    from sygnals_amd.core.audio import effects as FX
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    got = {}

    class Reg:
        def add_filter(self, name, fn):
            got[name] = fn
    SygnalsAmdPlugin().register_filters(Reg())
    for name in ("design_iir_sos", "sosfilt_zi", "apply_sos_filter_causal", "apply_sos_filter_causal_batch", "design_fir",
                 "apply_fir_filter_batch"):
        assert got[name] is getattr(F, name)
    assert got["apply_sos_filter"] is F.apply_sos_filter and got["band_pass_filter"] is F.band_pass_filter
    for name in ("apply_parametric_eq", "apply_parametric_eq_batch", "apply_graphic_eq", "apply_graphic_eq_batch", "design_eq_sos"):
        assert name in FX.__all__ and callable(getattr(FX, name))
    assert list(inspect.signature(FX.apply_parametric_eq).parameters) == ["y", "sr", "params"]
    sig = inspect.signature(FX.apply_graphic_eq)
    assert list(sig.parameters) == ["y", "sr", "band_gains", "q_factor"] and sig.parameters["q_factor"].default == 1.414


def test_band_parsing():
    import click
    from sygnals_amd.cli.main import parse_eq_band
    assert parse_eq_band("peak:1000:-6:1.4") == {"type": "peak", "freq": 1000.0, "gain_db": -6.0, "q": 1.4}
    assert parse_eq_band("low_shelf:120:3") == {"type": "low_shelf", "freq": 120.0, "gain_db": 3.0}
    assert parse_eq_band(" Notch : 50 ") == {"type": "notch", "freq": 50.0}
    for bad in ("peak", "bell:1000:3", "peak:abc", "peak:1000:3:1:9", "", "peak:1000:nan", ":1000", "peak:1000:x"):
        with pytest.raises(click.UsageError, match="--band"):
            parse_eq_band(bad)


@pytest.fixture()
def wav(tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(0)
    wavfile.write(tmp_path / "x.wav", 8000, (0.1 * rng.standard_normal(400)).astype(np.float32))
    return tmp_path


def test_cli_help_and_usage_errors(wav):
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    r = CliRunner()
    out = r.invoke(cli, ["filter", "--help"]).output
    assert all(c in out for c in ("apply", "eq", "fir"))
    out = r.invoke(cli, ["filter", "apply", "--help"]).output
    for opt in ("--type", "--cutoff", "--fs", "--order", "-o, --output", "--family", "--rp", "--rs", "--causal",
                "[butter|cheby1|cheby2|ellip|bessel]", "[default: butter]"):
        assert opt in out
    out = r.invoke(cli, ["filter", "eq", "--help"]).output
    assert "--band" in out and "TYPE:FREQ[:GAIN_DB[:Q]]" in out
    out = r.invoke(cli, ["filter", "fir", "--help"]).output
    for opt in ("--numtaps", "--cutoff", "--window", "--pass-zero / --no-pass-zero"):
        assert opt in out
    x, y = str(wav / "x.wav"), str(wav / "y.wav")
    apply = lambda *a: r.invoke(cli, ["filter", "apply", x, "-o", y, *a])                         # noqa: E731
    res = apply("--type", "lowpass", "--cutoff", "1000", "--family", "cheby1")
    assert res.exit_code == 2 and "Family 'cheby1' needs rp > 0 dB" in res.output
    res = apply("--type", "lowpass", "--cutoff", "1000", "--family", "ellip", "--rp", "1")
    assert res.exit_code == 2 and "needs rs > 0 dB" in res.output
    res = apply("--type", "lowpass", "--cutoff", "1000", "--family", "chebyshev")
    assert res.exit_code == 2
    res = apply("--type", "lowpass", "--cutoff", "4000", "--family", "ellip", "--rp", "1", "--rs", "40", "--causal")
    assert res.exit_code == 2 and "strictly between 0 and Nyquist" in res.output
    res = apply("--type", "bandpass", "--cutoff", "300,3400", "--order", "9")                  # 9 sections, zero-phase
    assert res.exit_code == 2 and "9 second-order sections" in res.output and "--causal" in res.output
    eq = lambda *a: r.invoke(cli, ["filter", "eq", x, "-o", y, *a])                               # noqa: E731
    assert eq().exit_code == 2
    res = eq("--band", "peak:1000:3", "--band", "bell:100:3")
    assert res.exit_code == 2 and "--band: cannot read 'bell:100:3'" in res.output
    for f in ("4000", "5000"):
        res = eq("--band", f"peak:{f}:3")
        assert res.exit_code == 2 and "must be between 0 and Nyquist (4000.0 Hz)" in res.output
    res = eq("--band", "peak:1000:3:0")
    assert res.exit_code == 2 and "Q factor must be positive" in res.output
    fir = lambda *a: r.invoke(cli, ["filter", "fir", x, "-o", y, *a])                             # noqa: E731
    assert fir("--cutoff", "1000").exit_code == 2 and fir("--numtaps", "31").exit_code == 2
    assert fir("--numtaps", "31", "--cutoff", "a,b").exit_code == 2
    assert fir("--numtaps", "31", "--cutoff", "1,2,3").exit_code == 2
    res = fir("--numtaps", "31", "--cutoff", "4000")
    assert res.exit_code == 2 and "Invalid cutoff frequency" in res.output
    res = fir("--numtaps", "32", "--cutoff", "1000", "--no-pass-zero")
    assert res.exit_code == 2 and "even number of coefficients" in res.output
    assert not os.path.exists(y)


def test_cli_apply_defaults_call_what_they_called(wav, monkeypatch):
    """Without the new options `filter apply` designs with design_butterworth_sos and filters with apply_sos_filter, as before;
    with them it goes to design_iir_sos / apply_sos_filter_causal."""
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    from sygnals_amd.core import filters as F
    calls = []
    sos = np.array([IDENT])
    monkeypatch.setattr(F, "design_butterworth_sos", lambda *a, **k: calls.append(("butter", a, k)) or sos)
    monkeypatch.setattr(F, "design_iir_sos", lambda *a, **k: calls.append(("iir", a, k)) or sos)
    monkeypatch.setattr(F, "apply_sos_filter", lambda s, x: calls.append(("zero-phase", s.shape, x.shape)) or np.asarray(x, dtype=np.float64))
    monkeypatch.setattr(F, "apply_sos_filter_causal", lambda s, x: calls.append(("causal", s.shape, x.shape)) or np.asarray(x, dtype=np.float64))
    x, y = str(wav / "x.wav"), str(wav / "y.wav")
    res = CliRunner().invoke(cli, ["filter", "apply", x, "-o", y, "--type", "bandpass", "--cutoff", "300,3400"])
    assert res.exit_code == 0 and "Filtered signal saved to 'y.wav'." in res.output
    assert calls == [("butter", ((300.0, 3400.0), 8000, 5, "bandpass"), {}), ("zero-phase", (1, 6), (400,))]
    calls.clear()
    res = CliRunner().invoke(cli, ["filter", "apply", x, "-o", y, "--type", "lowpass", "--cutoff", "1000", "--order", "4", "--family",
                                   "ellip", "--rp", "0.5", "--rs", "60", "--causal"])
    assert res.exit_code == 0
    assert calls == [("iir", (1000.0, 8000, 4, "lowpass"), {"family": "ellip", "rp": 0.5, "rs": 60.0}), ("causal", (1, 6), (400,))]
    calls.clear()
    res = CliRunner().invoke(cli, ["filter", "apply", x, "-o", y, "--type", "lowpass", "--cutoff", "1000", "--causal"])
    assert res.exit_code == 0 and [c[0] for c in calls] == ["butter", "causal"]
