"""The cepstral entries of the C ABI are declared, bound and exported and reject bad arguments before device work; the
constants are what the Python side reports; what is not served is refused without a device; the plugin registers the
whole-row functions; the CLI reports its usage errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_cepstrum_constants", "syg_cepstrogram2048_f32", "syg_cepstrum_logmag_c64", "syg_cepstrum_gather_f32",
       "syg_cepstrum_unwrap_work_bytes", "syg_cepstrum_unwrap_c64", "syg_cepstrum_exp_c64", "syg_cepstrum_peaks_f32"]


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
    k = ops.cepstrum_constants()
    assert k == {name: h.syg_cepstrum_constants(i) for i, name in
                 enumerate(("frame", "tile_frames", "waves", "scan", "lds_fixed", "lds_max"))}
    assert k["frame"] == 2048 and k["scan"] % 256 == 0 and 1 <= k["waves"] <= 16
    assert 64 % k["tile_frames"] == 0 and k["tile_frames"] >= k["waves"]      # a wave stores whole runs of frames
    assert k["lds_max"] <= 160 * 1024                                            # every n_ceps fits the LDS of a CU
    # the stage of n_ceps quefrencies: tile_frames rows of 64 ceil(Q / 64) + 64 / tile_frames floats
    assert k["lds_max"] == k["lds_fixed"] + 4 * k["tile_frames"] * (2048 + 64 // k["tile_frames"])
    assert 2 * (k["lds_fixed"] + 4 * k["tile_frames"] * (1088 + 64 // k["tile_frames"])) <= 160 * 1024   # two workgroups at Q = 1025
    assert h.syg_cepstrum_constants(6) == -1 and b"unknown key" in h.syg_last_error()
    assert h.syg_cepstrum_constants(-1) == -1
    assert h.syg_cepstrum_unwrap_work_bytes(3, 1024) == 4 * 3 * (1024 + 1)
    assert h.syg_cepstrum_unwrap_work_bytes(1, 1025) == 4 * (1025 + 2)
    for bad in ((0, 16), (1, 1), (1, (1 << 26) + 1), (1 << 20, 1 << 12)):
        assert h.syg_cepstrum_unwrap_work_bytes(*bad) == -1 and b"bad B / n" in h.syg_last_error()


def _fused(h, p, y=True, B=2, L=6000, ldy=6000, frame=2048, hop=512, center=1, T=12, win=True, tw=True, n_ceps=1025, amin=1e-5, out=True):
    a = lambda on: p if on else None                                 # noqa: E731
    return h.syg_cepstrogram2048_f32(a(y), B, L, ldy, frame, hop, center, T, a(win), a(tw), n_ceps, amin, a(out), None)


def test_fused_rejects(h, p):
    for kw in ({"y": False}, {"win": False}, {"tw": False}, {"out": False}):
        assert _fused(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    for n_ceps in (0, -3, 2049):
        assert _fused(h, p, n_ceps=n_ceps) == -1 and b"is outside 1 ... n_fft = 2048" in h.syg_last_error()
    for frame in (1024, 4096, 2047, 0):
        assert _fused(h, p, frame=frame) != 0 and b"is not served by the fused kernel" in h.syg_last_error()
    for amin in (-1e-5, float("nan"), float("inf"), -float("inf")):
        assert _fused(h, p, amin=amin) == -1 and b"amin must be finite and >= 0" in h.syg_last_error()
    for kw in ({"B": 0}, {"L": 0, "T": 1}, {"ldy": 5999}):
        assert _fused(h, p, **kw) == -1 and b"bad B / L / ldy" in h.syg_last_error()
    for kw in ({"hop": 0}, {"center": 2}):
        assert _fused(h, p, **kw) == -1 and b"bad hop / center" in h.syg_last_error()
    for T in (11, 13, 0):
        assert _fused(h, p, T=T) == -1 and b"framing rule" in h.syg_last_error()
    assert _fused(h, p, center=0, T=12) == -1 and b"framing rule (8)" in h.syg_last_error()
    assert _fused(h, p, B=1 << 20, n_ceps=2048, hop=1, T=6001) == -1 and b"above 2^31" in h.syg_last_error()


def test_pointwise_rejects(h, p):
    q = C.cast((C.c_double * 8)(), C.c_void_p)
    lm = lambda X=p, rows=2, bins=16, n=16, amin=1e-5, Z=q: h.syg_cepstrum_logmag_c64(X, rows, bins, n, amin, Z, None)   # noqa: E731
    assert lm(X=None) == -1 and b"null pointer" in h.syg_last_error() and lm(Z=None) == -1
    for kw in ({"rows": 0}, {"n": 0, "bins": 0}, {"n": (1 << 26) + 1}, {"rows": 1 << 28}):
        assert lm(**kw) == -1 and b"bad rows / n" in h.syg_last_error()
    for bins in (8, 10, 17):
        assert lm(bins=bins) == -1 and b"neither n = 16 nor n / 2 + 1" in h.syg_last_error()
    for amin in (-1.0, float("nan"), float("inf")):
        assert lm(amin=amin) == -1 and b"amin must be finite" in h.syg_last_error()
    assert lm(bins=9, Z=p) == -1 and b"in place" in h.syg_last_error()
    ga = lambda Z=p, rows=6, n=16, Q=9, T=3, amin=1e-5, out=q: h.syg_cepstrum_gather_f32(Z, rows, n, Q, T, amin, out, None)   # noqa: E731
    assert ga(Z=None) == -1 and b"null pointer" in h.syg_last_error() and ga(out=None) == -1
    for Q in (0, 17, -1):
        assert ga(Q=Q) == -1 and b"is outside 1 ... n_fft = 16" in h.syg_last_error()
    for T in (0, 4):
        assert ga(T=T) == -1 and b"neither a multiple of T" in h.syg_last_error()
    assert ga(amin=-2.0) == -1 and b"amin must be finite" in h.syg_last_error()
    uw = lambda X=p, B=2, n=16, amin=1e-5, work=p, wb=4 * 2 * 17, Z=q, nd=q: \
        h.syg_cepstrum_unwrap_c64(X, B, n, amin, work, wb, Z, nd, None)                        # noqa: E731
    for kw in ({"X": None}, {"Z": None}, {"nd": None}):
        assert uw(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"n": 1}, {"n": 0}):
        assert uw(**kw) == -1 and b"bad rows / n" in h.syg_last_error()
    assert uw(amin=float("nan")) == -1 and b"amin must be finite" in h.syg_last_error()
    for kw in ({"work": None}, {"wb": 4 * 2 * 17 - 1}):
        assert uw(**kw) == -1 and b"workspace of 136 bytes needed" in h.syg_last_error()
    ex = lambda Xh=p, B=2, n=16, nd=p, Z=q: h.syg_cepstrum_exp_c64(Xh, B, n, nd, Z, None)     # noqa: E731
    for kw in ({"Xh": None}, {"nd": None}, {"Z": None}):
        assert ex(**kw) == -1 and b"null pointer" in h.syg_last_error()
    assert ex(n=1) == -1 and b"bad rows / n" in h.syg_last_error()
    pk = lambda c=p, B=2, Q=100, T=5, qmin=10, qmax=90, sr=22050.0, thr=0.13, f0=q, s=q, qs=q, v=q: \
        h.syg_cepstrum_peaks_f32(c, B, Q, T, qmin, qmax, sr, thr, f0, s, qs, v, None)            # noqa: E731
    for kw in ({"c": None}, {"f0": None}, {"s": None}, {"qs": None}, {"v": None}):
        assert pk(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"Q": 0}, {"T": 0}, {"B": 1 << 20, "T": 1 << 20}):
        assert pk(**kw) == -1 and b"bad B / Q / T" in h.syg_last_error()
    for kw in ({"qmin": 0}, {"qmin": 91}, {"qmax": 100}):
        assert pk(**kw) == -1 and b"need 1 <= qmin <= qmax < Q" in h.syg_last_error()
    for kw in ({"sr": 0.0}, {"sr": float("inf")}, {"thr": float("nan")}):
        assert pk(**kw) == -1 and b"bad sr / threshold" in h.syg_last_error()


def test_signatures():
    from sygnals_amd import ops
    import sygnals_amd.core.dsp as D
    import sygnals_amd.core.audio.features as AF
    sig = inspect.signature(ops.cepstrogram)
    assert list(sig.parameters) == ["y", "n_fft", "hop", "center", "window", "win_length", "n_ceps", "amin", "form", "out"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [2048, 512, True, "hann", None, None, 1e-5, None, None]
    for fn in (ops.real_cepstrum, ops.complex_cepstrum, D.real_cepstrum, D.complex_cepstrum, D.real_cepstrum_batch,
               D.complex_cepstrum_batch):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == ["n", "amin"] and sig.parameters["n"].default is None and sig.parameters["amin"].default == 1e-5
    for fn in (ops.inverse_complex_cepstrum, D.inverse_complex_cepstrum, D.inverse_complex_cepstrum_batch):
        assert list(inspect.signature(fn).parameters)[1:] == ["ndelay"]
    assert list(inspect.signature(ops.cepstrum_peaks).parameters) == ["ceps", "qmin", "qmax", "sr", "threshold"]
    assert inspect.signature(ops.cepstrum_peaks).parameters["threshold"].default == 0.13
    assert list(inspect.signature(D.cepstrogram_batch).parameters) == ["y", "n_fft", "hop_length", "center", "window", "win_length",
                                                                      "n_ceps", "amin"]
    assert "threshold" in inspect.signature(AF.fundamental_frequency_batch).parameters


def test_refusals_need_no_device():
    from sygnals_amd import ops
    import sygnals_amd.core.dsp as D
    import sygnals_amd.core.audio.features as AF
    y = torch.zeros((2, 6000), dtype=torch.float32)                 # a host tensor: anything that got further would fail on it
    x = np.zeros(64)
    for kw in ({"n_ceps": 0}, {"n_ceps": 2049}, {"n_ceps": 1.5}, {"n_ceps": 129, "n_fft": 128}):
        with pytest.raises(ValueError) as e:
            ops.cepstrogram(y, **kw)
        assert "is outside 1 ... n_fft" in str(e.value)
    for amin in (-1e-5, float("nan"), float("inf")):
        for call in (lambda: ops.cepstrogram(y, amin=amin), lambda: ops.real_cepstrum(y, amin=amin),
                     lambda: ops.complex_cepstrum(y, amin=amin), lambda: D.real_cepstrum(x, amin=amin),
                     lambda: D.complex_cepstrum(x, amin=amin)):
            with pytest.raises(ValueError) as e:
                call()
            assert "amin must be finite and >= 0" in str(e.value)
    for kw in ({"form": "lds"}, {"form": "fused", "n_fft": 1024}, {"hop": 0}, {"hop": 1.5}, {"n_fft": 1}, {"n_fft": 2048.5}):
        with pytest.raises(ValueError):
            ops.cepstrogram(y, **kw)
    with pytest.raises(ValueError) as e:
        ops.cepstrogram(y, n_fft=1024, form="fused")
    assert "2048 only" in str(e.value)
    with pytest.raises(ValueError) as e:
        ops.cepstrogram(y[:, :100], center=False)
    assert "too short" in str(e.value)
    for bad in (x, torch.zeros(8), torch.zeros((2, 8), dtype=torch.float64), torch.zeros((0, 8)), torch.zeros((2, 0))):
        for call in (lambda: ops.cepstrogram(bad), lambda: ops.real_cepstrum(bad), lambda: ops.complex_cepstrum(bad)):
            with pytest.raises(ValueError):
                call()
    # results above 2^31 elements are refused by name and size.  (Expanded views: no memory.)
    big = torch.zeros((1, 1), dtype=torch.float32).expand(40000, 65536)
    with pytest.raises(ValueError) as e:
        ops.cepstrogram(big, hop=64)
    assert "cepstrogram" in str(e.value) and str(40000 * 1025 * 1025) in str(e.value) and "2^31" in str(e.value)
    for fn, name in ((ops.real_cepstrum, "real_cepstrum"), (ops.complex_cepstrum, "complex_cepstrum")):
        with pytest.raises(ValueError) as e:
            fn(big)
        assert name in str(e.value) and str(40000 * 65536) in str(e.value) and "2^31" in str(e.value)
    for n in (0, -4, 2.5, (1 << 26) + 1):
        for call in (lambda: ops.real_cepstrum(y, n), lambda: D.real_cepstrum(x, n), lambda: D.complex_cepstrum(x, n)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        ops.complex_cepstrum(y, 1)                                  # no bin beside bin 0
    for data in (np.zeros(0), np.zeros((2, 8))):
        for fn in (D.real_cepstrum, D.complex_cepstrum):
            with pytest.raises(ValueError):
                fn(data)
    with pytest.raises(ValueError):
        D.inverse_complex_cepstrum(x, 1.5)
    c = torch.zeros((2, 100, 5), dtype=torch.float32)
    for kw in ({"qmin": 0, "qmax": 50}, {"qmin": 60, "qmax": 50}, {"qmin": 10, "qmax": 100}, {"qmin": 1.5, "qmax": 50}):
        with pytest.raises(ValueError) as e:
            ops.cepstrum_peaks(c, sr=22050.0, **kw)
        assert "qmin <= qmax < Q" in str(e.value)
    with pytest.raises(ValueError):
        ops.cepstrum_peaks(c, 10, 50, 0.0)
    # the pitch method: fmin / fmax that leave no quefrency range are refused with all three named
    for fmin, fmax, sr in ((500.0, 400.0, 22050), (5.0, 8.0, 22050)):
        for call in (lambda: AF.fundamental_frequency(np.zeros(4096), sr, fmin, fmax, method="cepstrum"),
                     lambda: AF.fundamental_frequency_batch(y, sr, fmin, fmax, method="cepstrum"),
                     lambda: ops.pitch_cepstrum(y, sr, fmin, fmax)):
            with pytest.raises(ValueError) as e:
                call()
            assert all(s in str(e.value) for s in (f"fmin={fmin}", f"fmax={fmax}", f"sr={float(sr)}"))
    with pytest.raises(ValueError, match="Unsupported pitch estimation method"):
        AF.fundamental_frequency(np.zeros(4096), 22050, method="swipe")
    with pytest.raises(ValueError, match="Unsupported pitch estimation method"):
        AF.fundamental_frequency_batch(y, 22050, method="swipe")
    with pytest.raises(TypeError):
        AF.fundamental_frequency_batch(y, 22050, method="yin", threshold=0.2)


def test_plugin_registers_the_transforms():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    names = []

    class Reg:
        def add_transform(self, name, fn):
            names.append(name)
    SygnalsAmdPlugin().register_transforms(Reg())
    assert {"real_cepstrum", "complex_cepstrum", "inverse_complex_cepstrum"} <= set(names) and "compute_fft" in names


def test_cli_usage_errors(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    pd.DataFrame({"value": np.arange(8.0)}).to_csv(tmp_path / "x.csv", index=False)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", "cepstrum", str(tmp_path / "x.csv"), "-o", str(tmp_path / "y.npz"), *a])   # noqa: E731
    r = run("--frames", "--kind", "complex")
    assert r.exit_code == 2 and "cannot be combined with --kind complex" in r.output
    r = run("--frames", "--n", "16")
    assert r.exit_code == 2 and "--n-fft" in r.output
    r = run("--n", "0")
    assert r.exit_code == 2 and "--n must be at least 1" in r.output
    r = run("--kind", "complex", "--n", "1")
    assert r.exit_code == 2 and "--n must be at least 2" in r.output
    r = run("--frames", "--hop", "0")
    assert r.exit_code == 2 and "--hop at least 1" in r.output
    r = run("--frames", "--n-fft", "8", "--n-ceps", "9")
    assert r.exit_code == 2 and "is outside 1 ... n_fft = 8" in r.output
    r = run("--kind", "cubic")
    assert r.exit_code == 2
    r = CliRunner().invoke(cli, ["dsp", "--help"])
    assert r.exit_code == 0 and "cepstrum" in r.output
