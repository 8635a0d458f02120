"""The cross-spectrum and GCC entries of the C ABI are declared, bound and exported and reject bad arguments before device
work; the workspace rule by value; what is not served is refused without a device; the plugin registers the transforms;
the CLI reports its usage errors and writes the documented table and .npz shapes."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_csd_work_bytes", "syg_csd_f32", "syg_csd_rows_f32", "syg_gcc_weight_c64", "syg_gcc_crop_f32", "syg_peak_pick_f32"]


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


def test_workspace_rule(h):
    # runs of max(16, ceil(nseg / 2048)) segments per workgroup; float32 partials [B, wg, 4, F], then float64 slice sums
    # [B, slices, 4, F]: 16 slices from 64 workgroups, else one
    F = 129
    assert h.syg_csd_work_bytes(1, 1, 256) == 1 * 4 * F * 4 + 1 * 4 * F * 8
    assert h.syg_csd_work_bytes(1, 16, 256) == 1 * 4 * F * 4 + 1 * 4 * F * 8
    assert h.syg_csd_work_bytes(1, 17, 256) == 2 * 4 * F * 4 + 1 * 4 * F * 8
    assert h.syg_csd_work_bytes(1024, 255, 256) == 1024 * 16 * 4 * F * 4 + 1024 * 4 * F * 8
    assert h.syg_csd_work_bytes(3, 63 * 16 + 1, 256) == 3 * 64 * 4 * F * 4 + 3 * 16 * 4 * F * 8
    assert h.syg_csd_work_bytes(1, 2048 * 16, 8) == 2048 * 4 * 5 * 4 + 16 * 4 * 5 * 8
    assert h.syg_csd_work_bytes(1, 2048 * 16 + 1, 8) == 1928 * 4 * 5 * 4 + 16 * 4 * 5 * 8          # runs of 17: 1928 workgroups
    assert h.syg_csd_work_bytes(1, 8191, 4096) == 512 * 4 * 2049 * 4 + 16 * 4 * 2049 * 8
    for bad in ((0, 1, 256), (1, 0, 256), (1, 1, 1)):
        assert h.syg_csd_work_bytes(*bad) == -1


def _csd(h, p, x=True, y=True, B=2, By=2, L=1000, ldx=1000, ldy=1000, nperseg=256, step=128, nfft=256, win=True, tw=True,
         detrend=1, scale=1.0, outs=(True, True, True, True), work=True):
    a = lambda on: p if on else None                # noqa: E731
    return h.syg_csd_f32(a(x), a(y), B, By, L, ldx, ldy, nperseg, step, nfft, a(win), a(tw), detrend, scale,
                         *(a(o) for o in outs), a(work), None)


def test_csd_rejects(h, p):
    for kw in ({"x": False}, {"y": False}, {"win": False}, {"tw": False}, {"work": False}):
        assert _csd(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    assert _csd(h, p, outs=(False,) * 4) == -1 and b"no output asked for" in h.syg_last_error()
    for nfft in (4, 300, 16384, 0):
        assert _csd(h, p, nfft=nfft, nperseg=4, step=2) == -1 and b"power of two in [8, 8192]" in h.syg_last_error()
    for kw in ({"nperseg": 0}, {"nperseg": 257}, {"step": 0}, {"step": 257}):
        assert _csd(h, p, **kw) == -1 and b"bad nperseg/step" in h.syg_last_error()
    for kw in ({"B": 0, "By": 1}, {"B": 65536, "By": 1}, {"L": 255}, {"ldx": 999}):
        assert _csd(h, p, **kw) == -1 and b"bad B/L/ldx" in h.syg_last_error()
    for By in (0, 3):
        assert _csd(h, p, By=By) == -1 and b"one row or B = 2 rows" in h.syg_last_error()
    assert _csd(h, p, ldy=999) == -1 and b"bad ldy" in h.syg_last_error()
    for d in (-1, 3):
        assert _csd(h, p, detrend=d) == -1 and b"detrend must be" in h.syg_last_error()


def test_rows_and_gcc_rejects(h, p):
    rows = lambda X=p, Y=p, rows=4, n=100, acc=p, first=1, last=1, nseg=4, outs=(p, p, p, p): \
        h.syg_csd_rows_f32(X, Y, rows, n, acc, first, last, nseg, 1.0, *outs, None)          # noqa: E731
    for kw in ({"X": None}, {"Y": None}, {"acc": None}):
        assert rows(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"rows": 0}, {"rows": 65536, "nseg": 70000}, {"n": 0}):
        assert rows(**kw) == -1 and b"bad rows / n" in h.syg_last_error()
    assert rows(nseg=3) == -1 and b"below the rows of this call" in h.syg_last_error()
    assert rows(outs=(None,) * 4) == -1 and b"no output asked for" in h.syg_last_error()
    wt = lambda X=p, Y=p, rows=2, ry=2, n=64, phat=1, out=p: h.syg_gcc_weight_c64(X, Y, rows, ry, n, phat, out, None)   # noqa: E731
    for kw in ({"X": None}, {"Y": None}, {"out": None}):
        assert wt(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"rows": 0, "ry": 1}, {"ry": 3}, {"rows": 65536, "ry": 1}):
        assert wt(**kw) == -1 and b"bad row counts" in h.syg_last_error()
    assert wt(n=0) == -1 and b"bad n" in h.syg_last_error()
    assert wt(phat=2) == -1 and b"0 (none) or 1 (phat)" in h.syg_last_error()
    cr = lambda c=p, rows=2, n=64, ml=10, out=p: h.syg_gcc_crop_f32(c, rows, n, ml, out, None)   # noqa: E731
    assert cr(c=None) == -1 and b"null pointer" in h.syg_last_error() and cr(out=None) == -1
    assert cr(rows=0) == -1 and b"bad rows / n" in h.syg_last_error()
    for ml in (-1, 32):
        assert cr(ml=ml) == -1 and b"does not fit n = 64" in h.syg_last_error()
    pk = lambda r=p, B=2, W=21, ldr=21, lag0=-10, fs=1.0, d=p, l=p, k=p: h.syg_peak_pick_f32(r, B, W, ldr, lag0, fs, d, l, k, None)   # noqa: E731,E741
    for kw in ({"r": None}, {"d": None}, {"l": None}, {"k": None}):
        assert pk(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in ({"B": 0}, {"W": 0}, {"ldr": 20}):
        assert pk(**kw) == -1 and b"bad B / W / ldr" in h.syg_last_error()
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        assert pk(fs=fs) == -1 and b"fs must be positive and finite" in h.syg_last_error()


def test_signatures():
    from sygnals_amd import ops
    import sygnals_amd.core.alignment as A
    import sygnals_amd.core.dsp as D
    assert list(inspect.signature(ops.cross_spectrum).parameters) == ["x", "y", "nperseg", "noverlap", "nfft", "window_host", "detrend",
                                                                      "scale", "want"]
    welch = list(inspect.signature(D.welch_batch).parameters)[1:]
    for fn in (D.csd_batch, D.cross_spectra_batch):
        assert list(inspect.signature(fn).parameters) == ["x", "y"] + welch + ["average"]
    assert list(inspect.signature(D.coherence_batch).parameters) == ["x", "y"] + [k for k in welch if k != "scaling"] + ["average"]
    for fn, ref in ((D.csd_batch, D.welch_batch), (D.compute_csd, D.compute_psd_welch)):
        for k, v in inspect.signature(ref).parameters.items():
            if k != "x":
                assert inspect.signature(fn).parameters[k].default == v.default
    sig = inspect.signature(A.gcc_batch)
    assert list(sig.parameters) == ["x", "y", "max_lag", "weighting"] and sig.parameters["weighting"].default == "none"
    for fn in (A.estimate_delay_batch, A.estimate_delay):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["x", "y", "fs", "max_lag", "weighting"]
        assert [sig.parameters[k].default for k in ("fs", "max_lag", "weighting")] == [1.0, None, "phat"]
    assert ops.csd_fused_takes(8) and ops.csd_fused_takes(8192) and not ops.csd_fused_takes(16384) and not ops.csd_fused_takes(100)
    assert not ops.csd_fused_takes(4)


def test_refusals_need_no_device():
    import sygnals_amd.core.alignment as A
    import sygnals_amd.core.dsp as D
    x = torch.zeros((3, 600), dtype=torch.float32)      # host tensors: anything that got further would fail on them
    for fn in (D.csd_batch, D.coherence_batch, D.cross_spectra_batch):
        for call, msg in ((lambda: fn(x, x, average="median"), "average='median' is not served"),
                          (lambda: fn(x.to(torch.complex64), x), "complex input is not served"),
                          (lambda: fn(x, x[:, :500]), "rows of unequal length are not served"),
                          (lambda: fn(x, x[:2]), "one row or one row per row of x (3), got 2"),
                          (lambda: fn(x[:, :0], x[:, :0]), "is empty"),
                          (lambda: fn(x[:0], x[:0]), "is empty"),
                          (lambda: fn(x, x, detrend="quadratic"), "Trend type must be"),
                          (lambda: fn(x, x, nperseg=64, noverlap=64), "noverlap must be less than nperseg")):
            with pytest.raises(ValueError) as e:
                call()
            assert msg in str(e.value)
            if "not served" in msg:
                assert "served: real float32 rows" in str(e.value)
    with pytest.raises(ValueError, match="Unknown scaling"):
        D.csd_batch(x, x, scaling="power")
    for fn in (D.compute_csd, D.compute_coherence):
        for call, msg in ((lambda: fn(np.zeros(100), np.zeros(90)), "rows of unequal length"),
                          (lambda: fn(np.zeros(0), np.zeros(0)), "empty input"),
                          (lambda: fn(np.zeros(8, dtype=complex), np.zeros(8)), "complex input is not served"),
                          (lambda: fn(np.zeros((2, 8)), np.zeros(8)), "must be a 1D array"),
                          (lambda: fn(np.zeros(100), np.zeros(100), average="median"), "average='median'")):
            with pytest.raises(ValueError) as e:
                call()
            assert msg in str(e.value)
    for fn in (A.gcc_batch, A.estimate_delay_batch):
        for call, msg in ((lambda: fn(x, x, weighting="scot"), "weighting 'scot' is not served"),
                          (lambda: fn(x, x, max_lag=600), "max_lag=600 is outside 0 ... min(Lx, Ly) - 1 = 599"),
                          (lambda: fn(x, x[:, :100], max_lag=100), "max_lag=100 is outside 0 ... min(Lx, Ly) - 1 = 99"),
                          (lambda: fn(x, x, max_lag=-1), "max_lag=-1 is outside"),
                          (lambda: fn(x, x, max_lag=1.5), "max_lag=1.5 is outside"),
                          (lambda: fn(x.to(torch.complex64), x), "complex input is not served"),
                          (lambda: fn(x, x[:2]), "one row or one row per row of x (3), got 2"),
                          (lambda: fn(x, x[:, :0]), "y is empty"),
                          (lambda: fn(np.zeros(8), x), "must be a [rows, samples] device tensor")):
            with pytest.raises(ValueError) as e:
                call()
            assert msg in str(e.value) and "served: real float32 rows" in str(e.value)
    for call, msg in ((lambda: A.estimate_delay(np.zeros(0), np.zeros(4)), "empty input"),
                      (lambda: A.estimate_delay(np.zeros((2, 4)), np.zeros(4)), "must be a 1D array"),
                      (lambda: A.estimate_delay(np.zeros(4, dtype=complex), np.zeros(4)), "complex input"),
                      (lambda: A.estimate_delay(np.zeros(4), np.zeros(4), fs=0.0), "fs must be positive"),
                      (lambda: A.estimate_delay(np.zeros(4), np.zeros(4), max_lag=4), "max_lag=4 is outside"),
                      (lambda: A.estimate_delay(np.zeros(4), np.zeros(4), weighting="roth"), "weighting 'roth'"),
                      (lambda: A.estimate_delay_batch(x, x, fs=float("nan")), "fs must be positive")):
        with pytest.raises(ValueError) as e:
            call()
        assert msg in str(e.value)


def test_plugin_registers_the_transforms():
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin
    names = []

    class Reg:
        def add_transform(self, name, fn):
            names.append(name)
    SygnalsAmdPlugin().register_transforms(Reg())
    assert {"compute_csd", "compute_coherence", "estimate_delay", "compute_psd_welch"} <= set(names)


def _wav(path, sr, n=4000, seed=0):
    from scipy.io import wavfile
    g = np.random.default_rng(seed)
    wavfile.write(str(path), sr, (g.standard_normal(n) * 3000).astype(np.int16))


def test_cli_usage_errors_and_outputs(tmp_path, monkeypatch):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    import sygnals_amd.core.alignment as A
    import sygnals_amd.core.dsp as D
    _wav(tmp_path / "a.wav", 16000)
    _wav(tmp_path / "b.wav", 8000, seed=1)
    _wav(tmp_path / "c.wav", 16000, seed=2)
    run = lambda *a: CliRunner().invoke(cli, ["dsp", *a])                                      # noqa: E731
    out = run("--help").output
    for c in ("csd", "coherence", "delay"):
        assert c in out
    for c in ("csd", "coherence"):
        out = run(c, "--help").output
        for opt in ("--fs", "--window", "--nperseg", "--noverlap", "--nfft", "--detrend", "--scaling", "-o, --output",
                    "INPUT_FILE_1", "INPUT_FILE_2"):
            assert opt in out
    out = run("delay", "--help").output
    for opt in ("--max-lag", "--max-delay", "--weighting", "[none|phat]"):
        assert opt in out
    # two inputs of unequal rate: a usage error that names `dsp resample`
    for c in ("csd", "coherence", "delay"):
        r = run(c, str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), "-o", str(tmp_path / "o.npz"))
        assert r.exit_code == 2 and "different sampling rates (16000 Hz and 8000 Hz)" in r.output and "dsp resample" in r.output
    r = run("delay", str(tmp_path / "a.wav"), str(tmp_path / "c.wav"), "-o", str(tmp_path / "o.npz"), "--max-lag", "3",
            "--max-delay", "0.1")
    assert r.exit_code == 2 and "cannot be combined" in r.output
    r = run("delay", str(tmp_path / "a.wav"), str(tmp_path / "c.wav"), "-o", str(tmp_path / "o.npz"), "--max-lag", "4000")
    assert r.exit_code == 2 and "max_lag=4000 is outside" in r.output
    r = run("delay", str(tmp_path / "a.wav"), str(tmp_path / "c.wav"), "-o", str(tmp_path / "o.npz"), "--weighting", "scot")
    assert r.exit_code == 2
    r = run("csd", str(tmp_path / "a.wav"), str(tmp_path / "c.wav"), "-o", str(tmp_path / "o.npz"), "--nperseg", "64",
            "--noverlap", "64")
    assert r.exit_code == 2 and "noverlap must be less than nperseg" in r.output
    r = run("csd", str(tmp_path / "a.wav"), "-o", str(tmp_path / "o.npz"))
    assert r.exit_code == 2                                                                    # the second input is required

    # outputs, with the device functions replaced by recorders (no GPU here)
    seen = {}

    def fake_csd(x, y, **kw):
        seen["csd"] = (x.shape, y.shape, kw)
        return np.arange(5.0), np.arange(5) * (1 + 1j)

    def fake_coh(x, y, **kw):
        seen["coh"] = kw
        return np.arange(5.0), np.linspace(0, 1, 5)

    def fake_delay(x, y, fs=1.0, max_lag=None, weighting="phat"):
        seen["delay"] = (fs, max_lag, weighting)
        return 0.25, 4, 0.9
    monkeypatch.setattr(D, "compute_csd", fake_csd)
    monkeypatch.setattr(D, "compute_coherence", fake_coh)
    monkeypatch.setattr(A, "estimate_delay", fake_delay)
    pair = (str(tmp_path / "a.wav"), str(tmp_path / "c.wav"))
    r = run("csd", *pair, "-o", str(tmp_path / "p.npz"), "--nperseg", "128", "--detrend", "none", "--scaling", "spectrum")
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "p.npz")
    assert set(z.files) == {"frequencies", "csd"} and z["csd"].dtype == np.complex128 and z["csd"].shape == (5,)
    shp_x, shp_y, kw = seen["csd"]
    assert shp_x == shp_y == (4000,) and kw["fs"] == 16000 and kw["nperseg"] == 128 and kw["detrend"] is False and kw["scaling"] == "spectrum"
    r = run("csd", *pair, "-o", str(tmp_path / "p.csv"))
    assert r.exit_code == 0, r.output
    t = pd.read_csv(tmp_path / "p.csv")
    assert list(t.columns) == ["Frequency (Hz)", "Real", "Imag", "Magnitude", "Phase"] and len(t) == 5
    assert np.allclose(t["Magnitude"], np.arange(5) * np.sqrt(2.0))
    r = run("coherence", *pair, "-o", str(tmp_path / "c.npz"), "--fs", "100")
    assert r.exit_code == 0 and set(np.load(tmp_path / "c.npz").files) == {"frequencies", "coherence"} and seen["coh"]["fs"] == 100.0
    r = run("coherence", *pair, "-o", str(tmp_path / "c.csv"))
    assert r.exit_code == 0 and list(pd.read_csv(tmp_path / "c.csv").columns) == ["Frequency (Hz)", "Coherence"]
    r = run("delay", *pair, "-o", str(tmp_path / "d.npz"), "--max-delay", "0.01", "--weighting", "none")
    assert r.exit_code == 0, r.output
    assert seen["delay"] == (16000, 160, "none")
    z = np.load(tmp_path / "d.npz")
    assert float(z["delay_seconds"]) == 0.25 and int(z["lag"]) == 4 and float(z["peak"]) == 0.9 and str(z["weighting"]) == "none"
    r = run("delay", *pair, "-o", str(tmp_path / "d.csv"), "--max-lag", "7")
    assert r.exit_code == 0 and seen["delay"] == (16000, 7, "phat")
    assert list(pd.read_csv(tmp_path / "d.csv").columns) == ["delay_seconds", "lag", "peak"]
