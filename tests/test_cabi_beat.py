"""The rhythm entries of the C ABI are declared, bound and exported and reject bad arguments before device work; so do the
Python layers above them and the `dsp beats` command."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_cabi_symbols import declared_functions

NEW = ["syg_beat_constants", "syg_tempogram_tile", "syg_tempogram_work_bytes", "syg_tempogram_f32", "syg_tempo_pick_work_bytes",
       "syg_tempo_pick_f32", "syg_beat_local_score_work_bytes", "syg_beat_local_score_f32", "syg_beat_dp_f32",
       "syg_beat_track_f32"]


@pytest.fixture(scope="module")
def h():
    from sygnals_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    buf = (C.c_double * 64)()
    return C.cast(buf, C.c_void_p)


def test_symbols_declared_bound_exported(h):
    from sygnals_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(raw, name)


def test_constants_and_sizes(h):
    from sygnals_amd import _rhythm as RH
    from sygnals_amd import ops
    k = ops.beat_constants()
    assert k == {name: h.syg_beat_constants(i) for i, name in enumerate(ops._BEAT_KEYS)} and h.syg_beat_constants(99) == -1
    assert (k["win_max"], k["period_max"], k["log_table"], k["max_elems"]) == (RH.WIN_MAX, RH.PERIOD_MAX, RH.LOG_TABLE, RH.MAX_ELEMS)
    assert k["dp_wave_period"] == 383 and 2 * k["period_max"] <= k["log_table"]
    # a tile's result stays within 48 KiB of LDS: 64 frames up to win_length 192, 4 at 2048
    assert [h.syg_tempogram_tile(w) for w in (2, 192, 193, 384, 385, 750, 1500, 2048)] == [64, 64, 32, 32, 16, 16, 8, 4]
    assert h.syg_tempogram_tile(1) == -1 and h.syg_tempogram_tile(2049) == -1
    # one partial row of the aggregate per 16 tiles of a clip
    assert h.syg_tempogram_work_bytes(3, 3001, 384, 1) == 3 * 6 * 384 * 8
    assert h.syg_tempogram_work_bytes(1, 384, 384, 0) == 384 * 8 and h.syg_tempogram_work_bytes(1, 383, 384, 0) == -1
    assert h.syg_tempogram_work_bytes(0, 10, 384, 1) == -1 and h.syg_tempogram_work_bytes(1, 10, 1, 1) == -1
    assert h.syg_tempo_pick_work_bytes(5) == 40 and h.syg_tempo_pick_work_bytes(0) == -1
    assert h.syg_beat_local_score_work_bytes(5) == 40 and h.syg_beat_local_score_work_bytes(0) == -1


def _tg(h, p, env=True, B=2, T=30, ld=30, win=8, center=1, window=True, norm=1, tg=True, agg=False, work=False, wb=0):
    return h.syg_tempogram_f32(p if env else None, B, T, ld, win, center, p if window else None, norm, p if tg else None,
                               p if agg else None, p if work else None, wb, None)


def test_tempogram_rejects(h, p):
    for kw in (dict(env=False), dict(window=False)):
        assert _tg(h, p, **kw) == -1 and b"null pointer" in h.syg_last_error()
    assert _tg(h, p, tg=False) == -1 and b"neither tg nor agg" in h.syg_last_error()
    for win in (1, 0, -3, 2049):
        assert _tg(h, p, win=win) == -1 and b"is outside 2 .. 2048" in h.syg_last_error()
    for kw in (dict(B=0), dict(T=0), dict(ld=29), dict(T=-1)):
        assert _tg(h, p, **kw) == -1 and b"bad B / T / ld" in h.syg_last_error()
    for norm in (2, -1):
        assert _tg(h, p, norm=norm) == -1 and b"norm must be" in h.syg_last_error()
    assert _tg(h, p, T=7, ld=7, center=0) == -1 and b"fewer than win_length" in h.syg_last_error()
    assert _tg(h, p, B=1, T=(1 << 20) + 1, ld=(1 << 20) + 1, win=2048) == -1 and b"more than 2^31" in h.syg_last_error()
    assert _tg(h, p, agg=True) == -1 and b"needs a workspace" in h.syg_last_error()
    assert _tg(h, p, agg=True, work=True, wb=8) == -1 and b"needs a workspace" in h.syg_last_error()


def test_pick_and_score_reject(h, p):
    def pick(a=True, tg=False, B=2, win=8, n=1, env=True, T=30, ld=30, lp=True, kstar=True, work=True):
        return h.syg_tempo_pick_f32(p if a else None, p if tg else None, B, win, n, p if env else None, T, ld, p if lp else None, p,
                                    p if kstar else None, p, p if work else None, None)
    assert pick(a=True, tg=True) == -1 and b"not both" in h.syg_last_error()
    assert pick(a=False, tg=False) == -1 and b"not both" in h.syg_last_error()
    for kw in (dict(env=False), dict(lp=False), dict(kstar=False), dict(work=False)):
        assert pick(**kw) == -1 and b"null pointer" in h.syg_last_error()
    assert pick(win=1) == -1 and b"is outside 2 .. 2048" in h.syg_last_error()
    for kw in (dict(B=0), dict(n=0), dict(n=2), dict(T=0), dict(ld=29)):
        assert pick(**kw) == -1 and b"bad B / n / T / ld" in h.syg_last_error()

    def score(env=True, B=2, T=30, ld=30, period=True, ls=True, work=True):
        return h.syg_beat_local_score_f32(p if env else None, B, T, ld, p if period else None, p if ls else None, p,
                                          p if work else None, None)
    for kw in (dict(env=False), dict(period=False), dict(ls=False), dict(work=False)):
        assert score(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in (dict(B=0), dict(T=0), dict(ld=29)):
        assert score(**kw) == -1 and b"bad B / T / ld" in h.syg_last_error()


def test_dp_and_track_reject(h, p):
    def dp(ls=True, B=2, T=30, period=True, pmax=40, tight=100.0, logtab=True, cum=True):
        return h.syg_beat_dp_f32(p if ls else None, p, B, T, p if period else None, pmax, tight, p if logtab else None,
                                 p if cum else None, p, None)
    for kw in (dict(ls=False), dict(period=False), dict(logtab=False), dict(cum=False)):
        assert dp(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in (dict(B=0), dict(T=0), dict(B=1 << 20, T=1 << 20)):
        assert dp(**kw) == -1 and b"bad B / T" in h.syg_last_error()
    for pmax in (1, 0, 2048):
        assert dp(pmax=pmax) == -1 and b"period_max" in h.syg_last_error()
    for t in (0.0, -1.0, float("nan"), float("inf")):
        assert dp(tight=t) == -1 and b"tightness must be positive" in h.syg_last_error()

    def track(ls=True, cum=True, back=True, B=2, T=30, period=True, beats=True, count=True):
        return h.syg_beat_track_f32(p if ls else None, p if cum else None, p if back else None, B, T, p if period else None, 1,
                                    p if beats else None, p if count else None, None, None)
    for kw in (dict(ls=False), dict(cum=False), dict(back=False), dict(period=False), dict(beats=False), dict(count=False)):
        assert track(**kw) == -1 and b"null pointer" in h.syg_last_error()
    for kw in (dict(B=0), dict(T=0)):
        assert track(**kw) == -1 and b"bad B / T" in h.syg_last_error()


def test_python_layers_refuse_before_device_work(monkeypatch):
    from sygnals_amd import ops
    from sygnals_amd.core import rhythm as RY
    from sygnals_amd.core.audio import features as AF

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    for name in ("_call", "to_device_f32", "require_gpu"):
        monkeypatch.setattr(ops, name, no_device)
    monkeypatch.setattr(AF, "onset_strength_batch", no_device)
    env = np.ones((2, 40), dtype=np.float32)
    t = torch.ones((2, 40))
    for win in (1, 0, 2049, 3.0, None):
        with pytest.raises(ValueError, match="win_length"):
            ops.tempogram(t, win_length=win)
        with pytest.raises(ValueError, match="win_length"):
            RY.tempogram_batch(onset_envelope=env, win_length=win)
    for norm in (1, 2, "max", 0):
        with pytest.raises(ValueError, match="norm=.*not served"):
            ops.tempogram(t, norm=norm)
        with pytest.raises(ValueError, match="norm=.*not served"):
            RY.tempogram(onset_envelope=env[0], norm=norm)
    with pytest.raises(ValueError, match="fewer than win_length"):
        ops.tempogram(t, win_length=41, center=False)
    with pytest.raises(ValueError, match="more than 2\\^31 elements"):
        ops.tempogram(torch.empty((1, (1 << 20) + 1)), win_length=2048)
    with pytest.raises(ValueError, match="float32 tensor \\[B, T\\]"):
        ops.tempogram(t.double())
    for fn in (RY.tempo_batch, RY.beat_track_batch):
        with pytest.raises(ValueError, match="prior= distributions are not served"):
            fn(onset_envelope=env, prior=object())
    for agg in (np.median, "median", np.max):
        with pytest.raises(ValueError, match="aggregate=.*not served"):
            RY.tempo_batch(onset_envelope=env, aggregate=agg)
        with pytest.raises(ValueError, match="aggregate=.*not served"):
            RY.tempo(onset_envelope=env[0], aggregate=agg)
    with pytest.raises(ValueError, match="win_length=5512 is outside"):          # ac_size 64 s at 22050 / 256
        RY.tempo_batch(onset_envelope=env, hop_length=256, ac_size=64.0)
    for tight in (0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="tightness=.*strictly positive"):
            RY.beat_track_batch(onset_envelope=env, tightness=tight)
        with pytest.raises(ValueError, match="tightness"):
            ops.beat_dp(t, t[:, 0], 20, tightness=tight)
    for bpm in (0, -120.0, float("nan"), [120.0, 0.0]):
        with pytest.raises(ValueError, match="bpm must be strictly positive"):
            RY.beat_track_batch(onset_envelope=env, bpm=bpm)
    with pytest.raises(ValueError, match="beat period below 2 frames"):
        RY.beat_track_batch(onset_envelope=env, bpm=2000.0)                     # 60 * 43.07 / 2000 rounds to 1
    with pytest.raises(ValueError, match="beat period above 2047"):
        RY.beat_track_batch(onset_envelope=env, bpm=1.0)
    with pytest.raises(ValueError, match="time-varying bpm"):
        RY.beat_track(onset_envelope=env[0], bpm=[100.0, 110.0])
    with pytest.raises(ValueError, match="invalid unit type"):
        RY.beat_track(onset_envelope=env[0], units="beats")
    with pytest.raises(ValueError, match="either the audio y or onset_envelope"):
        RY.beat_track_batch()
    with pytest.raises(ValueError, match="1D array"):
        RY.beat_track(onset_envelope=env)


def test_host_tables():
    from sygnals_amd import _rhythm as RH
    from tests import beat_ref as R
    assert np.array_equal(RH.log_table(), R.L)
    for sr, hop in ((22050, 512), (48000, 256)):
        win = RH.tempo_win_length(8.0, sr, hop, "tempo")
        for kw in (dict(), dict(start_bpm=90.0, std_bpm=0.5, max_tempo=None)):
            got, want = RH.tempo_prior(win, sr, hop, **kw), R.prior(win, sr, hop, **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(RH.window_table("hann", 384).astype(np.float64), R.window32("hann", 384))
    assert RH.periods_from_bpm([120.0, 60.0, 172.265625], 3, 22050, 512, "x").tolist() == [22, 43, 15]
    assert RH.periods_from_bpm(60.0 * 22050 / 512 / 2.5, 2, 22050, 512, "x").tolist() == [2, 2]      # 2.5 rounds to even


def test_signatures_and_exports():
    from sygnals_amd.core import rhythm as RY
    from sygnals_amd.core import segmentation as SG
    from sygnals_amd import ops
    assert RY.__all__ == ["tempogram_batch", "tempo_batch", "beat_track_batch", "tempogram", "tempo", "beat_track"]
    sig = inspect.signature(RY.beat_track)
    assert list(sig.parameters)[:8] == ["y", "sr", "onset_envelope", "hop_length", "start_bpm", "tightness", "trim", "bpm"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["sr"], d["hop_length"], d["start_bpm"], d["tightness"], d["trim"], d["bpm"], d["units"]) == \
        (22050, 512, 120.0, 100, True, None, "frames")
    d = {k: v.default for k, v in inspect.signature(RY.tempo).parameters.items()}
    assert (d["start_bpm"], d["std_bpm"], d["ac_size"], d["max_tempo"], d["aggregate"]) == (120.0, 1.0, 8.0, 320.0, np.mean)
    d = {k: v.default for k, v in inspect.signature(RY.tempogram).parameters.items()}
    assert (d["win_length"], d["center"], d["window"], d["norm"]) == (384, True, "hann", np.inf)
    assert callable(SG.segment_by_beats)
    for name in ("tempogram", "tempo_pick", "beat_local_score", "beat_dp", "beat_track", "beat_constants"):
        assert callable(getattr(ops, name))


def test_plugin_registers_beat_track_and_tempo():
    from sygnals_amd.core import rhythm as RY
    from sygnals_amd.plugins.plugin import SygnalsAmdPlugin

    class Reg:
        def __init__(self): self.t = {}
        def add_transform(self, n, f): self.t[n] = f
    reg = Reg()
    SygnalsAmdPlugin().register_transforms(reg)
    assert reg.t["beat_track"] is RY.beat_track and reg.t["tempo"] is RY.tempo


def test_cli_usage_errors(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from sygnals_amd.cli import main as M
    from sygnals_amd.core import rhythm as RY
    src = tmp_path / "x.csv"
    src.write_text("value\n0.0\n1.0\n")
    run = CliRunner().invoke
    for bad in (["--bpm", "0"], ["--bpm", "-90"], ["--tightness", "0"], ["--tightness", "-5"], ["--hop-length", "0"]):
        r = run(M.cli, ["dsp", "beats", str(src), "-o", str(tmp_path / "o.npz"), *bad])
        assert r.exit_code == 2 and "must be positive" in r.output, r.output
    r = run(M.cli, ["dsp", "beats", str(src), "-o", str(tmp_path / "o.npz"), "--units", "bars"])
    assert r.exit_code == 2
    r = run(M.cli, ["dsp", "beats", str(src)])
    assert r.exit_code == 2 and "--output" in r.output
    r = run(M.cli, ["dsp", "beats", str(src), "-o", str(tmp_path / "o.npz")])
    assert r.exit_code == 2 and "sampling rate" in r.output
    # what the command writes, with the tracker replaced
    seen = {}

    def fake(x, **kw):
        seen.update(kw)
        return 120.0, np.array([4, 26, 48])
    monkeypatch.setattr(RY, "beat_track", fake)
    monkeypatch.setattr(M, "_load_signal", lambda f, s: (np.zeros(4096), 22050))
    r = run(M.cli, ["dsp", "beats", str(src), "-o", str(tmp_path / "o.npz"), "--no-trim", "--bpm", "100", "--units", "samples"])
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "o.npz")
    assert set(z.files) == {"tempo", "beats", "hop_length", "units"} and z["beats"].tolist() == [2048, 13312, 24576]
    assert float(z["tempo"]) == 120.0 and int(z["hop_length"]) == 512 and str(z["units"]) == "samples"
    assert seen["trim"] is False and seen["bpm"] == 100.0 and seen["units"] == "frames"
    r = run(M.cli, ["dsp", "beats", str(src), "-o", str(tmp_path / "o.csv")])
    assert r.exit_code == 0, r.output
    import pandas as pd
    df = pd.read_csv(tmp_path / "o.csv")
    assert list(df.columns) == ["index", "frame", "time"] and df["frame"].tolist() == [4, 26, 48]
    assert np.allclose(df["time"], np.array([4, 26, 48]) * 512 / 22050)
