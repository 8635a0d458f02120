"""Tempogram, tempo and beat tracking on the device (syg_tempogram_f32, syg_tempo_pick_f32, syg_beat_local_score_f32,
syg_beat_dp_f32, syg_beat_track_f32) against the float64 restatement of tests/beat_ref.py.

G1 and G3 are the usual 1e-5 gates.  The decisions (G2) are compared bit for bit with the restatement fed the device's own
float32 numbers; the chain (G4) with the pure float64 chain, on inputs that meet conditions (a) and (b) of tests/beat_cases.py.
"""
import numpy as np
import pytest
import torch

from sygnals_amd import ops
from sygnals_amd.core import rhythm as RY
from sygnals_amd.core import segmentation as SEG
from tests import beat_cases as K
from tests import beat_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
WORST = {}


def _note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))
    print(f"{key}: worst so far {WORST[key]:.3e}")


def _dev(x):
    return ops.to_device_f32(np.atleast_2d(x))


def _rows(T, seed, B=3):
    """Random rows, with a unit impulse at the first, a middle and the last frame and an all-zero row among them."""
    rng = np.random.default_rng(seed)
    env = rng.random((B + 4, T)).astype(np.float32)
    env[B:] = 0.0
    env[B, 0] = env[B + 1, T // 2] = env[B + 2, T - 1] = 1.0
    return env


def _check_tempogram(env, win, center, window="hann"):
    """tg, the unnormalised r and the aggregate of envelopes env [B, T] against the restatement; outputs into NaN."""
    B, T = env.shape
    n = T if center else T - win + 1
    d = _dev(env)
    out = torch.full((B, win, n), float("nan"), device=d.device)
    tg, a = ops.tempogram(d, win, center, window, aggregate="also", out=out)
    assert tg is out and a.dtype == torch.float64 and a.shape == (B, win)
    tg, a = tg.cpu().numpy(), a.cpu().numpy()
    raw = ops.tempogram(d, win, center, window, norm=None).cpu().numpy()
    only = ops.tempogram(d, win, center, window, aggregate="only").cpu().numpy()
    assert np.isfinite(tg).all() and np.isfinite(raw).all() and np.array_equal(only, a)
    for b in range(B):
        r = R.autocorr(env[b], win, center, window)
        ref = R.normalise(r)
        peak = np.max(np.abs(r))
        _note("G1 normalised", np.max(np.abs(tg[b] - ref)))
        assert np.max(np.abs(tg[b] - ref)) <= TOL, f"tempogram win={win} T={T} center={center} row {b}"
        if peak > 0:
            _note("G1 unnormalised / max|r|", np.max(np.abs(raw[b] - r)) / peak)
        assert np.max(np.abs(raw[b] - r)) <= TOL * peak, f"autocorrelation win={win} T={T} center={center} row {b}"
        assert np.max(np.abs(a[b] - R.aggregate(ref))) <= TOL, f"aggregate win={win} T={T} row {b}"
        if not env[b].any():
            assert not tg[b].any() and not raw[b].any() and not a[b].any()
    return tg, a


# ------------------------------------------------------------------------------------------------------- G1: tempogram
@pytest.mark.parametrize("win", [2, 3, 8, 63, 64, 65])
def test_tempogram_small_windows(win):
    tile = ops.tempogram_tile(win)
    for T in sorted({1, 2, max(1, win - 1), win, win + 1, tile - 1, tile, tile + 1}):
        _check_tempogram(_rows(T, 100 * win + T), win, True)
        if T >= win:
            _check_tempogram(_rows(T, 100 * win + T + 7), win, False)


def test_tempogram_default_window_length():
    win, tile = 384, ops.tempogram_tile(384)
    assert tile == 32
    for T in (1, 2, tile - 1, tile, tile + 1, win - 1, win, win + 1):
        _check_tempogram(_rows(T, T, B=1)[[0, 2]] if T > 2 else _rows(T, T, B=1)[:1], win, True)
    for T in (win, win + 1):
        _check_tempogram(_rows(T, T + 1, B=1)[:1], win, False)
    _check_tempogram(_rows(40, 9, B=1)[:1], win, True, window="hamming")


def test_tempogram_longest_window_once():
    _check_tempogram(_rows(6, 2048, B=1)[[0, 3]], 2048, True)


def test_tempogram_many_rows_slices_and_strides():
    win = 8
    per_slice = ops.beat_constants()["slice_tiles"] * ops.tempogram_tile(win)
    for B in (1, 3, 33):
        rng = np.random.default_rng(B)
        T = per_slice + 5 if B == 3 else 40                       # B = 3: two partial rows behind the aggregate
        big = rng.random((2 * B, T + 3)).astype(np.float32)
        d = ops.to_device_f32(big)[::2, 1:T + 1]                  # rows two apart, starting one sample in
        assert d.stride(0) == 2 * (T + 3) and d.stride(1) == 1
        tg, a = ops.tempogram(d, win, aggregate="also")
        want, wa = _check_tempogram(big[::2, 1:T + 1].copy(), win, True)
        assert np.array_equal(tg.cpu().numpy(), want) and np.array_equal(a.cpu().numpy(), wa)
        for b in range(0, B, 16):                                 # a batch equals its rows
            one, a1 = ops.tempogram(d[b:b + 1], win, aggregate="also")
            assert np.array_equal(one[0].cpu().numpy(), want[b]) and np.array_equal(a1[0].cpu().numpy(), wa[b])
        again, a2 = ops.tempogram(d, win, aggregate="also")
        assert torch.equal(again, tg) and torch.equal(a2, a)


# --------------------------------------------------------------------------------------------------- G3: local score
@pytest.mark.parametrize("P,T", [(2, 1), (2, 7), (3, 50), (21, 300), (64, 1500), (383, 1030), (2047, 5000)])
def test_local_score(P, T):
    env = np.stack([R.click_envelope(T, max(2, P), 1, 1.0, 0.3, P + i) for i in range(2)] + [np.zeros(T, dtype=np.float32)])
    ls, lsmax = ops.beat_local_score(_dev(env), [P] * 3)
    ls, lsmax = ls.cpu().numpy(), lsmax.cpu().numpy()
    assert np.array_equal(lsmax, ls.max(axis=1)) and not ls[2].any()
    for b in range(2):
        ref = R.local_score(env[b], P)
        bound = TOL * np.sum(R.taps(P)) * np.max(np.abs(R.scaled(env[b])))
        _note("G3 / (|g|_1 max|e|)", np.max(np.abs(ls[b] - ref)) / (bound / TOL))
        assert np.max(np.abs(ls[b] - ref)) <= bound, f"local score P={P} T={T} row {b}"
    pd = torch.tensor([P, 0, 1], dtype=torch.int32, device="cuda")            # periods below 2: no score
    z = ops.beat_local_score(_dev(env), pd)[0].cpu().numpy()
    assert np.array_equal(z[0], ls[0]) and not z[1:].any()


# ------------------------------------------------------------------------- G2: decisions on the device's own numbers
def _check_beats(env, periods, tightness=100.0, trim=True, period_max=None):
    """cum, back, the last beat and the beats of envelopes env [B, T], bit for bit against the restatement fed the
    device's float32 local score; every output into NaN / -2."""
    B, T = env.shape
    d = _dev(env)
    pd = torch.tensor(np.asarray(periods, dtype=np.int32), device=d.device)
    ls, lsmax = ops.beat_local_score(d, pd)
    cum = torch.full((B, T), float("nan"), dtype=torch.float64, device=d.device)
    back = torch.full((B, T), -2, dtype=torch.int32, device=d.device)
    beats = torch.full((B, T), -2, dtype=torch.int32, device=d.device)
    count = torch.full((B,), -2, dtype=torch.int32, device=d.device)
    ops.beat_dp(ls, lsmax, pd, tightness, period_max=period_max or max(2, int(max(periods))), out=(cum, back))
    _, _, last = ops.beat_track(ls, cum, back, pd, trim, out=(beats, count))
    ls, cum, back, beats, count, last = (t.cpu().numpy() for t in (ls, cum, back, beats, count, last))
    for b in range(B):
        wb, wl, wc, wk = R.beats_from(ls[b], int(periods[b]), tightness, trim)
        what = f"P={periods[b]} T={T} tightness={tightness} trim={trim} row {b}"
        assert np.array_equal(cum[b], wc), "cum " + what
        assert np.array_equal(back[b], wk), "back " + what
        assert last[b] == wl, "last beat " + what
        assert count[b] == len(wb) and np.array_equal(beats[b, :count[b]], wb) and np.all(beats[b, count[b]:] == -1), "beats " + what
    return beats, count


def _click_rows(T, P, B=2, seed=0):
    return np.stack([R.click_envelope(T, max(2, P), (3 * i) % max(2, P), 1.0, 0.1, seed + i) for i in range(B)])


@pytest.mark.parametrize("P", [2, 3, 21])
def test_dp_every_short_length(P):
    for T in range(1, 2 * P + 3):
        _check_beats(_click_rows(T, P, seed=T), [P, P])
    for tight in (1.0, 400.0):
        for trim in (True, False):
            _check_beats(_click_rows(700, P, seed=P), [P, P], tight, trim)


@pytest.mark.parametrize("P", [63, 64, 65, 383])
def test_dp_kernel_tiers(P):
    for T in (range(1, 2 * P + 3) if P < 100 else (1, 2, 3, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2 * P + 2)):
        _check_beats(_click_rows(T, P, seed=T), [P, P])
    beats, count = _check_beats(_click_rows(3000, P, seed=P), [P, P])
    assert count.min() >= 3000 // P - 4
    _check_beats(_click_rows(3000, P, seed=P + 1), [P, P], 400.0, False)
    if P == 63:                                                  # the same rows under the wider kernels: same bits
        for pmax in (84, 85, 383, 384, 2047):
            b2, c2 = _check_beats(_click_rows(3000, P, seed=P), [P, P], period_max=pmax)
            assert np.array_equal(b2, beats) and np.array_equal(c2, count)


def test_dp_longest_period_once():
    _check_beats(_click_rows(5000, 2047, B=1, seed=5), [2047])


def test_dp_ragged_batch():
    rng = np.random.default_rng(33)
    periods = rng.integers(2, 90, 33)
    periods[:4] = [1, 0, 2, 89]                                   # rows below 2 get no beats
    env = np.stack([R.click_envelope(2500, max(2, int(p)), int(rng.integers(0, max(2, int(p)))), 1.0, 0.1, 100 + i)
                    for i, p in enumerate(periods)])
    env[5] = 0.0
    env[6] = 0.7                                                  # a constant row: not scaled, tracked like any other
    beats, count = _check_beats(env, periods, period_max=383)
    assert count[0] == count[1] == count[5] == 0 and count[2:5].min() > 0
    d = _dev(env)
    for b in (2, 3, 17):                                          # a batch equals its rows
        ls, m = ops.beat_local_score(d[b:b + 1], [int(periods[b])])
        cum, back = ops.beat_dp(ls, m, [int(periods[b])], period_max=383)
        one, c1, _ = ops.beat_track(ls, cum, back, [int(periods[b])])
        assert np.array_equal(one[0].cpu().numpy(), beats[b]) and int(c1[0]) == count[b]


def test_tempo_pick_on_the_device_aggregate():
    names = sorted(K.ENV_CASES)
    bpms, lp = R.prior(K.WIN, K.SR, K.HOP)
    rng = np.random.default_rng(3)
    rows = [K.envelope(n) for n in names] + [rng.random(200).astype(np.float32), np.zeros(64, dtype=np.float32)]
    held = 0
    for env in rows:
        d = _dev(env)
        a = ops.tempogram(d, K.WIN, aggregate="only")
        k, bpm = ops.tempo_pick(a, d, lp, bpms)
        k, bpm, a = int(k[0]), float(bpm[0]), a[0].cpu().numpy()
        if not env.any():
            assert (k, bpm) == (0, 0.0)
            continue
        if K.condition_a(a, lp):
            held += 1
            assert k == R.tempo_pick(a, lp) and bpm == bpms[k]
    assert held >= len(names)
    # one tempo per frame, and a start_bpm / max_tempo of the caller's
    env = K.envelope(names[0])[:90]
    d = _dev(env)
    bp2, lp2 = R.prior(K.WIN, K.SR, K.HOP, start_bpm=90.0, std_bpm=0.5, max_tempo=None)
    tg = ops.tempogram(d, K.WIN)
    k, bpm = ops.tempo_pick(tg, d, lp2, bp2)
    k, bpm, tg = k[0].cpu().numpy(), bpm[0].cpu().numpy(), tg[0].cpu().numpy()
    assert k.shape == (90,)
    sure = [t for t in range(90) if K.condition_a(tg[:, t], lp2)]
    assert len(sure) >= 45
    for t in sure:
        assert k[t] == R.tempo_pick(tg[:, t], lp2) and bpm[t] == bp2[k[t]]


# ------------------------------------------------------------------------------------------------- G4: the whole chain
def test_chain_from_envelopes():
    for name in sorted(K.ENV_CASES):
        ref = K.reference(name)
        assert K.condition_a(ref["a"], ref["logprior"]) and K.condition_b(ref["env"], ref["k"])
        tempo, beats, count = RY.beat_track_batch(onset_envelope=ref["env"][None, :], sr=K.SR, hop_length=K.HOP)
        assert tempo.dtype == torch.float64 and float(tempo[0]) == ref["tempo"]
        assert np.array_equal(beats[0, :int(count[0])].cpu().numpy(), ref["beats"])
        t1, b1 = RY.beat_track(onset_envelope=ref["env"], sr=K.SR, hop_length=K.HOP, units="time")
        assert t1 == ref["tempo"] and np.array_equal(b1, ref["beats"] * K.HOP / float(K.SR))
        assert RY.tempo(onset_envelope=ref["env"], sr=K.SR, hop_length=K.HOP).tolist() == [ref["tempo"]]
        # a tempo of the caller's
        P = R.period_of(110.0, K.SR, K.HOP)
        assert K.condition_b(ref["env"], P)
        t2, b2 = RY.beat_track(onset_envelope=ref["env"], sr=K.SR, hop_length=K.HOP, bpm=110.0)
        assert t2 == 110.0 and np.array_equal(b2, R.beat_track(ref["env"], P))
    z = np.zeros((2, 80), dtype=np.float32)
    z[1] = K.envelope("p20")[:80]
    for bpm in (None, 100.0, [100.0, 129.19921875]):
        tempo, beats, count = RY.beat_track_batch(onset_envelope=z, sr=K.SR, hop_length=K.HOP, bpm=bpm)
        assert float(tempo[0]) == 0.0 and int(count[0]) == 0 and torch.all(beats[0] == -1) and float(tempo[1]) > 0


def _click_audio(sr, seconds, period_samples, seed):
    rng = np.random.default_rng(seed)
    y = 1e-3 * rng.standard_normal(int(sr * seconds))
    burst = np.hanning(256) * np.sin(2 * np.pi * 1000.0 * np.arange(256) / sr)
    for s in range(period_samples // 3, len(y) - 256, period_samples):
        y[s:s + 256] += burst
    return y.astype(np.float32)


def test_chain_from_audio_segments_and_cli(tmp_path):
    from click.testing import CliRunner
    from scipy.io import wavfile
    from sygnals_amd.cli import main as M
    from sygnals_amd.core.audio import features as F
    sr, hop = K.SR, K.HOP
    clips = np.stack([_click_audio(sr, 6.0, 20 * hop, 1), _click_audio(sr, 6.0, 24 * hop, 2)])
    env = F.onset_strength_batch(clips, sr, hop_length=hop).cpu().numpy()
    tempo, beats, count = RY.beat_track_batch(clips, sr, hop_length=hop)
    again = RY.beat_track_batch(clips, sr, hop_length=hop)
    assert torch.equal(again[0], tempo) and torch.equal(again[1], beats) and torch.equal(again[2], count)
    bpms, lp = R.prior(K.WIN, sr, hop)
    for b in range(2):
        a = R.aggregate(R.tempogram(env[b], K.WIN))
        k = R.tempo_pick(a, lp)
        assert K.condition_a(a, lp) and K.condition_b(env[b], k), f"clip {b}: the input does not meet the conditions"
        want = R.beat_track(env[b], k)
        assert float(tempo[b]) == bpms[k] and np.array_equal(beats[b, :int(count[b])].cpu().numpy(), want)
        assert len(want) >= 5 and np.all(np.abs(np.diff(want) - (20, 24)[b]) <= 1)
        one = RY.beat_track_batch(clips[b:b + 1], sr, hop_length=hop)                       # a batch equals its rows
        assert float(one[0][0]) == float(tempo[b]) and np.array_equal(one[1][0].cpu().numpy(), beats[b].cpu().numpy())
        t1, times = RY.beat_track(clips[b], sr=sr, hop_length=hop, units="time")
        assert t1 == float(tempo[b]) and np.array_equal(times, want * hop / float(sr))
        assert RY.beat_track(clips[b], sr=sr, hop_length=hop, units="samples")[1].tolist() == (want * hop).tolist()
        seg = SEG.segment_by_beats(clips[b], sr, hop_length=hop)
        assert seg == SEG.segment_by_event(clips[b], sr, times)
        assert len(seg) == len(want)
    # the command on a file agrees with the batch call on what the file holds
    wavfile.write(tmp_path / "c.wav", sr, np.round(clips[0] * 20000).astype(np.int16))
    y, sr2 = M._load_signal(str(tmp_path / "c.wav"), None)
    t, bt, ct = RY.beat_track_batch(np.asarray(y)[None, :], sr2, hop_length=hop)
    frames = bt[0, :int(ct[0])].cpu().numpy()
    r = CliRunner().invoke(M.cli, ["dsp", "beats", str(tmp_path / "c.wav"), "-o", str(tmp_path / "b.npz")])
    assert r.exit_code == 0, r.output
    z = np.load(tmp_path / "b.npz")
    assert float(z["tempo"]) == float(t[0]) and str(z["units"]) == "time" and int(z["hop_length"]) == hop
    assert np.array_equal(z["beats"], frames * hop / float(sr2)) and len(frames) >= 5
    r = CliRunner().invoke(M.cli, ["dsp", "beats", str(tmp_path / "c.wav"), "-o", str(tmp_path / "b.csv"), "--units", "frames",
                                   "--bpm", "129.2", "--no-trim"])
    assert r.exit_code == 0, r.output
    import pandas as pd
    tab = pd.read_csv(tmp_path / "b.csv")
    t3, b3, c3 = RY.beat_track_batch(np.asarray(y)[None, :], sr2, hop_length=hop, bpm=129.2, trim=False)
    assert tab["frame"].tolist() == b3[0, :int(c3[0])].cpu().numpy().tolist() and float(t3[0]) == 129.2


def test_tempogram_batch_and_single_clip_from_audio():
    y = _click_audio(K.SR, 2.0, 20 * K.HOP, 4)
    tb = RY.tempogram_batch(y[None, :], K.SR, hop_length=K.HOP, win_length=64)
    env = ops.to_device_f32(y[None, :])
    from sygnals_amd.core.audio import features as F
    want = ops.tempogram(F.onset_strength_batch(env, K.SR, hop_length=K.HOP), 64)
    assert torch.equal(tb, want) and tb.shape == (1, 64, 1 + len(y) // K.HOP)
    assert np.array_equal(RY.tempogram(y, K.SR, hop_length=K.HOP, win_length=64), want[0].cpu().numpy())
    per_frame = RY.tempo(y, K.SR, hop_length=K.HOP, aggregate=None)
    assert per_frame.shape == (1 + len(y) // K.HOP,) and per_frame.dtype == np.float64
