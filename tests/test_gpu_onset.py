"""Onset detection on the device (syg_onset_strength_f32, syg_onset_peaks_f32, syg_clip_metrics_f32, detect_onsets,
get_basic_audio_metrics, segment_by_silence, segment_by_onsets) against the float64 restatement of tests/onset_ref.py."""
import numpy as np
import pytest
import torch

from sygnals_amd import ops
from sygnals_amd.core import segmentation as SEG
from sygnals_amd.core.audio import features as F
from tests import onset_ref as R
from tests.gpu_util import assert_parity

pytestmark = pytest.mark.gpu

TOL = R.TOL


def _parity_clips(sr):
    """Tone bursts over a 1e-3 noise floor, bursts over digital silence, noise only, and a 9000-sample clip."""
    L = sr
    clips = [R.burst_clip(sr, L, 11), R.burst_clip(sr, L, 12, floor=0.0), 0.1 * np.random.default_rng(13).standard_normal(L),
             R.burst_clip(sr, 9000, 14)]
    return [c.astype(np.float32).astype(np.float64) for c in clips]


# ---------------------------------------------------------------- envelope
@pytest.mark.parametrize("sr,n_fft,hop", [(22050, 2048, 512), (48000, 2048, 512), (16000, 1024, 256), (48000, 4096, 1024)])
@pytest.mark.parametrize("opt", [dict(), dict(lag=2), dict(max_size=3), dict(center=False), dict(detrend=True),
                                 dict(lag=2, max_size=3, detrend=True)])
def test_envelope_parity(sr, n_fft, hop, opt):
    for i, y in enumerate(_parity_clips(sr)):
        env = F.onset_strength_batch(y[None, :], sr, n_fft=n_fft, hop_length=hop, **opt)[0].cpu().numpy()
        ref = R.onset_strength(y, sr, n_fft=n_fft, hop_length=hop, **opt)
        err = np.abs(env - ref).max() / max(np.abs(ref).max(), 1e-300)
        print(f"envelope sr={sr} n_fft={n_fft} hop={hop} {opt} clip {i}: peak-relative error {err:.3e}")
        assert_parity(env, ref, TOL, f"onset envelope sr={sr} n_fft={n_fft} {opt} clip {i}")


def test_envelope_kernel_alone_on_reference_mel():
    """The kernel on the restatement's own mel powers (rounded to float32): only the dB conversion and the flux differ."""
    from oracle import cpu_ref as O
    sr, n_fft, hop = 22050, 2048, 512
    for lag, k in ((1, 1), (2, 3), (1, 4)):
        for y in _parity_clips(sr):
            D = O.stft(y, n_fft=n_fft, hop_length=hop)
            P = (O.mel_filterbank(sr, n_fft, 128, 0.0, sr / 2.0).astype(np.float64) @ (np.abs(D) ** 2)).astype(np.float32)
            S = O.power_to_db(P.astype(np.float64), ref=1.0, amin=1e-10, top_db=80.0)
            ref = R.onset_strength_from_db(S, n_fft, hop, lag, k)
            env = ops.onset_strength(ops.to_device_f32(P[None]), lag, k, lag + 2, P.shape[1])[0].cpu().numpy()
            assert_parity(env, ref, TOL, f"flux alone lag={lag} max_size={k}")


def test_envelope_long_clip_matches_its_pieces():
    """More than 2048 frames: the sliced form (clip maximum from a first launch) against the restatement on the same mel."""
    from oracle import cpu_ref as O
    rng = np.random.default_rng(5)
    M, T = 128, 5000
    P = (rng.random((M, T)) ** 8 * 10.0 ** rng.uniform(-6, 2, size=(1, T))).astype(np.float32)
    S = O.power_to_db(P.astype(np.float64), ref=1.0, amin=1e-10, top_db=80.0)
    for lag, k, det in ((1, 1, False), (2, 3, True)):
        ref = R.onset_strength_from_db(S, 2048, 512, lag, k, True, det)
        env = ops.onset_strength(ops.to_device_f32(P[None]), lag, k, lag + 2, T, detrend=det)[0].cpu().numpy()
        assert_parity(env, ref, TOL, f"long clip lag={lag} max_size={k}")


def test_envelope_repeat_runs_are_bit_identical_and_batch_equals_single():
    sr = 22050
    Y = R.gpu_clips(sr, 33075, n=6)
    a = F.onset_strength_batch(Y, sr)
    b = F.onset_strength_batch(Y, sr)
    assert torch.equal(a, b)
    for i in (0, 3, 5):
        assert torch.equal(F.onset_strength_batch(Y[i:i + 1], sr)[0], a[i])


# ---------------------------------------------------------------- peak picking in isolation
def _envelope(T, seed):
    rng = np.random.default_rng(seed)
    e = np.convolve(np.maximum(rng.standard_normal(T + 4), 0.0) ** 2, np.hanning(5), mode="valid")
    return (e + 0.01 * rng.random(T)).astype(np.float32)


def _device_peaks(env, **kw):
    fr, cnt = ops.onset_peaks(ops.to_device_f32(env[None, :]), **kw)
    fr = fr[0].cpu().numpy()
    n = int(cnt[0].item())
    assert (fr[n:] == -1).all()
    return fr[:n].astype(np.int64)


WINDOWS = [R.default_windows(22050, 512), R.default_windows(48000, 512), R.default_windows(16000, 256)]


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 1000, 337501])
@pytest.mark.parametrize("wi", [0, 1, 2, 3])
def test_peaks_match_restatement(T, wi):
    if wi < 3:
        pk = dict(WINDOWS[wi])
    elif T <= 1000:                                # windows wider than the clip
        pk = dict(pre_max=T + 3, post_max=T + 5, pre_avg=T + 2, post_avg=T + 7, delta=0.05, wait=3)
    else:                                          # (a window costs T loads per frame: wide ones stay on short clips)
        pk = dict(pre_max=40, post_max=40, pre_avg=40, post_avg=41, delta=0.05, wait=40)
    for seed in range(3 if T <= 1000 else 1):
        env = _envelope(T, 1000 * wi + seed)
        for norm in (True, False):
            x = R.normalize(env) if norm else env.astype(np.float64)
            if T == 1 and norm:
                assert len(_device_peaks(env, normalize=True, **pk)) == 0
                continue
            W = pk["pre_avg"] + pk["post_avg"]
            unsure = R.unsure_mean(x, pk["pre_avg"], pk["post_avg"], pk["delta"], (W + 4) * 2.0 ** -24)
            if not unsure.any():
                want = R.peak_pick(x, **pk)
                got = _device_peaks(env, normalize=norm, **pk)
                assert np.array_equal(got, want), (T, wi, seed, norm, got[:10], want[:10])
            else:                                  # candidate flags (wait = 0) on the sure frames only
                cand = R.peak_candidates(x, pk["pre_max"], pk["post_max"], pk["pre_avg"], pk["post_avg"], pk["delta"])
                got = np.zeros(T, dtype=bool)
                got[_device_peaks(env, normalize=norm, **dict(pk, wait=0))] = True
                assert np.array_equal(got[~unsure], cand[~unsure]), (T, wi, seed, norm)


def test_peaks_degenerate_clips_and_batch():
    pk = WINDOWS[0]
    T = 200
    E = np.stack([_envelope(T, 1), np.zeros(T, np.float32), _envelope(T, 2), np.full(T, 0.3, np.float32), _envelope(T, 3)])
    E[2, 17] = np.nan
    E[4, 100] = np.inf
    fr, cnt = ops.onset_peaks(ops.to_device_f32(E), **pk)
    cnt = cnt.cpu().numpy()
    assert cnt[1] == 0 and cnt[2] == 0 and cnt[3] == 0 and cnt[4] == 0 and cnt[0] > 0
    assert (fr[1:].cpu().numpy() == -1).all()
    assert np.array_equal(fr[0, :cnt[0]].cpu().numpy(), R.peak_pick(R.normalize(E[0]), **pk))
    fr2, cnt2 = ops.onset_peaks(ops.to_device_f32(E), **pk)
    assert torch.equal(fr, fr2) and torch.equal(cnt2, torch.as_tensor(cnt, device=cnt2.device))


def test_peaks_sliced_clips_in_a_batch():
    """More than 4096 frames: flags from several workgroups a clip, then the pick; degenerate rows stay empty."""
    pk = WINDOWS[1]
    T = 9001
    E = np.stack([_envelope(T, 21), _envelope(T, 22), np.zeros(T, np.float32), _envelope(T, 23)])
    E[1, 8000] = np.inf
    fr, cnt = ops.onset_peaks(ops.to_device_f32(E), backtrack=True, **pk)
    fr, cnt = fr.cpu().numpy(), cnt.cpu().numpy()
    assert cnt[1] == 0 and cnt[2] == 0 and (fr[1:3] == -1).all()
    for i in (0, 3):
        x = R.normalize(E[i])
        W = pk["pre_avg"] + pk["post_avg"]
        assert not R.unsure_mean(x, pk["pre_avg"], pk["post_avg"], pk["delta"], (W + 4) * 2.0 ** -24).any()
        assert np.array_equal(fr[i, :cnt[i]], R.backtrack(R.peak_pick(x, **pk), x))
        assert (fr[i, cnt[i]:] == -1).all()


def test_wait_and_backtrack_on_the_device():
    x = np.zeros(40, np.float32)
    x[10], x[13] = 1.0, 0.9
    kw = dict(pre_max=1, post_max=1, pre_avg=2, post_avg=2, delta=0.1)
    assert _device_peaks(x, wait=3, **kw).tolist() == [10]
    assert _device_peaks(x, wait=2, **kw).tolist() == [10, 13]
    e = np.array([0.5, 0.2, 0.2, 0.6, 1.0, 0.4, 0.3, 0.9, 0.1, 0.1], np.float32)
    kw = dict(pre_max=1, post_max=2, pre_avg=1, post_avg=1, delta=0.05, wait=0)
    assert _device_peaks(e, **kw).tolist() == [4, 7]
    assert _device_peaks(e, backtrack=True, **kw).tolist() == [2, 6]
    for seed in range(4):
        env = _envelope(700, 50 + seed)
        en = _envelope(700, 90 + seed)
        x = R.normalize(env)
        on = R.peak_pick(x, **WINDOWS[1])
        assert np.array_equal(_device_peaks(env, backtrack=True, **WINDOWS[1]), R.backtrack(on, x))
        got = ops.onset_peaks(ops.to_device_f32(env[None]), backtrack=True, energy=ops.to_device_f32(en[None]), **WINDOWS[1])
        assert np.array_equal(got[0][0, :int(got[1][0])].cpu().numpy(), R.backtrack(on, en))


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("sr,hop,L", R.E2E_CASES)
def test_detect_onsets_batch_end_to_end(sr, hop, L):
    """A clip without an unsure frame (onset_ref.unsure_frames at 10 * tol: a close test counts only where the other test
    is not failed outright, a subset of the frames either closeness alone would mark) must give the restatement's onset
    list exactly; unsure frames are capped at 1 % of the frames and one clip in ten, and the test fails beyond the cap.
    Measured on an MI355X: 0 unsure frames in 650 / 940 / 630, every list equal."""
    Y = R.gpu_clips(sr, L)
    ref = R.e2e_reference(sr, hop, Y)
    ok, figures = R.within_cap([u for _, u in ref])
    print(f"end to end sr={sr} hop={hop}: unsure frames / frames / clips with any / clips = {figures}")
    assert ok, f"unsure frames over the cap: {figures}"
    fr, cnt = F.detect_onsets_batch(Y, sr, hop)
    fr, cnt = fr.cpu().numpy(), cnt.cpu().numpy()
    for i, (on, un) in enumerate(ref):
        got = fr[i, :cnt[i]]
        if not un.any():
            assert np.array_equal(got, on), (sr, i, got, on)
        # the single-clip mirror is the batch row
        if i < 2:
            one = F.detect_onsets(Y[i], sr=sr, hop_length=hop)
            assert one.dtype == np.int64 and np.array_equal(one, got)
    fr2, cnt2 = F.detect_onsets_batch(Y, sr, hop)
    assert np.array_equal(fr2.cpu().numpy(), fr) and np.array_equal(cnt2.cpu().numpy(), cnt)


def test_detect_onsets_units_backtrack_and_envelope_input():
    sr, hop, L = R.E2E_CASES[0]
    y = R.gpu_clips(sr, L)[0]
    env = R.onset_strength(y, sr, hop_length=hop)
    fr = F.detect_onsets(y, sr=sr, hop_length=hop)
    assert np.array_equal(fr, R.onset_detect(onset_envelope=env, sr=sr, hop_length=hop))
    s = F.detect_onsets(y, sr=sr, hop_length=hop, units="samples")
    t = F.detect_onsets(y, sr=sr, hop_length=hop, units="time")
    assert s.dtype == np.int64 and np.array_equal(s, fr * hop)
    assert t.dtype == np.float64 and np.array_equal(t, fr * hop / float(sr))
    # a given envelope (float32 values, so that both sides read the same numbers)
    e32 = env.astype(np.float32)
    for bt in (False, True):
        want = R.onset_detect(onset_envelope=e32, sr=sr, hop_length=hop, backtrack_=bt)
        assert np.array_equal(F.detect_onsets(onset_envelope=e32, sr=sr, hop_length=hop, backtrack=bt), want)
    want = R.onset_detect(onset_envelope=e32, sr=sr, hop_length=hop, delta=0.2, wait=5, normalize_=False)
    assert np.array_equal(F.detect_onsets(onset_envelope=e32, sr=sr, hop_length=hop, delta=0.2, wait=5, normalize=False), want)
    assert len(F.detect_onsets(np.zeros(L), sr=sr)) == 0
    assert F.detect_onsets(np.zeros(L), sr=sr, units="time").dtype == np.float64
    click = np.zeros(L)
    click[11025] = 1.0
    on = F.detect_onsets(click, sr=sr)
    assert len(on) == 1 and abs(int(on[0]) - round(11025 / hop)) <= 1


# ---------------------------------------------------------------- metrics and segmentation
def test_get_basic_audio_metrics():
    rng = np.random.default_rng(2)
    y = 0.3 * rng.standard_normal(48000)
    m = F.get_basic_audio_metrics(y, 48000)
    assert set(m) == {"duration_seconds", "rms_global", "peak_amplitude"} and all(isinstance(v, float) for v in m.values())
    assert m["duration_seconds"] == 1.0
    assert abs(m["rms_global"] - np.sqrt(np.mean(y ** 2))) <= TOL * np.sqrt(np.mean(y ** 2))
    assert abs(m["peak_amplitude"] - np.abs(y).max()) <= TOL * np.abs(y).max()
    st = np.stack([y, 0.5 * rng.standard_normal(48000)])            # channels first: mono by the mean
    mono = st.mean(axis=0)
    for arr in (st, st.T):
        m2 = F.get_basic_audio_metrics(arr, 48000)
        assert abs(m2["rms_global"] - np.sqrt(np.mean(mono ** 2))) <= TOL * np.sqrt(np.mean(mono ** 2))
        assert abs(m2["peak_amplitude"] - np.abs(mono).max()) <= TOL * np.abs(mono).max()
    Y = ops.to_device_f32(rng.standard_normal((5, 100001)))
    out = ops.clip_metrics(Y)
    Yh = Y.cpu().numpy().astype(np.float64)
    assert_parity(out[:, 0].cpu().numpy(), (Yh ** 2).sum(axis=1), TOL, "sum of squares")
    assert np.array_equal(out[:, 1].cpu().numpy(), np.abs(Yh).max(axis=1).astype(np.float32))
    assert torch.equal(out, ops.clip_metrics(Y))


def test_segment_by_silence_matches_restatement():
    c = R.SILENCE_CASE
    y = R.silence_clip(c["sr"])
    rms = R.rms_frames(y, c["frame_length"], c["hop_length"])
    un = R.silence_unsure(rms, c["threshold_db"])
    assert un.sum() <= 0.01 * len(un)
    got = SEG.segment_by_silence(y, c["sr"], c["threshold_db"], frame_length=c["frame_length"], hop_length=c["hop_length"])
    want = SEG._segments_from_rms(rms, len(y), c["sr"], c["hop_length"], c["threshold_db"])
    if not un.any():
        assert got == want
    assert len(want) == 3


def test_segment_by_onsets_feeds_the_formatter():
    sr, hop, L = R.E2E_CASES[0]
    Y = R.gpu_clips(sr, L)
    ref = R.e2e_reference(sr, hop, Y)
    i = next(k for k, (_, u) in enumerate(ref) if not u.any())
    y = Y[i]
    want = SEG.segment_by_event(y, sr, ref[i][0] * hop / float(sr))
    got = SEG.segment_by_onsets(y, sr, hop_length=hop)
    assert got == want and len(got) >= 2
    from sygnals_amd.core.ml_utils.formatters import format_feature_vectors_per_segment
    feats = {"a": np.arange(L, dtype=np.float64), "b": np.ones(L)}
    X = format_feature_vectors_per_segment(feats, got, output_format="numpy")
    assert X.shape == (len(got), 2) and np.isfinite(X).all()
