"""The float64 restatement of tests/onset_ref.py against the form librosa 0.10.0 writes and against closed forms, the host
rules of sygnals_amd.core.segmentation against hand-computed index lists, and the fixture check of the GPU tests'
inputs.  No device."""
import numpy as np
import pytest
import scipy.ndimage

from tests import onset_ref as R


# ---------------------------------------------------------------- peak_pick: explicit windows == the scipy-filter form
@pytest.mark.parametrize("sr,hop", [(22050, 512), (48000, 512), (16000, 256)])
def test_peak_pick_matches_scipy_filter_form(sr, hop):
    pk = R.default_windows(sr, hop)
    for seed in range(30):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(40, 400))
        # a smooth positive envelope with peaks: rectified, smoothed noise, normalised like onset_detect does
        x = R.normalize(np.convolve(np.maximum(rng.standard_normal(n + 4), 0.0) ** 2, np.hanning(5), mode="valid"))
        a = R.peak_pick(x, **pk)
        b = R.peak_pick_scipy(x, **pk)
        assert np.array_equal(a, b), (seed, a, b)
        assert len(a) > 0


def test_peak_pick_rejects_what_librosa_rejects():
    x = np.linspace(0, 1, 10)
    for kw in (dict(pre_max=-1), dict(post_max=0), dict(pre_avg=-1), dict(post_avg=0), dict(delta=-0.1), dict(wait=-1)):
        args = dict(pre_max=1, post_max=1, pre_avg=1, post_avg=1, delta=0.0, wait=0)
        args.update(kw)
        with pytest.raises(ValueError):
            R.peak_pick(x, **args)


def test_default_windows_are_pinned():
    want = {(22050, 512): (1, 1, 4, 5, 1), (48000, 512): (2, 1, 9, 10, 2), (16000, 256): (1, 1, 6, 7, 1)}
    for (sr, hop), w in want.items():
        pk = R.default_windows(sr, hop)
        assert (pk["pre_max"], pk["post_max"], pk["pre_avg"], pk["post_avg"], pk["wait"]) == w
        assert pk["delta"] == 0.07
    # the product's own defaults follow the same precedence
    from sygnals_amd.core.audio.features import _peak_defaults
    for (sr, hop), w in want.items():
        pk = _peak_defaults(sr, hop, {})
        assert (pk["pre_max"], pk["post_max"], pk["pre_avg"], pk["post_avg"], pk["wait"]) == w
        assert all(isinstance(pk[k], int) for k in ("pre_max", "post_max", "pre_avg", "post_avg", "wait"))


def test_superflux_reference_is_the_clipped_running_maximum():
    """maximum_filter1d's reflected edges only repeat values of the clipped window (what the kernel takes)."""
    rng = np.random.default_rng(3)
    for M, k in ((128, 3), (128, 4), (7, 5), (3, 7), (5, 2), (1, 3)):
        S = rng.standard_normal((M, 6))
        want = scipy.ndimage.maximum_filter1d(S, k, axis=0)
        got = np.stack([S[max(0, m - k // 2):min(M, m - k // 2 + k)].max(axis=0) for m in range(M)])
        assert np.array_equal(got, want), (M, k)


# ---------------------------------------------------------------- closed-form anchors
@pytest.mark.parametrize("pos", [5000, 11025, 16400])
def test_one_click_in_silence(pos):
    sr, hop = 22050, 512
    y = np.zeros(22050)
    y[pos] = 1.0
    on = R.onset_detect(y, sr=sr, hop_length=hop)
    assert len(on) == 1 and abs(int(on[0]) - round(pos / hop)) <= 1, on


def test_all_zero_input_gives_nothing():
    for units in ("frames", "samples", "time"):
        assert len(R.onset_detect(np.zeros(22050), sr=22050, units=units)) == 0
    assert len(R.onset_detect(onset_envelope=np.zeros(50), sr=22050)) == 0
    env = np.ones(50)
    env[7] = np.inf
    assert len(R.onset_detect(onset_envelope=env, sr=22050)) == 0


def test_wait_suppresses_the_second_of_two_close_candidates():
    x = np.zeros(40)
    x[10] = 1.0
    x[13] = 0.9
    kw = dict(pre_max=1, post_max=1, pre_avg=2, post_avg=2, delta=0.1)
    assert R.peak_pick(x, wait=3, **kw).tolist() == [10]          # 13 is `wait` after 10
    assert R.peak_pick(x, wait=2, **kw).tolist() == [10, 13]      # and wait + 1 after it here


def test_backtrack_on_a_hand_written_envelope():
    #            0    1    2    3    4    5    6    7    8    9
    e = np.array([0.5, 0.2, 0.2, 0.6, 1.0, 0.4, 0.3, 0.9, 0.1, 0.1])
    assert R.local_minima(e).tolist() == [0, 2, 6]                # 8 is not below its right neighbour, 9 has none
    assert R.backtrack([4, 7, 9, 1, 0], e).tolist() == [2, 6, 6, 0, 0]
    on = R.onset_detect(onset_envelope=e, sr=22050, pre_max=1, post_max=2, pre_avg=1, post_avg=1, delta=0.05, wait=0)
    assert on.tolist() == [4, 7]
    bt = R.onset_detect(onset_envelope=e, sr=22050, backtrack_=True, pre_max=1, post_max=2, pre_avg=1, post_avg=1,
                        delta=0.05, wait=0)
    assert bt.tolist() == [2, 6]


def test_units():
    e = np.zeros(30)
    e[12] = 1.0
    assert R.onset_detect(onset_envelope=e, sr=16000, hop_length=256, units="samples").tolist() == [12 * 256]
    assert R.onset_detect(onset_envelope=e, sr=16000, hop_length=256, units="time").tolist() == [12 * 256 / 16000]


def test_envelope_padding_and_trim():
    sr, n_fft, hop = 22050, 2048, 512
    y = R.burst_clip(sr, 9000, 1)
    T = 1 + 9000 // hop
    e = R.onset_strength(y, sr)
    assert e.shape == (T,) and (e[:3] == 0).all()                 # lag + n_fft // (2 hop) = 3 zeros in front
    e2 = R.onset_strength(y, sr, lag=2)
    assert e2.shape == (T,) and (e2[:4] == 0).all()
    e3 = R.onset_strength(y, sr, center=False)
    assert e3.shape == (1 + (9000 - n_fft) // hop,) and e3[0] == 0
    d = R.onset_strength(y, sr, detrend=True)
    assert d.shape == (T,) and abs(d[3] - e[3]) < 1e-12 and not np.allclose(d, e)


# ---------------------------------------------------------------- segmentation (host rules)
def test_segment_fixed_length():
    from sygnals_amd.core.segmentation import segment_fixed_length
    y = np.arange(10, dtype=np.float64)
    s = segment_fixed_length(y, 1, 4.0)
    assert [a.tolist() for a in s] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 0, 0]]
    s = segment_fixed_length(y, 1, 4.0, pad=False)                # the tail rule: no partial segment
    assert [a.tolist() for a in s] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    s = segment_fixed_length(y, 1, 4.0, overlap_ratio=0.5)
    assert [int(a[0]) for a in s] == [0, 2, 4, 6, 8] and all(len(a) == 4 for a in s)
    s = segment_fixed_length(y, 1, 4.0, overlap_ratio=0.5, pad=False)
    assert [int(a[0]) for a in s] == [0, 2, 4, 6]
    s = segment_fixed_length(y, 1, 4.0, min_segment_length_sec=3.0)
    assert [a.tolist() for a in s] == [[0, 1, 2, 3], [4, 5, 6, 7]]   # the 2-sample tail is under the minimum
    assert segment_fixed_length(y, 1, 0.5) == []
    assert all(a.dtype == np.float64 for a in segment_fixed_length(y.astype(np.float32), 1, 4.0))
    with pytest.raises(ValueError):
        segment_fixed_length(y, 1, 0.0)
    with pytest.raises(ValueError):
        segment_fixed_length(y, 1, 1.0, overlap_ratio=1.0)
    with pytest.raises(ValueError):
        segment_fixed_length(np.zeros((2, 5)), 1, 1.0)


def test_segment_by_event():
    from sygnals_amd.core.segmentation import segment_by_event
    y = np.zeros(1000)
    ev = np.array([0.01, 0.5, 0.99])
    assert segment_by_event(y, 1000, ev) == [(0, 210), (450, 700), (940, 1000)]
    assert segment_by_event(y, 1000, ev, segment_duration_sec=0.101) == [(0, 61), (450, 551), (940, 1000)]
    assert segment_by_event(y, 1000, np.array([1.5])) == []       # clipped to nothing
    assert segment_by_event(y, 1000, np.array([])) == []
    with pytest.raises(ValueError):
        segment_by_event(y, 1000, ev, pre_event_sec=-1.0)
    with pytest.raises(ValueError):
        segment_by_event(y, 1000, ev, segment_duration_sec=0.0)


def test_segments_from_rms():
    from sygnals_amd.core.segmentation import _segments_from_rms
    sr, hop = 1000, 10
    #      frames:  0-4 loud, 5-19 silent (15), 20-24 loud, 25-27 silent (3: too short to split), 28-39 loud, 40-49 silent
    rms = np.concatenate([np.ones(5), np.zeros(15), np.ones(5), np.zeros(3), np.ones(12), np.zeros(10)])
    kw = dict(threshold_db=-40.0, min_silence_duration_sec=0.1, min_segment_duration_sec=0.0, padding_sec=0.0)
    assert _segments_from_rms(rms, 500, sr, hop, **kw) == [(0, 50), (200, 400)]
    kw["padding_sec"] = 0.02                                      # 20 samples each side, clipped at 0
    assert _segments_from_rms(rms, 500, sr, hop, **kw) == [(0, 70), (180, 420)]
    kw["padding_sec"] = 0.08                                      # (0, 130) and (120, 480) overlap: merged
    assert _segments_from_rms(rms, 500, sr, hop, **kw) == [(0, 480)]
    kw["padding_sec"] = 0.075                                     # (0, 125) and (125, 475) touch: not merged
    assert _segments_from_rms(rms, 500, sr, hop, **kw) == [(0, 125), (125, 475)]
    kw.update(padding_sec=0.0, min_segment_duration_sec=0.06)     # the 50-sample piece is dropped
    assert _segments_from_rms(rms, 500, sr, hop, **kw) == [(200, 400)]
    kw.update(min_segment_duration_sec=0.0, min_silence_duration_sec=0.02)   # now the 3-frame gap splits too
    assert _segments_from_rms(rms, 500, sr, hop, **kw) == [(0, 50), (200, 250), (280, 400)]
    assert _segments_from_rms(np.zeros(20), 200, sr, hop) == []
    assert _segments_from_rms(np.zeros(0), 0, sr, hop) == []
    assert _segments_from_rms(np.ones(20), 195, sr, hop, min_segment_duration_sec=0.0) == [(0, 195)]
    # the threshold is relative to the loudest frame: -40 dB of 1.0 is 0.01
    r2 = np.array([1.0] * 3 + [0.0101] * 12 + [1.0] * 3)
    assert _segments_from_rms(r2, 180, sr, hop, min_segment_duration_sec=0.0, padding_sec=0.0) == [(0, 180)]
    r2[3:15] = 0.0099
    assert _segments_from_rms(r2, 180, sr, hop, min_segment_duration_sec=0.0, padding_sec=0.0) == [(0, 30), (150, 180)]


def test_mirror_argument_errors_need_no_device():
    from sygnals_amd.core.audio.features import detect_onsets, onset_strength_batch
    with pytest.raises(ValueError, match="must be provided"):
        detect_onsets()
    with pytest.raises(ValueError, match="Sampling rate 'sr' must be provided"):
        detect_onsets(np.zeros(100))
    with pytest.raises(ValueError, match="required when units='time'"):
        detect_onsets(onset_envelope=np.zeros(10), units="time")
    with pytest.raises(TypeError, match="unsupported librosa arguments"):
        detect_onsets(np.zeros(100), sr=22050, feature=lambda *a: None)
    with pytest.raises(TypeError, match="not offloaded"):
        onset_strength_batch(np.zeros((1, 100)), 22050, aggregate=np.median)


# ---------------------------------------------------------------- the fixture check
def test_gpu_fixture_has_no_unsure_frames_to_speak_of():
    """Every input of the end-to-end GPU tests, restatement alone: unsure frames within the cap (1 % of frames, one clip
    in ten), and every clip has onsets to find."""
    for sr, hop, L in R.E2E_CASES:
        ref = R.e2e_reference(sr, hop, R.gpu_clips(sr, L))
        ok, figures = R.within_cap([u for _, u in ref])
        assert ok, (sr, hop, figures)
        assert all(len(o) >= 2 for o, _ in ref)


def test_silence_fixture_is_clear_of_the_threshold():
    c = R.SILENCE_CASE
    rms = R.rms_frames(R.silence_clip(c["sr"]), c["frame_length"], c["hop_length"])
    un = R.silence_unsure(rms, c["threshold_db"])
    assert un.sum() <= 0.01 * len(un)
