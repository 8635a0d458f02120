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


# ---------------------------------------------------------------- the parameter sweep's tables (tests/onset_cases.py)
def test_flux_envelope_is_the_restatement_in_both_paddings():
    from tests import onset_cases as C
    rng = np.random.default_rng(8)
    S = 10.0 * rng.standard_normal((7, 40))
    for lag, k, det in ((1, 1, False), (2, 3, True), (39, 1, False), (3, 12, True)):
        for hop, extra in ((512, 2), (64, 16), (2048, 0)):
            want = R.onset_strength_from_db(S, 2048, hop, lag, k, True, det)
            assert np.array_equal(R.flux_envelope(S, lag, k, lag + extra, 40, det), want)
        want = R.onset_strength_from_db(S, 2048, 512, lag, k, False, det)
        assert np.array_equal(R.flux_envelope(S, lag, k, lag, None, det), want) and len(want) == 40
        assert len(R.flux_envelope(S, lag, k, lag + 2, None, det)) == 42
    assert C.FLUX_SLICED_FROM == 2049


def test_flux_table_reaches_every_value_and_both_sides_of_every_switch():
    from tests import onset_cases as C
    cases = C.flux_cases()
    assert 200 <= len(cases) <= 500 and len({C.flux_id(c) for c in cases}) == len(cases)
    assert {c.M for c in cases} == set(C.FLUX_M) and {c.T for c in cases} == set(C.FLUX_T)
    assert {c.top_db for c in cases} == set(C.FLUX_TOP_DB) and {c.amin for c in cases} == set(C.FLUX_AMIN)
    for T in C.FLUX_T:                     # every frame count with every (lag, max_size) it admits, and with every M
        here = [c for c in cases if c.T == T]
        assert {c.M for c in here} == set(C.FLUX_M)
        assert {c.detrend for c in here} == {False, True}
        for lag, k in C.FLUX_LAGK:
            lag_ = T - 1 if lag == "T-1" else lag
            if lag_ < T:
                assert any(c.lag == lag_ and (c.max_size == k or not isinstance(k, int)) for c in here), (T, lag, k)
    assert any(c.max_size == c.M for c in cases) and any(c.max_size == c.M + 5 for c in cases)
    assert any(c.lag == c.T - 1 and c.T > 2048 for c in cases) and any(c.lag >= 64 and c.max_size > 1 for c in cases)
    # the one-workgroup / sliced switch, a slice of output frames and a slice of the partial maximum, from both sides
    assert {2047, 2048, 2049} <= set(C.FLUX_T) and {2303, 2304, 2305} <= set(C.FLUX_T) and {3071, 3072, 3073} <= set(C.FLUX_T)
    outs = {(c.pad + c.T - c.lag if c.T_out is None else c.T_out) for c in cases if c.T >= C.FLUX_SLICED_FROM}
    assert {2303, 2304, 2305, 2306, 2307} <= outs                    # T_out at 9 * 256 - 1 ... + 3
    assert any(c.T_out is None and c.pad == c.lag and c.T >= C.FLUX_SLICED_FROM for c in cases)   # center=False, sliced
    assert all(c.B == 3 for c in cases if c.T >= C.FLUX_SLICED_FROM)
    assert any(c.detrend and c.B == 3 and c.T in (63, 64, 65) for c in cases)
    for c in cases[::40]:                  # the inputs are the long-clip test's: float32, a different clip per row
        P = C.flux_power(c)
        assert P.dtype == np.float32 and P.shape == (c.B, c.M, c.T) and (c.B == 1 or not np.array_equal(P[0], P[1]))
        S = np.stack([np.zeros((c.M, c.T)), np.full((c.M, c.T), -19.1)])
        assert all(not R.flux_envelope(s, c.lag, c.max_size, c.pad, c.T_out, c.detrend).any() for s in S)


def test_mirror_table_names_the_front_end_that_serves_each_row():
    """What can be decided without a device: which frame lengths have a segment-sum table for the filterbank (the packers
    of sygnals_amd._tables raise ValueError when they have none), which the fused power-of-two kernel takes and which
    filterbanks the fused 2048 kernel has a plan for.  tests/test_gpu_onset_params.py spies on the call for every row."""
    from sygnals_amd import ops, _tables as T
    from tests import onset_cases as C
    cases = C.mirror_cases()
    assert {c.front for c in cases} == set(C.FRONT_ENDS)
    assert {c.n_fft // (2 * c.hop) for c in cases} == {0, 1, 2, 16} and {c.n_mels for c in cases} == {40, 128}
    for front in C.FRONT_ENDS:
        assert {c.n_fft // (2 * c.hop) for c in cases if c.front == front} >= ({0, 2, 16} if front == "pow2" else {1, 2, 16})
    assert any(c.fmin > 0 and c.fmax is not None for c in cases)

    def has_table(c):
        k = ops._SEG.get(c.n_fft)
        if k is None or c.n_mels > k["max_mels"]:
            return False
        fmax = c.sr / 2.0 if c.fmax is None else c.fmax
        try:
            k["pack"](c.sr, c.n_fft, c.n_mels, c.fmin, fmax, basis=T.mel_filterbank(c.sr, c.n_fft, c.n_mels, c.fmin, fmax),
                      **k["pack_kw"])
            return True
        except ValueError:
            return False
    for c in cases:
        if c.front == "fused2048":             # fused_mel_ok: a block-sparse plan for the filterbank
            fmax = c.sr / 2.0 if c.fmax is None else c.fmax
            assert c.n_fft == 2048 and c.n_mels <= 256
            T.pack_mel_plan(T.mel_filterbank(c.sr, 2048, c.n_mels, c.fmin, fmax), ops.fused_waves())
        elif c.front.startswith("seg"):
            assert c.front == f"seg{c.n_fft}" and has_table(c), C.mirror_id(c)
        elif c.front == "pow2":
            assert not has_table(c) and ops.fused_pow2_ok(c.n_fft, c.n_mels), C.mirror_id(c)
        else:
            assert not has_table(c) and not ops.fused_pow2_ok(c.n_fft, c.n_mels) and c.n_fft != 2048, C.mirror_id(c)


def test_peak_table_reaches_every_size_halo_and_wait():
    from tests import onset_cases as C
    cases = C.peak_cases()
    assert len({C.peak_id(c) for c in cases}) == len(cases)
    assert {c.T for c in cases} == set(C.PEAK_T)
    for T in C.PEAK_T:
        assert {c.wait for c in cases if c.T == T} >= {0, 1, 62, 63, 64, 65, 200, T + 1}
    halos = {(max(c.pre_max, c.pre_avg), max(c.post_max, c.post_avg)) for c in cases}
    assert {(a, b) for a in C.PEAK_HALO for b in C.PEAK_HALO if (a, b) != (1, 1)} <= halos
    for T in (255, 256, 257, 1024, 1025, 4095, 4096, 4097, 8192, 8193):     # every halo pair on every such size
        here = {(max(c.pre_max, c.pre_avg), max(c.post_max, c.post_avg)) for c in cases if c.T == T}
        assert {(257, 1), (1, 257), (256, 256), (257, 256), (256, 257), (257, 257), (255, 255)} <= here
    wide = [c for c in cases if max(c.pre_max, c.pre_avg, c.post_max, c.post_avg) > 200]
    assert all(c.T <= C.PEAK_WIDE_T_MAX for c in wide)
    assert any(c.pre_max >= 255 for c in wide) and any(c.pre_avg >= 255 for c in wide)
    assert any(c.post_max >= 255 for c in wide) and any(c.post_avg >= 255 for c in wide)
    assert {c.kind for c in cases} == set(C.GRID_KINDS) | {"smooth"}
    for T in (4096, 4097, 131072, 131073):
        assert any(c.T == T and c.kind == "plateau" and c.wait == 0 and c.delta == 0.0 for c in cases)
    for c in cases:
        assert c.post_max >= 1 and c.post_avg >= 1 and min(c.pre_max, c.pre_avg) >= 0


def test_grid_envelopes_are_on_the_grid_and_say_what_their_names_say():
    """Multiples of 2^-10 in [-1, 1]: a window sum is an integer multiple of 2^-10 below 2^18, exact in float64 in any
    order, so the restatement's own answer does not depend on how it sums."""
    from tests import onset_cases as C
    for kind in C.GRID_KINDS:
        for T in (1, 2, 257, 4097):
            e = C.grid_envelope(kind, T, 5)
            q = e.astype(np.float64) / C.GRID
            assert e.dtype == np.float32 and e.shape == (T,) and np.array_equal(q, np.round(q)) and np.abs(e).max() <= 1.0
    e = C.grid_envelope("plateau", 300, 0)
    assert (e == e[0]).all() and e[0] != 0
    assert R.peak_pick(e.astype(np.float64), 1, 1, 4, 5, 0.0, 0).tolist() == list(range(300))   # every frame a candidate
    assert (C.grid_envelope("negative", 300, 0) < 0).all()
    z = C.grid_envelope("zero-run", 4097, 0)
    runs = np.flatnonzero(np.diff(np.concatenate(([0], (z == 0).astype(np.int8), [0]))))
    assert (z == 0).any() and (z != 0).any() and (runs[1::2] - runs[0::2]).max() >= 5
    x = z.astype(np.float64)                       # a zero that passes the maximum and the mean test is still no peak
    mx, av = R.peak_terms(x, 3, 2, 0, 1)
    assert ((x == 0) & (x == mx) & (x >= av)).any() and not (R.peak_candidates(x, 3, 2, 0, 1, 0.0) & (x == 0)).any()
    s = C.grid_envelope("stairs", 4097, 0).astype(np.float64)
    mx, _ = R.peak_terms(s, 3, 2, 1, 1)
    assert any((s[max(0, n - 3):n + 2] == mx[n]).sum() > 1 for n in range(100))     # a repeated maximum inside a window
    up, down = C.grid_envelope("ramp-up", 4097, 0), C.grid_envelope("ramp-down", 4097, 0)
    assert up[-1] > up[-2] and down[0] > down[1] and (up != 0).all()


def test_peak_smooth_rows_stay_within_the_cap():
    """The seeded smooth envelopes of group C, restatement alone: at most 1 % of a row's frames within (W + 4) 2^-24 of the
    mean test's threshold, and at most one row in ten with any such frame."""
    from tests import onset_cases as C
    rows = [c for c in C.peak_cases() if c.kind == "smooth" and c.T > 1]
    marked = 0
    for c in rows:
        env, norm = C.peak_envelope(c)
        assert norm and env.dtype == np.float32
        un = R.unsure_mean(R.normalize(env), c.pre_avg, c.post_avg, c.delta, R.peak_margin(c.pre_avg, c.post_avg))
        assert un.sum() <= 0.01 * c.T, (C.peak_id(c), int(un.sum()))
        marked += bool(un.any())
    assert len(rows) >= 100 and 1 <= marked <= 0.1 * len(rows), (marked, len(rows))


def test_e2e_table_is_within_the_cap_by_the_restatement_alone():
    from tests import onset_cases as C
    assert len(C.e2e_cases()) == len(C.E2E_CASES) * len(C.E2E_PEAK_ARGS) + len(C.E2E_BACKTRACK) * len(C.E2E_PEAK_ARGS)
    total = {}
    for sr, hop, L in C.E2E_CASES:
        Y = R.gpu_clips(sr, L)
        for ai, peak in enumerate(C.E2E_PEAK_ARGS):
            ref = R.e2e_reference_with(sr, hop, Y, **peak)
            ok, figures = R.within_cap([u for _, u in ref])
            assert ok, (sr, hop, L, peak, figures)
            assert all(len(o) >= 1 for o, _ in ref), (sr, hop, L, peak)
            total[(sr, hop, L, ai)] = figures[0]
            if not peak:                           # the defaults are e2e_reference's
                base = R.e2e_reference(sr, hop, Y)
                assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(ref, base))
    assert sum(total.values()) <= 4, total


def test_short_clips_in_the_restatement():
    """No more frames than `lag`: the flux is empty and the envelope is its padding."""
    from tests import onset_cases as C
    for sr, hop in C.SHORT_SR_HOP:
        for L in C.short_lengths(hop):
            y = np.random.default_rng(L).standard_normal(L)
            T = 1 + L // hop
            for lag in C.SHORT_LAGS:
                e = R.onset_strength(y, sr, hop_length=hop, lag=lag)
                assert e.shape == (T,) and (T > lag or not e.any())
            assert len(R.onset_detect(y, sr=sr, hop_length=hop)) == 0
    e = R.onset_strength(np.zeros(100), 22050)
    assert e.tolist() == [0.0] and len(R.onset_detect(np.zeros(100), sr=22050)) == 0
    y = np.random.default_rng(0).standard_normal(2048 + 1024)       # three frames without centre padding, lag 4
    assert R.onset_strength(y, 22050, lag=4, center=False).tolist() == [0.0] * 4


def test_silence_parameter_sets_are_clear_of_the_threshold():
    from sygnals_amd.core.segmentation import _segments_from_rms
    from tests import onset_cases as C
    assert len(C.SILENCE_CASES) == len(C.SILENCE_SEGMENTS)
    assert {c["threshold_db"] for c in C.SILENCE_CASES} == {-20.0, -60.0}
    assert any(c["hop_length"] is None for c in C.SILENCE_CASES)
    assert len({(c["frame_length"], c["hop_length"]) for c in C.SILENCE_CASES} - {(512, 128)}) >= 2
    for c, n in zip(C.SILENCE_CASES, C.SILENCE_SEGMENTS):
        hop = c["hop_length"] if c["hop_length"] is not None else c["frame_length"] // 4
        y = R.silence_clip(c["sr"])
        rms = R.rms_frames(y, c["frame_length"], hop)
        un = R.silence_unsure(rms, c["threshold_db"])
        assert un.sum() <= 0.01 * len(un), c
        kw = C.silence_kwargs(c)
        segs = _segments_from_rms(rms, len(y), c["sr"], hop, **kw)
        assert len(segs) == n, (c, segs)
        plain = _segments_from_rms(rms, len(y), c["sr"], hop, threshold_db=c["threshold_db"])
        assert len(plain) == 3                     # what the extra argument changes is the gap, not the passages
