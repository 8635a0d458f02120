"""The float64 restatement of the rhythm family against NumPy / SciPy forms of the same definitions, its edge rules, and
the conditions the GPU tests' inputs must meet (tests/beat_cases.py)."""
import numpy as np
import pytest
import scipy.signal

from tests import beat_cases as K
from tests import beat_ref as R


def _rand_env(T, seed):
    return np.random.default_rng(seed).random(T).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ tempogram
@pytest.mark.parametrize("win,T,center", [(8, 20, True), (9, 20, True), (8, 20, False), (64, 3, True), (3, 1, True), (2, 5, True)])
def test_tempogram_is_np_correlate_of_the_windowed_frame(win, T, center):
    env = _rand_env(T, win + T)
    r = R.autocorr(env, win, center)
    p = win // 2
    xp = np.pad(env.astype(np.float64), p, mode="linear_ramp", end_values=0) if center else env.astype(np.float64)
    w = R.window32("hann", win)
    assert r.shape == (win, T if center else T - win + 1)
    for t in range(r.shape[1]):
        f = w * xp[t:t + win]
        assert np.allclose(r[:, t], np.correlate(f, f, "full")[win - 1:], rtol=1e-13, atol=1e-15)
    tg = R.tempogram(env, win, center)
    assert np.array_equal(tg, r / np.max(np.abs(r), axis=0)) and np.all(tg[0] == 1.0)
    assert np.array_equal(R.tempogram(env, win, center, norm=None), r)


@pytest.mark.parametrize("T,p", [(1, 1), (1, 4), (5, 3), (7, 192)])
def test_pad_is_np_pad_linear_ramp(T, p):
    env = _rand_env(T, 10 * T + p).astype(np.float64) + 0.25
    assert np.allclose(R.pad_ramp(env, p), np.pad(env, p, mode="linear_ramp", end_values=0), rtol=4e-16, atol=0)
    assert R.pad_ramp(env, p)[0] == 0.0 and R.pad_ramp(env, p)[p] == env[0]
    assert R.pad_ramp(env, p)[-1] == 0.0 and len(R.pad_ramp(env, p)) == T + 2 * p


def test_tempogram_refuses_too_few_frames_and_leaves_tiny_columns():
    with pytest.raises(ValueError):
        R.autocorr(np.ones(7), 8, center=False)
    assert R.autocorr(np.ones(8), 8, center=False).shape == (8, 1)
    z = R.tempogram(np.zeros(6), 4)
    assert z.shape == (4, 6) and not z.any()
    t = R.tempogram(np.full(6, 1e-25), 4)                         # r ~ 1e-50 is below the smallest normal float32
    assert np.all(np.abs(t) < R.TINY) and t.any()


# ---------------------------------------------------------------------------------------------------------------- tempo
@pytest.mark.parametrize("sr,hop", [(22050, 512), (48000, 512), (48000, 256), (16000, 160)])
def test_the_period_of_a_lag_is_the_lag(sr, hop):
    win = min(2048, int(np.floor(8.0 * sr / hop)))
    bpms, lp = R.prior(win, sr, hop)
    k = np.arange(1, win)
    assert np.array_equal(np.round(60.0 * (sr / hop) / bpms[1:]).astype(int), k)
    assert all(R.period_of(bpms[j], sr, hop) == j for j in (1, 2, 3, win - 1))
    assert bpms[0] == np.inf and lp[0] == -np.inf
    first = int(np.argmax(bpms < 320.0))
    assert np.all(lp[:first] == -np.inf) and np.all(np.isfinite(lp[first:])) and bpms[first] < 320.0 <= bpms[first - 1]
    assert np.all(np.isfinite(R.prior(win, sr, hop, max_tempo=None)[1][1:]))


@pytest.mark.parametrize("P", [12, 20, 24, 31, 43])
def test_click_tracks_give_their_lag_or_twice_it(P):
    env = R.click_envelope(400, P, 5, 1.0, 0.1, P)
    bpm, k = R.tempo(env, K.SR, K.HOP)
    assert k in (P, 2 * P) and bpm == 60.0 * K.SR / (K.HOP * k)
    beats = R.beat_track(env, P)
    assert len(beats) >= 400 // P - 4 and np.all(np.diff(beats) == P) and np.all((beats - 5) % P == 0)
    per_frame, ks = R.tempo(env[:60], K.SR, K.HOP, aggregated=False)
    assert per_frame.shape == (60,) and np.array_equal(per_frame, R.prior(K.WIN, K.SR, K.HOP)[0][ks])


def test_all_zero_rows_have_no_tempo_and_no_beats():
    z = np.zeros(50, dtype=np.float32)
    assert R.tempo(z, K.SR, K.HOP) == (0.0, 0)
    assert not R.tempo(z, K.SR, K.HOP, aggregated=False)[0].any()
    assert len(R.beat_track(z, 20)) == 0 and R.chain(z, K.SR, K.HOP) [0] == 0.0 and R.chain(z, K.SR, K.HOP, bpm=100.0)[0] == 0.0
    assert len(R.beat_track(np.ones(50), 1)) == 0                 # a period below 2: no beats


# ---------------------------------------------------------------------------------------------------------- local score
@pytest.mark.parametrize("T,P", [(1, 2), (2, 2), (5, 7), (40, 3), (100, 21)])
def test_local_score_is_scipy_convolve_same(T, P):
    env = _rand_env(T, T + P)
    e = R.scaled(env)
    want = scipy.signal.convolve(e, R.taps(P), "same", method="direct")
    assert np.allclose(R.local_score(env, P), want, rtol=1e-12, atol=1e-14)
    if T >= 2:
        assert np.allclose(e, env.astype(np.float64) / np.std(env.astype(np.float64), ddof=1))
    assert np.array_equal(R.scaled(np.full(9, 3.0)), np.full(9, 3.0))            # a constant row is not divided
    assert np.array_equal(R.scaled(np.array([2.0])), np.array([2.0]))            # nor is a single frame


# ------------------------------------------------------------------------------------------------------------------- DP
@pytest.mark.parametrize("P", list(range(2, 41)))
def test_explicit_dp_is_the_negative_index_form_bit_for_bit(P):
    rng = np.random.default_rng(P)
    T = int(rng.integers(2 * P + 3, 6 * P + 40))
    ls = (rng.standard_normal(T) + 0.5).astype(np.float32)
    for tight in (1.0, 100.0, 400.0):
        c0, b0 = R.dp(ls, P, tight)
        c1, b1 = R.dp_negative_index(ls, P, tight)
        c2, b2 = R.dp_vector(ls, P, tight)
        assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and np.array_equal(c0, c2) and np.array_equal(b0, b2)
    o = R.offsets(P)
    assert o[0] == -2 * P and o[-1] == -int(np.round(P / 2)) and np.all(np.diff(o) == 1)
    assert np.allclose(R.transition(P, 100.0), -100.0 * np.log(-o / P) ** 2, rtol=0, atol=1e-11)
    assert R.transition(P, 100.0)[P] == 0.0                       # offset -P costs nothing


def test_back_links_wait_for_the_first_beat():
    ls = np.zeros(40, dtype=np.float32)
    ls[17] = 1.0
    ls[10] = 0.005                                                # below a hundredth of the maximum
    cum, back = R.dp(ls, 4)
    assert np.all(back[:17] == -1) and back[17] == 17 - 4 and np.all(back[18:] >= 0) and np.all(back[18:] < np.arange(18, 40))
    ls[2] = 0.5
    assert R.dp(ls, 4)[1][2] == 2 - 4 and R.dp(ls, 4)[1][1] == -1           # a link may point before the clip: it ends a walk
    assert np.array_equal(R.backtrack(np.array([-1, -3, 0, 1]), 3), [1, 3])


# ----------------------------------------------------------------------------------------------------- last beat, trim
def test_local_maxima_and_last_beat_edges():
    assert not R.local_maxima(np.array([5.0])).any() and R.last_beat(np.array([5.0])) == -1                 # T = 1
    assert not R.local_maxima(np.full(6, 2.0)).any() and R.last_beat(np.full(6, 2.0)) == -1                # constant
    assert not R.local_maxima(np.arange(5.0)[::-1]).any()                                                  # falling: none
    assert np.array_equal(R.local_maxima(np.array([0.0, 1.0, 1.0, 0.0, 2.0])), [False, True, False, False, True])
    assert not R.local_maxima(np.array([3.0, 1.0]))[0]                                                     # frame 0 never
    c = np.array([0.0, 4.0, 0.0, 10.0, 0.0, 3.0, 0.0, 4.5, 0.0])     # maxima 4, 10, 3, 4.5: median 4.25; 2 * 3 > 4.25
    assert R.last_beat(c) == 7 and R.last_beat(c[:6]) == 5
    c = np.array([0.0, -4.0, -9.0, -3.0, -9.0])                       # a negative median: 2 cum lm = 0 passes at any frame
    assert np.median(c[R.local_maxima(c)]) < 0 and R.last_beat(c) == 4
    assert len(R.beats_from(np.ones(1, dtype=np.float32), 3)[0]) == 0
    assert len(R.beats_from(np.zeros(30, dtype=np.float32), 3)[0]) == 0


def test_trim_rules_and_the_exclusive_upper_end():
    ls = np.zeros(100, dtype=np.float32)
    b = np.arange(5, 100, 10)
    ls[b] = [0.01, 1, 1, 1, 1, 1, 1, 1, 0.01, 0.01]
    sm = R.smooth(ls, b)
    f = np.float64(np.float32(0.01))
    assert sm[0] == (0.5 * 0.0 + f) + 0.5 * 1.0 and sm[-1] == (0.5 * f + f) + 0.0 and sm[8] == (0.5 * 1.0 + f) + 0.5 * f
    th = 0.5 * np.sqrt(np.cumsum(sm * sm)[-1] / 10)
    v = np.flatnonzero(sm > th)
    assert v.min() == 1 and v.max() == 7                                         # 0.51 and 0.515 are under th, about 0.6
    assert np.array_equal(R.trim_beats(ls, b), b[1:7])                           # beat 7 passes and is dropped
    assert np.array_equal(R.trim_beats(ls, b, trim=False), b[:9])                # th = 0: all pass, the last one goes
    assert len(R.trim_beats(np.zeros(100, dtype=np.float32), b)) == 0            # nothing above the threshold
    assert len(R.trim_beats(ls, b[:1])) == 0 and len(R.trim_beats(ls, b[:0])) == 0


# ------------------------------------------------------------------------------------------- what the GPU tests rely on
@pytest.mark.parametrize("name", sorted(K.ENV_CASES))
def test_end_to_end_inputs_meet_both_conditions(name):
    ref = K.reference(name)
    P = K.ENV_CASES[name][1]
    assert ref["k"] in (P, 2 * P)
    assert K.condition_a(ref["a"], ref["logprior"])
    assert K.condition_b(ref["env"], ref["k"]) and K.condition_b(ref["env"], ref["k"], trim=False)
    assert len(ref["beats"]) >= 5 and np.all(np.diff(ref["beats"]) > 0)
    bpm, beats = R.chain(ref["env"], K.SR, K.HOP)
    assert bpm == ref["tempo"] and np.array_equal(beats, ref["beats"])
    given = R.period_of(110.0, K.SR, K.HOP)
    assert K.condition_b(ref["env"], given)


def test_conditions_reject_what_they_should():
    lp = R.prior(16, K.SR, K.HOP, max_tempo=None)[1]
    a = np.zeros(16)
    a[5] = a[6] = 0.5
    assert not K.condition_a(a, np.where(np.isfinite(lp), 0.0, lp))               # two equal lags: no margin
    a[6] = 0.1
    assert K.condition_a(a, np.where(np.isfinite(lp), 0.0, lp))
